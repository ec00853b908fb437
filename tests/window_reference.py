"""An fp64 (and wider) reference of `mshgnn_assemble_windows` that reads the DESCRIPTOR TABLES of include/mshgnn.h themselves -- runs [K][n_runs][5],
rows [n_rows][2], label_cols [K][n_label] -- not a `WindowRecipe`, so that it can express what recipes cannot: any first feature, any length <= 256 per
run, rows that mix lengths, features no run covers, up to 128 runs and 12 sources.  It returns, per node type, the expected value of every element of
[B][n_t][pitch], which elements no run covers (they keep the caller's sentinel), which pad columns the chunk kernel zeroes, and a PER-ELEMENT error
bound: 0 for unstandardised data (the gather is a copy), the bound derived below for standardised data and rotated labels.  No tolerance in
tests/test_windows_exact_gpu.py is a measured number; tests/test_window_reference.py shows on the host that the checkers accept an fp64 emulation of
the kernels' arithmetic and reject one mutation per way a gather goes wrong.

Meaning of the tables (include/mshgnn.h; the kernels are k_assemble_windows / k_assemble_windows_fast / window_labels_one):
  run = {type, node, first feature f0, word, length}; word -1: the constant 1; else source = word >> 8, column = word & 255, and with sign_flags bit 0
  bit 30 of the word negates the run (BEFORE the statistics).  x[b][node][f0 + k] = src(row + k, column), k < length.  sign_flags bits 8..15 = K > 1:
  window b takes block min(starts[b] >> 56, K - 1) of runs / label_cols and row = starts[b] & (2^56 - 1).  Labels: src[label_src](row + history - 1,
  label_cols[k]), rotated per triple by the world->body matrix of the NORMALISED quaternion of that row (x, y, z, w), negated AFTER the rotation when the
  label column carries bit 30.

THE BOUND FOR STANDARDISED VALUES.  The device computes, for a run x_1 .. x_n (fp32, exact in fp64; n <= 256), in fp64 with u = 2^-53 and
gamma_k = k u / (1 - k u), X = max |x_i|:
  1. S^ = the sum: a lane adds its <= 4 elements (<= 3 roundings after the exact 0 + x), six butterfly steps add lanes: every x_i passes <= 9 additions,
     so S^ = sum x_i (1 + t_i), |t_i| <= gamma_9, |S^ - S| <= gamma_9 n X.
  2. m^ = S^ / n (one rounding): |m^ - m| <= gamma_9 X + u (1 + gamma_9) X <= gamma_10 X =: em.
  3. d_i^ = fl(x_i - m^): |d_i^ - d_i| <= em + u (|d_i| + em) <= em + u (2 X + em) =: eta      (|d_i| <= 2 X).
  4. Q^ = the fma chain of d_i^^2 (<= 4 fma per lane, 6 butterfly additions: <= 10 roundings per term): Q^ = sum d_i^^2 (1 + t_i), |t_i| <= gamma_10.
     With d_i^^2 = d_i^2 + 2 d_i h_i + h_i^2, |h_i| <= eta, Cauchy-Schwarz gives |sum 2 d_i h_i| <= 2 eta sqrt(n Q), so with rho = eta sqrt(n / Q):
     |Q^ - Q| / Q <= (1 + gamma_10) (1 + rho)^2 - 1 =: rq.
  5. var^ = Q^ / (n - 1) and sd^ = sqrt(var^), each allowed one ulp (2 u): |sqrt(1 + a) - 1| <= |a|, so |sd^ - sd| / sd <= (1 + rq) (1 + 2 u)^2 - 1 =: rs.
  6. z_i^ = d_i^ / sd^ (one ulp allowed): |z_i^ - z_i| <= (eta / sd + |z_i| rs) / (1 - rs) + 2 u (|z_i| + that) =: e_i.
  7. one rounding to fp32: not part of e_i -- the checker takes it as the OUTWARD rounding of the interval's ends, fl32_down(z - e), fl32_up(z + e): round
     to nearest is monotonic, so a z^ inside [z - e, z + e] rounds inside that.  (bf16: the bf16 roundings of those two fp32 ends, again monotonic.)
  So e_i is about 16 u |z_i| plus eta / sd ~ 12 u X / sd, far below the 2^-24 |z_i| of the fp32 rounding: the second term matters only where X / sd is very large (an offset
  of 1e6 under noise of 0.1: 1.3e-8, a fifth of an fp32 ulp of z ~ 1).  rs >= 1/4 (X / sd beyond ~1e14) is refused: the bound says nothing there.
  The reference itself is computed in numpy's longdouble where that is the 64-bit-mantissa x87 format (its own error is then 2^-11 of the above and e_i is
  enlarged by 2^-10); where longdouble is fp64 the reference's error has the same form as the device's and e_i is doubled.
  Exact cases, bound 0 and compared BIT FOR BIT (the sign of the zero counts): a constant run -- k c is exact in fp64 for k <= 256 and a 24-bit c, so
  m^ = c, every d_i^ = +0, sd^ = 0, 0 / 0 = NaN -> +0.0f, also for a negated run; a run with a NaN inside -- every z is NaN -> +0.0f.
  The sign "applied after the statistics" cannot be seen beyond that zero: round to nearest is symmetric, every intermediate of -x is the exact negative
  of x's, so -standardise(x) == standardise(-x) except that the NaN -> +0 replacement would then come out as -0.  The constant negated run shows it.

THE BOUND FOR ROTATED LABELS.  y_i = fl32(fl64(R_i0 v_0 + R_i1 v_1 + R_i2 v_2)), R from the quaternion q / |q| in fp64:
  |q|^: four products and three additions (gamma_4 relative on a sum of squares), one sqrt: <= 4 u relative after the root (halved, plus the root's ulp).
  Every normalised component carries <= 4 u + 2 u (division) = 6 u.  An off-diagonal entry 2 (a b -+ c d): each product (1 + 6u)^2 (1 + u), the sum one
  more rounding: |dR| <= gamma_15 * 2 (|a b| + |c d|) <= gamma_15 (a^2 + b^2 + c^2 + d^2) = gamma_15.  A diagonal entry 1 - 2 (b^2 + c^2): <= 2 gamma_15 inside,
  one rounding of the result (|R| <= 1): <= 2 gamma_15 + u.  So |dR_ij| <= 32 u for every entry: the PROPAGATED ERROR OF THE NORMALISED QUATERNION is
  32 u sum_j |v_j|.  The dot product, fused or not, adds c u sum_j |R_ij v_j| with c = 3.  e_i = 32 u sum_j |v_j| + 3 u sum_j |R_ij v_j| (enlarged for the
  reference's own error as above); the half fp32 ulp of the result is again the outward rounding of the ends.  The sign (after the rotation) is exact.
  Rotated labels are all compared under the bound, never bit for bit: an all-zero triple gives bound 0 and a zero whose sign depends on the order of the
  three products' sum (and on fusing), which nothing specifies; the interval [0, 0] takes either zero.
"""
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np
import torch

SIGN_FLAG = 1 << 30
ELEMENT_SHIFT = 56
ROW_MASK = (1 << ELEMENT_SHIFT) - 1
U = 2.0 ** -53
LD_WIDE = np.finfo(np.longdouble).eps < 2.0 ** -60
REF_SLACK = (1.0 + 2.0 ** -10) if LD_WIDE else 2.0
SENTINEL_F32 = 0x7FC0BEEF          # a quiet NaN with a payload no kernel produces: "not written" is told from "a NaN was written"
SENTINEL_BF16 = 0x7FC5


def gamma(k):
    return k * U / (1.0 - k * U)


@dataclass
class WindowTables:
    """The tables and scalars of one mshgnn_window_desc, on the host."""
    runs: List[List[List[int]]]            # [K][n_runs][5]
    rows: List[List[int]]                  # [n_rows][2]
    type_nodes: List[int]
    pitch: List[int]                       # row pitch (elements) of every type's output
    history: int
    normalize: int = 0
    label_cols: List[List[int]] = field(default_factory=list)      # [K][n_label]
    label_src: int = 0
    label_rotate: int = 0
    quat_src: int = -1
    sign_flags: int = 0

    @property
    def K(self):
        k = (self.sign_flags >> 8) & 0xff
        return k if k > 1 else 1

    @property
    def n_runs(self):
        return len(self.runs[0])

    @property
    def n_label(self):
        return len(self.label_cols[0]) if self.label_cols else 0

    @property
    def type_width(self):
        w = [1] * len(self.type_nodes)
        for r in self.runs[0]:
            w[r[0]] = max(w[r[0]], r[2] + r[4])
        return w


@dataclass
class Expected:
    x: List[np.ndarray]                    # per type fp64 [B][n_t][pitch] (NaN: a NaN is expected there)
    covered: List[np.ndarray]              # bool: some run writes the element
    pad_zero: List[np.ndarray]             # bool: a pad column inside a row's last 16-byte chunk (the chunk kernel writes +0 there)
    bound: List[np.ndarray]                # fp64 >= 0; 0: bit for bit
    run: List[np.ndarray]                  # int: the run an element belongs to (-1: none)
    y: Optional[np.ndarray] = None         # [B][n_label] fp64
    y_bound: Optional[np.ndarray] = None
    quat: Optional[np.ndarray] = None      # [B][4] fp32, copied
    y_rotated: bool = False                # rotated labels: every element under its bound (an all-zero triple gives a zero whose sign is the summation order's)


def split_start(start, K):
    u = int(start) & ((1 << 64) - 1)
    if K <= 1:
        return 0, int(start)
    return min(u >> ELEMENT_SHIFT, K - 1), u & ROW_MASK


def decode(word, signed):
    """(source, column, negated) of a run's word; source None: the constant 1."""
    if word == -1:
        return None, 0, False
    neg = bool(signed and word >= 0 and (word & SIGN_FLAG))
    if neg:
        word &= ~SIGN_FLAG
    return word >> 8, word & 0xff, neg


def f32(a):
    """The host series as the store uploads them: rounded to fp32 first."""
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32))


# ---- the arithmetic of one standardised run ------------------------------------------------------------------------------------------------------
def standardise_exact(x):
    """(z fp64, bound fp64) of one run x (fp32 values, already negated where the run is): the reference in the widest float there is."""
    n = x.size
    if np.isnan(x).any():
        return np.zeros(n), np.zeros(n)
    if np.isinf(x).any():
        raise ValueError("infinities in a standardised series are not covered (see tests/test_windows_exact_gpu.py)")
    xl = x.astype(np.longdouble)
    m = xl.sum() / n
    d = xl - m
    Q = (d * d).sum()
    if float(x.max()) == float(x.min()):
        return np.zeros(n), np.zeros(n)                  # 0 / 0 = NaN -> +0, exact (see above)
    sd = np.sqrt(Q / (n - 1))
    z = (d / sd).astype(np.float64)
    X = float(np.abs(x).max())
    sdf, Qf = float(sd), float(Q)
    em = gamma(10) * X
    eta = em + U * (2.0 * X + em)
    rho = eta * np.sqrt(n / Qf)
    rq = (1.0 + gamma(10)) * (1.0 + rho) ** 2 - 1.0
    rs = (1.0 + rq) * (1.0 + 2.0 * U) ** 2 - 1.0
    if not rs < 0.25:
        raise ValueError(f"max |x| / sd = {X / sdf:.3g}: the derived bound says nothing for this run; use other data")
    e = (eta / sdf + np.abs(z) * rs) / (1.0 - rs)
    e = e + 2.0 * U * (np.abs(z) + e)
    return z, e * REF_SLACK


LANE_OF = np.arange(256) % 128 // 2          # element k sits in lane (k % 128) / 2, slot 2 (k / 128) + (k & 1)
SLOT_OF = 2 * (np.arange(256) // 128) + (np.arange(256) & 1)


def _wave_sum(v):
    for m in (32, 16, 8, 4, 2, 1):
        v = v + v[np.arange(64) ^ m]
    return v[0]


def standardise_kernel(x, ddof=1, mean_fp32=False, constant_nan=False):
    """run_stats / standardise_one of mshgnn_device.hpp in fp64, in the kernel's order, then ONE rounding to fp32.  The keyword arguments are the
    mutations of tests/test_window_reference.py."""
    n = x.size
    xd = x.astype(np.float64)
    part = np.zeros(64)
    for q in range(4):
        sel = SLOT_OF[:n] == q
        part[LANE_OF[:n][sel]] += xd[sel]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        mean = _wave_sum(part) / n
        if mean_fp32:
            acc = np.float32(0)
            for v in x:
                acc = np.float32(acc + v)
            mean = float(np.float32(acc / np.float32(n)))
        qs = np.zeros(64)
        for q in range(4):
            sel = SLOT_OF[:n] == q
            d = xd[sel] - mean
            qs[LANE_OF[:n][sel]] += d * d            # (the device fuses this multiply-add: one rounding fewer, inside the bound either way)
        sd = np.sqrt(_wave_sum(qs) / (n - ddof))
        z = (xd - mean) / sd
    if not constant_nan:
        z = np.where(np.isnan(z), 0.0, z)
    with np.errstate(over="ignore"):
        return z.astype(np.float32)


# ---- the rotation ----------------------------------------------------------------------------------------------------------------------------
def quat_matrix(q, dtype=np.longdouble, normalise=True):
    x, y, z, w = (np.asarray(q, dtype=dtype) / (np.sqrt((np.asarray(q, dtype=dtype) ** 2).sum()) if normalise else dtype(1)))
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], dtype=dtype)


# ---- the walk over the tables ------------------------------------------------------------------------------------------------------------------
MUTATIONS = ("start+1", "drop-last", "swap-runs", "feature-late", "neighbour-column", "sign-after-stats", "sign-dropped-in-chunk", "ddof0", "mean-fp32",
             "constant-nan", "ones-standardised", "label-first-row", "R-transposed", "quat-not-normalised", "label-negated-before-rotation",
             "element-not-clamped", "pad-outside-last-chunk", "uncovered-overwritten")


def _walk(tab: WindowTables, series: Sequence[np.ndarray], starts, chunk: int, exact: bool, mut: Optional[str]):
    """Both the reference (exact=True, mut None) and the emulation of the kernels (exact=False: fp64 in the kernels' order, one rounding to fp32, with one
    mutation `mut` or none).  chunk: 0 = the run-by-run kernel, else the elements of a 16-byte chunk of the chunk kernel (4 fp32, 8 bf16)."""
    K, B = tab.K, len(starts)
    signed = bool(tab.sign_flags & 1) or K > 1
    nt = len(tab.type_nodes)
    shape = [(B, tab.type_nodes[t], tab.pitch[t]) for t in range(nt)]
    x = [np.zeros(s) for s in shape]
    covered = [np.zeros(s, dtype=bool) for s in shape]
    pad = [np.zeros(s, dtype=bool) for s in shape]
    bound = [np.zeros(s) for s in shape]
    runid = [np.full(s, -1, dtype=np.int64) for s in shape]
    for b, sw in enumerate(starts):
        el, row = split_start(sw, K)
        if mut == "element-not-clamped" and K > 1 and ((int(sw) & ((1 << 64) - 1)) >> ELEMENT_SHIFT) >= K:
            el = 0
        if mut == "start+1":
            row += 1
        runs = [list(r) for r in tab.runs[el]]
        if mut == "swap-runs":      # the first two sourced runs of different words in one row trade sources
            for r0, r1 in tab.rows:
                cand = [r for r in range(r0, r1) if runs[r][3] != -1]
                pair = next(((a, c) for a in cand for c in cand if a < c and runs[a][3] != runs[c][3]), None)
                if pair:
                    runs[pair[0]][3], runs[pair[1]][3] = runs[pair[1]][3], runs[pair[0]][3]
                    break
        for ri, (r0, r1) in enumerate(tab.rows):
            for r in range(r0, r1):
                t, node, f0, word, ln = runs[r]
                s, c, neg = decode(word, signed)
                if mut == "feature-late" and r == r0:
                    f0 += 1
                if s is None:
                    v = np.ones(ln, dtype=np.float32)
                    if mut == "ones-standardised" and tab.normalize:
                        v = np.zeros(ln, dtype=np.float32)
                    e = np.zeros(ln)
                    vals = v.astype(np.float64)
                else:
                    if mut == "neighbour-column" and r == r0:
                        c = c + 1 if c + 1 < series[s].shape[1] else c - 1
                    v = series[s][row:row + ln, c]
                    if v.size < ln and mut == "start+1":      # (the mutant reads past the series' end: whatever lies there)
                        v = np.concatenate([v, np.full(ln - v.size, np.nan, dtype=np.float32)])
                    assert v.size == ln, "window past the end of the series"
                    late_sign = neg and mut == "sign-after-stats"
                    if neg and not late_sign:
                        v = -v
                    if mut == "sign-dropped-in-chunk" and chunk and r > r0:
                        # a chunk that starts in the run before: this run's elements inside it get THAT run's sign
                        k_first = (r - r0) * ln
                        head = (-k_first) % chunk
                        if head:
                            _, _, neg_prev = decode(runs[r - 1][3], signed)
                            if neg_prev != neg:
                                v = v.copy(); v[:head] = -v[:head]
                    if tab.normalize:
                        if exact:
                            vals, e = standardise_exact(v)
                        else:
                            vals = standardise_kernel(v, ddof=0 if mut == "ddof0" else 1, mean_fp32=mut == "mean-fp32", constant_nan=mut == "constant-nan").astype(np.float64)
                            e = np.zeros(ln)
                        if late_sign:
                            vals = -vals
                    else:
                        vals, e = v.astype(np.float64), np.zeros(ln)
                        if late_sign:
                            vals = -vals
                n_out = ln - 1 if (mut == "drop-last" and r == r1 - 1) else ln
                if mut == "feature-late":
                    n_out = min(n_out, tab.pitch[t] - f0)      # (the emulation stays inside its row)
                x[t][b, node, f0:f0 + n_out] = vals[:n_out]
                covered[t][b, node, f0:f0 + n_out] = True
                bound[t][b, node, f0:f0 + n_out] = e[:n_out]
                runid[t][b, node, f0:f0 + n_out] = r
            if chunk:      # the chunk kernel: zeros up to the end of the row's last chunk
                t, node, f0 = runs[r0][0], runs[r0][1], runs[r0][2]
                width = (r1 - r0) * runs[r0][4]
                end = (width + chunk - 1) // chunk * chunk
                if mut == "pad-outside-last-chunk":
                    end += chunk      # (clipped at the row's pitch by the slice below: a row narrower than its type's pitch shows it)
                pad[t][b, node, f0 + width:f0 + end] = True
        if mut == "uncovered-overwritten":
            for t in range(nt):
                free = np.argwhere(~covered[t][b] & ~pad[t][b])
                if len(free):
                    covered[t][b, free[0][0], free[0][1]] = True      # (value 0)
                    break
    out = Expected(x, covered, pad, bound, runid)
    # labels and quaternions
    qsrc = series[tab.quat_src] if tab.quat_src >= 0 else None
    nl = tab.n_label
    if nl or qsrc is not None:
        y, yb = np.zeros((B, nl)), np.zeros((B, nl))
        quat = np.zeros((B, 4), dtype=np.float32)
        wide = np.longdouble if exact else np.float64
        for b, sw in enumerate(starts):
            el, row = split_start(sw, K)
            if mut == "element-not-clamped" and K > 1 and ((int(sw) & ((1 << 64) - 1)) >> ELEMENT_SHIFT) >= K:
                el = 0
            if mut == "start+1":
                row = (row + 1) % (series[tab.label_src].shape[0] - tab.history + 1)
            row += tab.history - 1
            lrow = row - (tab.history - 1) if mut == "label-first-row" else row
            R = None
            if qsrc is not None:
                quat[b] = qsrc[row, :4]
                if tab.label_rotate:
                    R = quat_matrix(qsrc[lrow, :4], wide, normalise=mut != "quat-not-normalised")
                    if mut == "R-transposed":
                        R = R.T
            if nl:
                cols = [c & ~SIGN_FLAG if signed else c for c in tab.label_cols[el]]
                negs = np.array([bool(signed and (c & SIGN_FLAG)) for c in tab.label_cols[el]])
                v = series[tab.label_src][lrow, cols].astype(wide)
                if R is not None:
                    if mut == "label-negated-before-rotation":
                        v = np.where(negs, -v, v)
                    v3 = v.reshape(-1, 3)
                    yy = (v3 @ R.T).reshape(-1)
                    e = (32 * U * np.abs(v3).sum(axis=1, keepdims=True) + 3 * U * (np.abs(v3) @ np.abs(R).T)).astype(np.float64).reshape(-1) * REF_SLACK
                    if mut == "label-negated-before-rotation":
                        negs = np.zeros_like(negs)
                else:
                    yy, e = v, np.zeros(nl)
                yy = np.where(negs, -yy, yy).astype(np.float64)
                if exact:
                    y[b], yb[b] = yy, e
                else:
                    with np.errstate(over="ignore"):
                        y[b] = yy.astype(np.float32)
        out.y_rotated = bool(tab.label_rotate and nl)
        out.y, out.y_bound, out.quat = (y if nl else None), (yb if nl else None), (quat if qsrc is not None else None)
    return out


def reference(tab, series, starts, chunk=0) -> Expected:
    """The expected result of mshgnn_assemble_windows for these tables, series ([rows][columns] fp32 per source) and starts (packed when K > 1)."""
    return _walk(tab, series, starts, chunk, True, None)


def emulate(tab, series, starts, dtype, chunk=0, mut=None, batch_rows=None):
    """What the kernels write, emulated on the host in fp64 + one rounding (optionally with one mutation): (xs, y, quat) as torch CPU tensors in the
    harness' layout -- xs[t] [batch_rows][n_t][pitch] at `dtype` over the sentinel fill, y / quat with 64 sentinel elements behind."""
    k = _walk(tab, series, starts, chunk, False, mut)
    B = len(starts)
    xs = []
    for t in range(len(tab.type_nodes)):
        buf = sentinel_tensor((batch_rows or B + 2, tab.type_nodes[t], tab.pitch[t]), dtype)
        with np.errstate(over="ignore", invalid="ignore"):
            v = torch.from_numpy(np.where(k.pad_zero[t], 0.0, k.x[t]).astype(np.float32)).to(buf.dtype)
        m = torch.from_numpy(k.covered[t] | k.pad_zero[t])
        buf[:B][m] = v[m]
        xs.append(buf)
    y = q = None
    if k.y is not None:
        y = sentinel_tensor((B * tab.n_label + 64,), "f32")
        y[:B * tab.n_label] = torch.from_numpy(k.y.astype(np.float32)).reshape(-1)
    if k.quat is not None:
        q = sentinel_tensor((B * 4 + 64,), "f32")
        q[:B * 4] = torch.from_numpy(k.quat).reshape(-1)
    return xs, y, q


# ---- checkers ------------------------------------------------------------------------------------------------------------------------------------
def sentinel_tensor(shape, dtype, device="cpu"):
    if dtype == "bf16":
        return torch.full(shape, SENTINEL_BF16, dtype=torch.int16, device=device).view(torch.bfloat16)
    return torch.full(shape, SENTINEL_F32, dtype=torch.int32, device=device).view(torch.float32)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _f32_of(want64):
    with np.errstate(over="ignore", invalid="ignore"):
        return torch.from_numpy(np.asarray(want64, dtype=np.float64).astype(np.float32))


def first_mismatch(got: torch.Tensor, want64, mask=None):
    """Index (tuple) of the first element of `got` (fp32 or bf16, CPU) whose BITS are not those of the fp32 value `want64` cast by torch to got's dtype
    (fp32 -> bf16: torch's own cast), or None.  Any NaN matches any NaN; the sign of a zero counts.  mask: only where True."""
    want = _f32_of(want64).to(got.dtype)
    bad = (_bits(got) != _bits(want)) & ~(torch.isnan(got) & torch.isnan(want))
    if mask is not None:
        bad &= torch.as_tensor(mask)
    idx = torch.nonzero(bad)
    return tuple(int(i) for i in idx[0]) if len(idx) else None


def fl32_down(v):
    with np.errstate(over="ignore", invalid="ignore"):
        f = np.asarray(v, dtype=np.float64).astype(np.float32)
        return np.where(f.astype(np.float64) > v, np.nextafter(f, np.float32(-np.inf)), f).astype(np.float32)


def fl32_up(v):
    with np.errstate(over="ignore", invalid="ignore"):
        f = np.asarray(v, dtype=np.float64).astype(np.float32)
        return np.where(f.astype(np.float64) < v, np.nextafter(f, np.float32(np.inf)), f).astype(np.float32)


def within_bound(got: torch.Tensor, want64, bound, mask=None):
    """Index of the first element outside its interval, or None.  fp32: [fl32_down(want - e), fl32_up(want + e)]; bf16: between torch's bf16 roundings of
    those two fp32 ends (rounding is monotonic: exactly the results some fp32 value inside the bound could give).  NaN is outside every interval."""
    want64, bound = np.asarray(want64, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    lo, hi = torch.from_numpy(fl32_down(want64 - bound)), torch.from_numpy(fl32_up(want64 + bound))
    if got.dtype == torch.bfloat16:
        lo, hi = lo.to(torch.bfloat16), hi.to(torch.bfloat16)
    g = got.double()
    bad = ~((g >= lo.double()) & (g <= hi.double()))
    if mask is not None:
        bad &= torch.as_tensor(mask)
    idx = torch.nonzero(bad)
    return tuple(int(i) for i in idx[0]) if len(idx) else None


def _sentinel_broken(got, mask):
    sent = SENTINEL_BF16 if got.dtype == torch.bfloat16 else SENTINEL_F32
    idx = torch.nonzero((_bits(got) != sent) & torch.as_tensor(mask))
    return tuple(int(i) for i in idx[0]) if len(idx) else None


def check(tab: WindowTables, exp: Expected, xs, y=None, quat=None, starts=None, sentinels=True):
    """None, or the description of the first wrong element of what a gather wrote: xs[t] [>= B][n_t][pitch] over the sentinel fill (rows behind the batch,
    uncovered features and pad columns outside a last chunk must still hold it), y / quat flat with sentinel elements behind."""
    for t, got in enumerate(xs):
        got = got.cpu()
        B = exp.x[t].shape[0]
        head, tail = got[:B], got[B:]
        def where(i, what, want=None):
            b, n, f = i
            r = int(exp.run[t][b, n, f])
            at = ""
            if r >= 0:
                el, row = split_start(starts[b], tab.K) if starts is not None else (0, -1)
                run = tab.runs[el][r]
                at = f"; run {r} {run} (element block {el}), position {f - run[2]} of {run[4]}, window row {row}"
            return (f"{what}: window {i[0]}, type {t}, node {n}, feature {f}: got {float(head[i]):.9g} (bits {int(_bits(head)[i]) & (0xffff if head.dtype == torch.bfloat16 else 0xffffffff):#x})"
                    + (f", want {want:.17g} +- {float(exp.bound[t][i]):.3g}" if want is not None else "") + at)
        i = _sentinel_broken(tail, np.ones(tuple(tail.shape), dtype=bool)) if tail.numel() and sentinels else None
        if i is not None:
            return f"type {t}: row {B + i[0]} behind the batch of {B} was written (node {i[1]}, feature {i[2]})"
        free = ~exp.covered[t] & ~exp.pad_zero[t]
        i = _sentinel_broken(head, free) if sentinels else None      # (sentinels=False: buffers of a SequenceStore, whose pad columns are zeroed once)
        if i is not None:
            return where(i, "an element no run covers was written")
        i = first_mismatch(head, np.zeros(exp.x[t].shape), exp.pad_zero[t])
        if i is not None:
            return where(i, "a pad column inside the row's last chunk is not +0")
        exact = exp.covered[t] & (exp.bound[t] == 0)
        i = first_mismatch(head, exp.x[t], exact)
        if i is not None:
            return where(i, "not the expected bits", float(exp.x[t][i]))
        i = within_bound(head, exp.x[t], exp.bound[t], exp.covered[t] & ~exact)
        if i is not None:
            return where(i, "outside the derived bound", float(exp.x[t][i]))
    for name, got, want, bnd in (("y", y, exp.y, exp.y_bound), ("quat", quat, exp.quat, None)):
        if want is None:
            if got is not None and _sentinel_broken(got.cpu(), np.ones(tuple(got.shape), dtype=bool)) is not None:
                return f"{name} was written although the descriptor asks for none"
            continue
        if got is None:
            continue
        got = got.cpu()
        n = want.size
        i = _sentinel_broken(got[n:], np.ones(got.numel() - n, dtype=bool))
        if i is not None:
            return f"{name}: element {n + i[0]} behind the result was written"
        g = got[:n].reshape(want.shape)
        b0 = np.zeros(want.shape) if bnd is None else bnd
        exact = np.zeros(want.shape, dtype=bool) if (name == "y" and exp.y_rotated) else b0 == 0
        i = first_mismatch(g, want, exact) or within_bound(g, want, b0, ~exact)
        if i is not None:
            return f"{name}[window {i[0]}][{i[1]}]: got {float(g[i]):.9g}, want {float(want[i]):.17g} +- {float(b0[i]):.3g} (window row {split_start(starts[i[0]], tab.K)[1] if starts is not None else '?'})"
    return None


# ---- case builders: the descriptors of tests/test_windows_exact_gpu.py, shared with the host controls ------------------------------------------------
SPECIALS = np.array([0.0, -0.0, 1e-45, -1e-45, 1.1754942e-38, 3.4028235e38, -3.4028235e38, np.inf, -np.inf, np.nan, 3.3895314e38], dtype=np.float32)
N_ROWS_SERIES = 300
CSTRIDE_EXTRA = (0, 8, 13)


def make_series(n_src, seed, n_rows=N_ROWS_SERIES, specials=False, wide_first=True):
    """n_src fp32 series [n_rows][columns]: source 0 has 256 columns (column 255 exists), the others 1 .. 9.  specials: +-0, subnormals, the largest
    finite value (infinity on bf16), +-inf and a NaN are sprinkled in, several per window of any length >= 2."""
    rng = np.random.default_rng(seed)
    out = []
    for s in range(n_src):
        ncol = 256 if (s == 0 and wide_first) else 1 + (3 * s + 2) % 9
        a = rng.standard_normal((n_rows, ncol)).astype(np.float32)
        if specials:
            at = rng.random((n_rows, ncol)) < 0.3
            a[at] = SPECIALS[rng.integers(0, len(SPECIALS), int(at.sum()))]
        out.append(a)
    return out


def general_case(counts, seed, *, lengths=(1, 2, 3, 5, 4, 7, 2, 6), n_types=4, n_src=12, normalize=0, signed=False, K=1, history=None, pitch_extra=(1, 0, 8, 5),
                 gaps=True, ones_every=5, fast_layout=False, chunk=0, series_rows=N_ROWS_SERIES, specials=True, series=None, const_rows=0, row_lengths=None):
    """Tables for the run-by-run kernel: row i has counts[i] runs (lengths cycle through `lengths`; fast_layout: all `history` long from feature 0), rows
    are dealt to n_types types in contiguous blocks, gaps of 0..2 uncovered features in front of / between runs, every `ones_every`-th run the constant
    1, sources and columns random (column 255 included), signs in the pattern + + - - (every arrangement of two neighbours).  K > 1: block e takes
    other columns and flips other signs.  Returns (tables, series)."""
    rng = np.random.default_rng(seed)
    series = series if series is not None else make_series(n_src, seed + 1, series_rows, specials and not normalize)
    n_src = len(series)
    n_rows = len(counts)
    n_types = min(n_types, n_rows)
    per = [(n_rows + n_types - 1 - t) // n_types for t in range(n_types)]
    runs = [[] for _ in range(K)]
    rows = []
    i = j = 0
    for t in range(n_types):
        for node in range(per[t]):
            f = 0
            r0 = len(runs[0])
            for _ in range(counts[i]):
                ln = row_lengths[i] if row_lengths else (history if fast_layout else lengths[j % len(lengths)])
                if gaps and not fast_layout:
                    f += int(rng.integers(0, 3))
                s = int(rng.integers(0, n_src)) if j % 14 else 0      # (every 14th run: source 0, whose last column is 255)
                c = int(rng.integers(0, series[s].shape[1])) if j % 7 else series[s].shape[1] - 1
                ones = bool(ones_every) and j % ones_every == ones_every - 1 and not fast_layout
                for e in range(K):
                    ce = (c + e) % series[s].shape[1]
                    neg = signed and (((j % 4) >= 2) != bool(e & 1 and j % 3 == 0))
                    runs[e].append([t, node, f, -1 if ones else ((s << 8) | ce | (SIGN_FLAG if neg else 0)), ln])
                f += ln
                j += 1
            rows.append([r0, len(runs[0])])
            i += 1
    if const_rows:      # a last type of width-1 constant rows (what a recipe gives a type without variables)
        for node in range(const_rows):
            rows.append([len(runs[0]), len(runs[0]) + 1])
            for e in range(K):
                runs[e].append([n_types, node, 0, -1, 1])
        per.append(const_rows); n_types += 1
    widths = [1] * n_types
    for r in runs[0]:
        widths[r[0]] = max(widths[r[0]], r[2] + r[4])
    if chunk:
        pitch = [(w + chunk - 1) // chunk * chunk + chunk * (t % 2) for t, w in enumerate(widths)]
    else:
        pitch = [w + pitch_extra[t % len(pitch_extra)] for t, w in enumerate(widths)]
    hist = history or max(r[4] for r in runs[0])
    tab = WindowTables(runs, rows, per, pitch, hist, normalize=normalize, sign_flags=((1 if signed or K > 1 else 0) | ((K << 8) if K > 1 else 0)))
    return tab, series


def starts_for(tab, series, B, seed=0, elements=None):
    """B starts: 0, the last valid row, repeats and random ones; elements (K > 1): one per window, packed into bits 56..63 (values >= K are kept: the
    kernels clamp them)."""
    need = max(tab.history, max(r[4] for r in tab.runs[0]))
    last = min(s.shape[0] for s in series) - need
    rng = np.random.default_rng(seed)
    st = [0, last, last // 2, last // 2, 0][:B] + [int(v) for v in rng.integers(0, last + 1, max(0, B - 5))]
    if tab.K > 1:
        el = list(elements) if elements is not None else [b % tab.K for b in range(B)]
        st = [(int(e) << ELEMENT_SHIFT) | s for s, e in zip(st, (el * B)[:B])]
        st = [s - (1 << 64) if s >= (1 << 63) else s for s in st]      # as int64
    return st


def lengths_case(normalize=0, signed=False):
    """Every run length of the matrix at an even and an odd first feature: 24 node rows of one run each."""
    L = (1, 2, 3, 63, 64, 65, 127, 128, 129, 130, 255, 256)
    series = make_series(3, 11, specials=not normalize)
    runs, rows = [], []
    rng = np.random.default_rng(12)
    for i, ln in enumerate(L):
        for par in (0, 1):
            s = int(rng.integers(0, 3))
            c = int(rng.integers(0, series[s].shape[1]))
            rows.append([len(runs), len(runs) + 1])
            runs.append([0, 2 * i + par, 2 + par, (s << 8) | c | (SIGN_FLAG if signed and (i + par) % 2 else 0), ln])
    return WindowTables([runs], rows, [24], [261], 256, normalize=normalize, sign_flags=int(signed)), series


STD_LENGTHS = (2, 3, 64, 129, 256)


def standardise_case(words=None):
    """One node row per length in STD_LENGTHS, every row: random, constant, negated constant, offset 1e6 under noise of a few fp32 spacings, two-valued,
    magnitude 1e30, magnitude 1e-30, a NaN inside, a negated random run beside a plain one of the same column, the constant 1, a negated offset run."""
    rng = np.random.default_rng(21)
    n = N_ROWS_SERIES
    a = np.zeros((n, 8), dtype=np.float32)
    a[:, 0] = rng.standard_normal(n)
    a[:, 1] = 0.7321
    # (two values / an offset under noise: both alternate with the row's parity, so no window of length >= 2 is constant)
    a[::2, 2] = np.float32(1e6) + np.float32(0.0625) * rng.integers(1, 4, (n + 1) // 2).astype(np.float32)
    a[1::2, 2] = np.float32(1e6) - np.float32(0.0625) * rng.integers(0, 4, n // 2).astype(np.float32)
    a[::2, 3] = -2.5; a[1::2, 3] = 1.25
    a[:, 4] = rng.standard_normal(n) * 1e30
    a[:, 5] = rng.standard_normal(n) * 1e-30
    a[:, 6] = rng.standard_normal(n); a[::2, 6] = np.nan     # (a NaN inside every window of length >= 2)
    a[:, 7] = rng.standard_normal(n) * 3 + 5
    series = [a, rng.standard_normal((n, 2)).astype(np.float32)]
    runs, rows = [], []
    words = words or [0, 1, SIGN_FLAG | 1, 2, 3, 4, 5, 6, 7, SIGN_FLAG | 7, -1, SIGN_FLAG | 2, (1 << 8) | 1]
    for node, ln in enumerate(STD_LENGTHS):
        f = node % 2      # odd and even first features
        r0 = len(runs)
        for w in words:
            runs.append([0, node, f, w, 1 if w == -1 else ln])
            f += 1 if w == -1 else ln
        rows.append([r0, len(runs)])
    width = max(r[2] + r[4] for r in runs)
    return WindowTables([runs], rows, [len(STD_LENGTHS)], [width + 3], 256, normalize=1, sign_flags=1), series


QUAT_KINDS = 6


def label_series(n_label_cols=256, seed=31, n_rows=N_ROWS_SERIES):
    """(labels [n_rows][256], quaternions [n_rows][4]): row r's quaternion is, by r % 6: unit, norm 0.5, norm 3, negative w, near identity, near a half turn."""
    rng = np.random.default_rng(seed)
    lab = (rng.standard_normal((n_rows, n_label_cols)) * 40).astype(np.float32)
    lab[rng.random(lab.shape) < 0.1] = 0.0
    q = rng.standard_normal((n_rows, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    k = np.arange(n_rows) % QUAT_KINDS
    q[k == 1] *= 0.5
    q[k == 2] *= 3.0
    q[k == 3, 3] = -np.abs(q[k == 3, 3]) - 0.1
    small = rng.standard_normal((n_rows, 3)) * 1e-4
    q[k == 4, :3] = small[k == 4]; q[k == 4, 3] = 1.0
    q[k == 5, :3] /= np.linalg.norm(q[k == 5, :3], axis=1, keepdims=True); q[k == 5, 3] = 1e-4 * rng.standard_normal(int((k == 5).sum()))
    return lab, q.astype(np.float32)


def label_case(n_label, rotate, signed=False, K=1, history=5, quat=True, seed=0):
    """A one-node, width-1 constant window (the gather kernels still run) with n_label labels from random columns of a 256-column series (column 255
    included), optionally rotated by the quaternion series, signed (mixed signs inside every triple), K label blocks."""
    rng = np.random.default_rng(100 + n_label + seed)
    lab, q = label_series()
    cols = []
    for e in range(K):
        c = [int(v) for v in rng.integers(0, 256, n_label)]
        if n_label:
            c[-1] = 255
        if signed or K > 1:
            c = [v | (SIGN_FLAG if (i + e) % 3 != 1 else 0) for i, v in enumerate(c)]
        cols.append(c)
    runs = [[[0, 0, 0, -1, 1]] for _ in range(K)]
    tab = WindowTables(runs, [[0, 1]], [1], [3], history, label_cols=cols if n_label else [], label_src=0, label_rotate=int(rotate), quat_src=1 if quat else -1,
                       sign_flags=((1 if signed or K > 1 else 0) | ((K << 8) if K > 1 else 0)))
    return tab, [lab, q]


def recipe_tables(recipe, names, dtype, padded_width, tables=None):
    """WindowTables of a `WindowRecipe` (or of an orbit's stacked recipes) as a SequenceStore describes it: the tie to the recipes' own evaluators."""
    if tables is None:
        runs, rows, lab, signed = recipe.tables(names)
        runs_k, lab_k, K = [runs], [lab], 1
    else:
        runs_k, rows, lab_k = tables
        K, signed = len(runs_k), True
    sidx = {s: i for i, s in enumerate(names)}
    return WindowTables([[list(r) for r in blk] for blk in runs_k], [list(r) for r in rows], [recipe.num_nodes[t] for t in recipe.node_types],
                        [padded_width(t) for t in recipe.node_types], recipe.history, normalize=int(recipe.normalize),
                        label_cols=[list(c) for c in lab_k] if recipe.label_cols else [], label_src=sidx[recipe.label_series] if recipe.label_series else 0,
                        label_rotate=int(recipe.label_rotate), quat_src=sidx[recipe.quat_series] if recipe.quat_series else -1,
                        sign_flags=((1 if signed else 0) | ((K << 8) if K > 1 else 0)))
