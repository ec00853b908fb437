"""Host references (numpy fp64, no GPU) for the kernels that publish a run's numbers (csrc/mshgnn_train_ops.hip: k_metrics_reg, k_metrics_cls, k_metrics_com,
k_grf_to_world and the one-workgroup forms of the first two), the data the GPU tests feed them, the checkers those tests apply, and `damaged`: wrong results of
the kinds such kernels produce, which tests/test_metrics_reference.py shows every checker to reject for every case tests/test_metrics_exact_gpu.py runs.

ORDER MIRROR (`order_sum`).  The regression sums, the squared-error sums of the COM step and (on exact data) its cosine sums are reproduced rounding by
rounding: a thread adds the terms of its grid-stride items in index order (thread g of nt * blocks takes items g, g + nt * blocks, ...), a wave adds its 64
lanes in the xor butterfly of strides 32 .. 1 (every lane ends with the same bits: fp64 addition commutes), thread 0 adds the workgroup's waves in order from
0.0, the last workgroup adds the workgroups' partials in index order from 0.0, and the epoch state has the total added.  The launch geometry is a parameter,
restated here from the entry points' text (not imported): the step calls run 256 threads on clamp(ceil(items / (per_thread * 256)), 1, 64) workgroups with
per_thread = 16 elements for the regression and 1 window for the classification / COM step; the accumulating entry points run one workgroup of 1024.
`s += d * d` may be compiled to a fused multiply-add: the makers below only produce residuals whose square is exact in fp64, so both forms give the same bits.

BOUNDS.  u = 2^-53.  gamma_k = k u / (1 - k u) (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2).
  * cross-entropy sum of m per-foot terms: gamma_(m + 4) * sum |terms| against math.fsum of the fp64 terms (the bound tests/test_segmented_metrics_gpu.py
    uses), plus K u |term| per term for the device's exp / log, K measured on the device (tests/test_metrics_exact_gpu.py states the figures).
  * one window's cosine (`com_window_bound`): v = x * std + mean carries at most u (|x std| + |v|) whether it is fused or not; a vector off by dv moves its
    unit vector by less than 2 |dv| / |v|, so the cosine by 2 (|dp|_1 / |p| + |dy|_1 / |y|); the arithmetic after that -- two three-term sums of squares
    (1.5 u each on the norm), two square roots (u each), six divisions (2 u per product), three products (u) and the three-term sum (3 u) -- is within
    COS_ROUNDINGS = 12 u of sum_k |p_k y_k| / (|p| |y|).  `com_random` refuses data whose bound exceeds 1e-13 in any window, 5e5 times below one fp32 step.
    The values these bounds are applied against are formed in numpy's extended precision, whose own error is 2^-11 of them.
  * the rotation (`grf_bound`): the kernel forms the fp64 value and rounds once to fp32: 0.5 ulp32(want) + 16 u sum_j A_ji |f_j|.  A_ji is the entry R_ji
    with every term of its formula taken in absolute value (1 + 2 (y^2 + z^2), 2 (|x y| + |z w|), ...): the roundings of an entry scale with its terms, not
    with what is left after they cancel; A = |R| where nothing cancels.  Counted: a unit component carries 4 u (four-term sum, root, division), a product of
    two 9 u, the difference / sum one more, the three-term dot product 3 u: 14 u.
"""
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
MET_BLOCKS, MET_THREADS, ACC_THREADS, N_COUNTS = 64, 256, 1024, 18
EPS = 1e-8
COS_ROUNDINGS = 12
COM_WINDOW_LIMIT = 1e-13
EXT = np.longdouble
assert np.finfo(EXT).eps <= 2.0 ** -63, "the extended-precision references need a long double wider than fp64"


def gamma(k):
    return k * U / (1.0 - k * U)


def step_blocks(items, per_thread):
    """Workgroups of a step launch (met_blocks in the library)."""
    return max(1, min(MET_BLOCKS, -(-int(items) // (per_thread * MET_THREADS))))


def geometry(kind, items, entry="step"):
    """(threads per workgroup, workgroups) of the launch for `items` elements (kind "reg") or windows ("cls", "com")."""
    if entry == "acc":
        return ACC_THREADS, 1
    return MET_THREADS, step_blocks(items, 16 if kind == "reg" else 1)


def block_of(items, nt, blocks):
    """The workgroup that takes each item."""
    return (np.arange(items) // nt) % blocks


def order_sum(terms, nt, blocks, dtype=np.float64, skip_block=None, stale=None):
    """The kernels' sum of `terms` [items] or [items][per_item] (module docstring).  skip_block / stale: the damaged sums -- a partial left out, and a further
    partial (the value `stale`, what an earlier and larger call left behind) added after the last one."""
    terms = np.asarray(terms, dtype=dtype)
    terms = terms.reshape(terms.shape[0], -1)
    items, per = terms.shape
    stride = nt * blocks
    sweeps = -(-items // stride)
    pad = np.zeros((sweeps * stride, per), dtype=dtype)          # (x + 0.0 == x bit for bit for every x a sum started at +0.0 can hold)
    pad[:items] = terms
    seq = pad.reshape(sweeps, stride, per).transpose(1, 0, 2).reshape(stride, sweeps * per)
    s = np.zeros(stride, dtype=dtype)
    for j in range(seq.shape[1]):
        s = s + seq[:, j]
    v = s.reshape(blocks, nt // 64, 64)
    lane = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ m]
    part = np.zeros(blocks, dtype=dtype)
    for k in range(nt // 64):
        part = part + v[:, k, 0]
    total = dtype(0.0)
    for b in range(blocks):
        if b != skip_block:
            total = total + part[b]
    if stale is not None:
        total = total + dtype(stale)
    return np.float64(total)


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


def first_bit_mismatch(got, want, what):
    got, want = np.asarray(got, dtype=np.float64).ravel(), np.asarray(want, dtype=np.float64).ravel()
    if got.shape != want.shape:
        return f"{what}: {got.shape} values, {want.shape} expected"
    bad = np.nonzero(_bits(got) != _bits(want))[0]
    if bad.size:
        i = int(bad[0])
        return f"{what}[{i}] = {got[i]!r} ({got[i].hex() if np.isfinite(got[i]) else got[i]}), the reference has {want[i]!r} ({bad.size} of {got.size} differ)"
    return None


# ---------------------------------------------------------------------------------------------------
# regression
# ---------------------------------------------------------------------------------------------------
REG_N = [1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8193, 262143, 262144, 262145, 266245]
REG_ACC_N = [1, 1023, 1024, 1025, 5000]
BATCH_FILL = 7.5                                   # what the batch state holds before a call: it must be overwritten
REG_EPOCH0 = np.array([3.0, 5.0, 7.0])             # what the epoch state holds before the first call: it must be added to
STALE = (12345.0, 678.0, 91.0, 17.0)               # the partials an earlier, larger call is taken to have left (integers: exact cases stay exact)
REG_DAMAGES = ("drop_last_element", "drop_partial", "stale_partial", "n_minus_1", "abs_is_squares", "batch_accumulated", "epoch_overwritten", "fp32_sums")


def _reg_case(kind, pred, y, n, entry, epoch0):
    nt, blocks = geometry("reg", n, entry)
    return {"kind": kind, "pred": pred, "y": y, "n": n, "nt": nt, "blocks": blocks, "entry": entry,
            "epoch0": REG_EPOCH0.copy() if epoch0 is None else np.asarray(epoch0, dtype=np.float64).copy()}


def exact_reg(n, entry="step", seed=0, epoch0=None):
    """Integers of magnitude <= 64: every term and every partial sum is an integer below 2^53, each addition exact in any order.  The last residual is +-3
    (a dropped last element, or squares in the abs column, change the sums at every n)."""
    rng = np.random.default_rng(1000 * seed + n)
    pred, y = rng.integers(-64, 65, n).astype(np.float32), rng.integers(-64, 65, n).astype(np.float32)
    y[-1] = pred[-1] - 3 if pred[-1] > 0 else pred[-1] + 3
    d = pred.astype(np.float64) - y
    assert np.abs(pred).max() <= 64 and np.abs(y).max() <= 64 and (d == np.round(d)).all() and float((d * d).sum()) < 2.0 ** 53
    return _reg_case("exact", pred, y, n, entry, epoch0)


def _binade(rng, shape):
    mag = np.minimum(rng.uniform(1.0, 4.0, shape).astype(np.float32), np.nextafter(np.float32(4.0), np.float32(0.0)))
    return (mag * rng.choice(np.array([-1.0, 1.0], dtype=np.float32), shape)).astype(np.float32)


def assert_binade_residuals(d):
    """Every residual is a multiple of 2^-23 below 8 (26 bits), so its square (52 bits) is exact in fp64."""
    k = d * 2.0 ** 23
    assert (k == np.round(k)).all() and (np.abs(d) < 8.0).all()
    ki = np.abs(k).astype(np.int64)
    assert (ki * ki < 2 ** 53).all() and ((ki * ki).astype(np.float64) * 2.0 ** -46 == d * d).all()


def binade_reg(n, entry="step", seed=0, epoch0=None):
    """fp32 values with random sign and magnitude in [1, 4): the sums round, and the order mirror must give the device's bits."""
    rng = np.random.default_rng(2000 * seed + n + 7)
    pred, y = _binade(rng, n), _binade(rng, n)
    pred[-1], y[-1] = 1.2345678, -2.3456789                      # (the last residual's square needs more than fp32's 24 bits)
    d = pred.astype(np.float64) - y
    assert np.float64(np.float32(d[-1] * d[-1])) != d[-1] * d[-1]
    assert_binade_residuals(d)
    return _reg_case("binade", pred, y, n, entry, epoch0)


def reg_expected(case, damage=None):
    """{"batch": [8], "epoch": [3]} after one call on `case` (batch: only the step entry writes it), or None where `damage` has no meaning for the case."""
    nt, blocks, n = case["nt"], case["blocks"], case["n"]
    d = case["pred"].astype(np.float64) - case["y"].astype(np.float64)
    kw, dtype = {}, np.float64
    if damage == "drop_last_element":
        d = d.copy()
        d[-1] = 0.0
    elif damage == "drop_partial":
        if blocks == 1:
            return None
        kw["skip_block"] = blocks - 1
    elif damage == "stale_partial":
        if blocks == MET_BLOCKS or case["entry"] == "acc":
            return None
    elif damage == "fp32_sums":
        if case["kind"] == "exact":
            return None                     # integers: an fp32 sum below 2^24 is as exact as the fp64 one, by design of the case
        dtype = np.float32
    elif damage == "batch_accumulated" and case["entry"] == "acc":
        return None
    sq = order_sum((d * d).astype(dtype), nt, blocks, dtype, stale=STALE[0] if damage == "stale_partial" else None, **kw)
    ab = order_sum(np.abs(d).astype(dtype), nt, blocks, dtype, stale=STALE[1] if damage == "stale_partial" else None, **kw)
    if damage == "abs_is_squares":
        ab = sq
    cnt = np.float64(n - 1 if damage == "n_minus_1" else n)
    sums = np.array([sq, ab, cnt])
    if damage == "batch_accumulated":
        sums = BATCH_FILL + sums
    with np.errstate(divide="ignore", invalid="ignore"):
        batch = np.array([sums[0], sums[1], sums[2], sums[0] / sums[2], np.sqrt(sums[0] / sums[2]), sums[1] / sums[2], 0.0, 0.0])
    epoch = np.array([sq, ab, cnt]) if damage == "epoch_overwritten" else case["epoch0"] + np.array([sq, ab, cnt])
    return {"batch": batch, "epoch": epoch}


def reg_check(case, batch, epoch):
    """None, or what differs: batch[0..7] (None: not given to the call) and epoch[0..2] (likewise) bit for bit."""
    want = reg_expected(case)
    for got, key in ((batch, "batch"), (epoch, "epoch")):
        if got is not None:
            d = first_bit_mismatch(got, want[key], key)
            if d:
                return d
    return None


# ---------------------------------------------------------------------------------------------------
# classification
# ---------------------------------------------------------------------------------------------------
CLS_B = [1, 63, 64, 65, 255, 256, 257, 513, 16383, 16384, 16385, 16643]
CLS_ACC_B = [1, 1023, 1025, 3000]
GAP = 1.0e4
MIN_GAP = 2.0 ** -20
PRODUCT_MARGIN = 1e-9
CLS_CE0 = np.array([11.0, 13.0])
CLS_COUNTS0 = np.arange(100, 100 + N_COUNTS, dtype=np.int64)
CLS_DAMAGES = ("drop_last_element", "drop_partial", "stale_partial", "batch_accumulated", "epoch_overwritten", "labels_equal_1", "last_maximum_wins",
               "foot0_low_bit", "fp_fn_swapped", "f1_nan_kept", "ce_unrounded", "fp32_sums")


def cls_windows(logits, labels, equal_1=False, last_wins=False, foot0_low=False):
    """Per window: the four per-foot cross-entropy terms [B][4] and the 18 counters [B][18] (counts[0] = 1, [1] = the 16-class argmax equals the label state,
    [2 + 4 k ..] = tp, fp, fn, tn of leg k), in the kernel's formulas; also the 16 products [B][16]."""
    lg = np.asarray(logits, dtype=np.float64).reshape(-1, 4, 2)
    lab = (np.asarray(labels).reshape(-1, 4) == 1) if equal_1 else (np.asarray(labels).reshape(-1, 4) != 0)
    B = lg.shape[0]
    l0, l1 = lg[..., 0], lg[..., 1]
    m = np.maximum(l0, l1)
    e0, e1 = np.exp(l0 - m), np.exp(l1 - m)
    se = e0 + e1
    terms = (m + np.log(se)) - np.where(lab, l1, l0)
    p0, p1 = e0 / se, e1 / se
    pred = (p1 >= p0) if last_wins else (p1 > p0)
    counts = np.zeros((B, N_COUNTS), dtype=np.int64)
    counts[:, 0] = 1
    for k in range(4):
        for j, cell in enumerate((pred[:, k] & lab[:, k], pred[:, k] & ~lab[:, k], ~pred[:, k] & lab[:, k], ~pred[:, k] & ~lab[:, k])):
            counts[:, 2 + 4 * k + j] = cell
    prods = np.empty((B, 16))
    for j in range(16):
        bit = [j & 1, j & 2, j & 4, j & 8] if foot0_low else [j & 8, j & 4, j & 2, j & 1]
        f = [np.where(bit[k] != 0, p1[:, k], 1.0 - p1[:, k]) for k in range(4)]
        prods[:, j] = (f[0] * f[1]) * (f[2] * f[3])
    best = (15 - np.argmax(prods[:, ::-1], axis=1)) if last_wins else np.argmax(prods, axis=1)
    state = 8 * lab[:, 0] + 4 * lab[:, 1] + 2 * lab[:, 2] + 1 * lab[:, 3]
    counts[:, 1] = best == state
    return terms, counts, prods


def f1_of(tp, fp, fn, keep_nan=False):
    """BinaryF1Score's operation order; 0/0 -> 0."""
    with np.errstate(divide="ignore", invalid="ignore"):
        tp, fp, fn = np.float64(tp), np.float64(fp), np.float64(fn)
        precision, recall = tp / (tp + fp), tp / (tp + fn)
        f1 = 2.0 * (precision * recall) / (precision + recall)
    return f1 if keep_nan or f1 == f1 else np.float64(0.0)


def cls_published(ce_sum, counts, B, unrounded=False, keep_nan=False):
    """batch_ce[0..7] from the cross-entropy sum and the 18 counters."""
    out = np.zeros(8)
    out[0], out[1] = ce_sum, 4.0 * B
    out[2] = (np.float64(ce_sum) if unrounded else np.float64(np.float32(ce_sum))) / np.float64(4 * B)
    with np.errstate(divide="ignore", invalid="ignore"):
        out[3] = np.float64(counts[1]) / np.float64(counts[0])
    for k in range(4):
        out[4 + k] = f1_of(counts[2 + 4 * k], counts[3 + 4 * k], counts[4 + 4 * k], keep_nan)
    return out


def cls_case(B, entry="step", seed=0):
    """Random logits (scale 3) and labels from {0, 1, 2, -1} with the ties, the saturated pairs and the empty F1 cells planted (tests docstring); window 0 is
    built by hand so that one window already tells every damage: foot 0 a missed contact with label 2, foot 1 an equal pair, foot 3 a false alarm -- label
    state 8, best class 1.  Odd B: leg 1 never holds tp, fp or fn, leg 2 never a tp (prediction = not label): the two 0/0 paths of F1."""
    rng = np.random.default_rng(3000 * seed + B + 13)
    lg = (rng.standard_normal((B, 4, 2)) * 3.0).astype(np.float32)
    lab = rng.choice(np.array([0, 1, 2, -1], dtype=np.int32), (B, 4), p=[0.5, 0.3, 0.1, 0.1]).astype(np.int32)
    flat = lg.reshape(B * 4, 2)
    flab = lab.reshape(B * 4)
    idx = np.arange(B * 4)
    flat[idx % 7 == 5, 1] = flat[idx % 7 == 5, 0]                     # equal pairs: p = 1/2 exactly, no-contact wins
    sat = idx % 13 == 3                                              # saturated pairs: exp underflows to 0, p = 0 or 1, the term is 0 or GAP exactly
    side = (idx // 13) % 2
    flat[sat, 0], flat[sat, 1] = np.where(side[sat] == 0, GAP, 0.0), np.where(side[sat] == 0, 0.0, GAP)
    flab[sat] = np.where((idx[sat] // 13) % 5 == 4, 1 - side[sat], side[sat])      # one in five disagrees with its label: a term of 1e4
    if B % 2 == 1:
        lg[:, 1, 0] = lg[:, 1, 1] + np.abs(lg[:, 1, 0] - lg[:, 1, 1])       # leg 1: no-contact predicted (or a tie, which no-contact wins) ...
        lab[:, 1] = 0                                                       # ... and no contact labelled: tn only
        hi, lo = np.maximum(lg[:, 2, 0], lg[:, 2, 1]) + 1.0, np.minimum(lg[:, 2, 0], lg[:, 2, 1])
        contact = lab[:, 2] != 0
        lg[:, 2, 0], lg[:, 2, 1] = np.where(contact, hi, lo), np.where(contact, lo, hi)      # leg 2: the prediction is the opposite of the label
    lg[np.arange(B) % 11 == 2] = 0.75                                # whole windows of equal logits: all 16 products tie, class 0 wins (legs 1, 2: tn / fn)
    lg[0] = np.array([[1.5, -2.0], [0.75, 0.75], [1.0, -1.0], [0.5, 2.0]], dtype=np.float32)
    lab[0] = np.array([2, 0, 0, 0], dtype=np.int32)
    gap = np.abs(lg[..., 1].astype(np.float64) - lg[..., 0])
    close = (gap > 0) & (gap < MIN_GAP)
    lg[close, 1] = lg[close, 0]
    nt, blocks = geometry("cls", B, entry)
    case = {"kind": "cls", "logits": lg, "labels": lab, "B": B, "nt": nt, "blocks": blocks, "entry": entry, "ce0": CLS_CE0.copy(), "counts0": CLS_COUNTS0.copy()}
    assert_cls_condition(case)
    return case


def assert_cls_condition(case):
    """Every pair has gap 0 or >= 2^-20, and in every window the best and the second-best of the 16 products are equal or more than 1e-9 (relative) apart:
    the last bits of exp cannot move a counter."""
    lg = case["logits"].astype(np.float64)
    gap = np.abs(lg[..., 1] - lg[..., 0])
    assert ((gap == 0) | (gap >= MIN_GAP)).all()
    _, _, prods = cls_windows(case["logits"], case["labels"])
    top = np.sort(prods, axis=1)[:, ::-1]
    assert ((top[:, 0] == top[:, 1]) | (top[:, 0] - top[:, 1] > PRODUCT_MARGIN * top[:, 0])).all()
    assert set(np.unique(case["labels"]).tolist()) <= {0, 1, 2, -1} and case["labels"].dtype == np.int32


def cls_expected(case, damage=None):
    """{"terms", "ce" (math.fsum of the terms), "abs" (sum |terms|), "counts", "ce_b" [8], "counts_b" [18], "ce_e" [2], "counts_e" [18]}, or None."""
    B, nt, blocks = case["B"], case["nt"], case["blocks"]
    terms, counts, _ = cls_windows(case["logits"], case["labels"], equal_1=damage == "labels_equal_1", last_wins=damage == "last_maximum_wins",
                                   foot0_low=damage == "foot0_low_bit")
    keep = np.ones(B, dtype=bool)
    if damage == "drop_last_element":
        keep[-1] = False
    elif damage == "drop_partial":
        if blocks == 1:
            return None
        keep = block_of(B, nt, blocks) != blocks - 1
    elif damage == "stale_partial" and blocks == MET_BLOCKS:
        return None
    if case["entry"] == "acc" and damage in ("stale_partial", "batch_accumulated", "ce_unrounded", "f1_nan_kept"):
        return None                                  # (the accumulating entry has no scratch and no batch state)
    t = terms[keep].ravel()
    if damage == "fp32_sums":
        ce = float(order_sum(t.astype(np.float32).reshape(-1, 4), nt, blocks, np.float32))
    else:
        ce = math.fsum(t)
    c = counts[keep].sum(axis=0)
    if damage == "stale_partial":
        ce += STALE[0]
        c = c + np.arange(1, N_COUNTS + 1)
    if damage == "fp_fn_swapped":
        c = c.copy()
        for k in range(4):
            c[3 + 4 * k], c[4 + 4 * k] = c[4 + 4 * k], c[3 + 4 * k]
    if damage == "f1_nan_kept" and all(c[2 + 4 * k] + c[3 + 4 * k] > 0 and c[2 + 4 * k] > 0 for k in range(4)):
        return None                                  # (no leg of this case divides 0 by 0: even B)
    ce_s, c_s = (BATCH_FILL + ce, c + 7) if damage == "batch_accumulated" else (ce, c)
    ce_b = cls_published(ce_s, c_s, B, unrounded=damage == "ce_unrounded", keep_nan=damage == "f1_nan_kept")
    if damage == "batch_accumulated":
        ce_b[1] += BATCH_FILL
    over = damage == "epoch_overwritten"
    return {"terms": t, "ce": ce, "abs": math.fsum(np.abs(t)), "counts": c, "ce_b": ce_b, "counts_b": c_s,
            "ce_e": np.array([ce, 4.0 * B]) + (0.0 if over else case["ce0"]), "counts_e": c + (0 if over else case["counts0"])}


def ce_bound(want, K):
    m = want["terms"].size
    return gamma(m + 4) * want["abs"] + K * U * want["abs"]


def ce_ratio(case, ce_got):
    """|device sum - fsum| over the gamma bound alone (K = 0): what the GPU file's docstring records."""
    want = cls_expected(case)
    return abs(float(ce_got) - want["ce"]) / ce_bound(want, 0)


def cls_check(case, ce_b, counts_b, ce_e, counts_e, K):
    """None, or what is wrong.  Counters, ce_b[1], ce_b[3..7], ce_e[1]: exact.  ce_b[0], ce_e[0] - ce0: within `ce_bound`.  ce_b[2]: float32(the ce_b[0] GIVEN) /
    (4 B), bit for bit.  A pair that was not given to the call is None."""
    want = cls_expected(case)
    bound = ce_bound(want, K)
    if counts_b is not None:
        counts_b, ce_b = np.asarray(counts_b, dtype=np.int64), np.asarray(ce_b, dtype=np.float64)
        if not np.array_equal(counts_b, want["counts_b"]):
            i = int(np.nonzero(counts_b != want["counts_b"])[0][0])
            return f"batch counter {i} is {counts_b[i]}, the reference has {want['counts_b'][i]}"
        if not abs(ce_b[0] - want["ce"]) <= bound:
            return f"batch CE sum {ce_b[0]!r} is {abs(ce_b[0] - want['ce']):.3e} from {want['ce']!r}, the bound is {bound:.3e}"
        pub = cls_published(ce_b[0], counts_b, case["B"])
        d = first_bit_mismatch(ce_b[1:], pub[1:], "batch_ce[1:] from the call's own sum and counters: slot 1 + ")
        if d:
            return d
    if counts_e is not None:
        counts_e, ce_e = np.asarray(counts_e, dtype=np.int64), np.asarray(ce_e, dtype=np.float64)
        if not np.array_equal(counts_e, want["counts_e"]):
            i = int(np.nonzero(counts_e != want["counts_e"])[0][0])
            return f"epoch counter {i} is {counts_e[i]}, the reference has {want['counts_e'][i]}"
        if ce_e[1] != want["ce_e"][1]:
            return f"epoch rows {ce_e[1]!r}, the reference has {want['ce_e'][1]!r}"
        slack = bound + U * abs(want["ce_e"][0])                      # (the addition into the state rounds once more)
        if not abs(ce_e[0] - (case["ce0"][0] + want["ce"])) <= slack:
            return f"epoch CE sum {ce_e[0]!r} is {abs(ce_e[0] - (case['ce0'][0] + want['ce'])):.3e} from the reference, the bound is {slack:.3e}"
    return None


# ---------------------------------------------------------------------------------------------------
# centroidal momentum
# ---------------------------------------------------------------------------------------------------
COM_B = [1, 64, 257, 16385]
COM_NB = [1, 4]
COM_EPOCH0 = np.array([2.0, 4.0, 6.0, 8.0, 10.0, 12.0, 14.0, 16.0])
TINY = 2.0 ** -30                    # a vector this long is below eps = 1e-8 before and after un-standardising by 2: the clamp divides it by 1e-8
EDGE = 2.0 ** -27                    # below eps standardised (7.45e-9), above it after un-standardising by 2 (1.49e-8)
COM_DAMAGES = ("drop_last_element", "drop_partial", "stale_partial", "n_minus_1", "batch_accumulated", "epoch_overwritten", "lin_ang_swapped",
               "cosine_on_base_1", "cosine_standardised", "no_eps_clamp", "fp32_sums")


def com_cosines(pred, y, nb, mean, std, base=0, standardised=False, clamp=True, dtype=np.float64):
    """Per window (cos(lin_pred, lin), cos(ang_pred, ang)) [B][2] of base node `base`: CosineSimilarity(dim=1, eps=1e-8) after v * std + mean, in the
    kernel's operation order."""
    p = np.asarray(pred, dtype=dtype).reshape(-1, nb, 6)[:, base]
    t = np.asarray(y, dtype=dtype).reshape(-1, nb, 6)[:, base]
    if not standardised:
        p, t = p * np.asarray(std, dtype=dtype) + np.asarray(mean, dtype=dtype), t * np.asarray(std, dtype=dtype) + np.asarray(mean, dtype=dtype)
    out = np.empty((p.shape[0], 2), dtype=dtype)
    with np.errstate(divide="ignore", invalid="ignore"):
        for h in range(2):
            a, b = p[:, 3 * h:3 * h + 3], t[:, 3 * h:3 * h + 3]
            an = np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2])
            bn = np.sqrt((b[:, 0] * b[:, 0] + b[:, 1] * b[:, 1]) + b[:, 2] * b[:, 2])
            if clamp:
                an, bn = np.maximum(an, dtype(EPS)), np.maximum(bn, dtype(EPS))
            q = (a / an[:, None]) * (b / bn[:, None])
            out[:, h] = (q[:, 0] + q[:, 1]) + q[:, 2]
    return out


def com_window_bound(pred, y, nb, mean, std):
    """[B][2]: how far one window's fp64 cosine may lie from its true value (module docstring)."""
    out = []
    mean, std = np.asarray(mean, dtype=np.float64), np.asarray(std, dtype=np.float64)
    vec = []
    for x in (pred, y):
        x0 = np.asarray(x, dtype=np.float64).reshape(-1, nb, 6)[:, 0]
        v = x0 * std + mean
        vec.append((v, U * (np.abs(x0 * std) + np.abs(v))))
    for h in range(2):
        sl = slice(3 * h, 3 * h + 3)
        (p, dp), (t, dt) = [(v[:, sl], e[:, sl]) for v, e in vec]
        pn, tn = np.linalg.norm(p, axis=1), np.linalg.norm(t, axis=1)
        assert (pn > 1e-6).all() and (tn > 1e-6).all(), "com_random keeps clear of the eps clamp"
        out.append(2.0 * (dp.sum(axis=1) / pn + dt.sum(axis=1) / tn) + COS_ROUNDINGS * U * (np.abs(p * t).sum(axis=1) / (pn * tn)))
    return np.stack(out, axis=1)


def _com_case(kind, pred, y, B, nb, mean, std):
    nt, blocks = geometry("com", B)
    return {"kind": kind, "pred": pred, "y": y, "B": B, "nb": nb, "mean": np.asarray(mean, dtype=np.float64), "std": np.asarray(std, dtype=np.float64),
            "nt": nt, "blocks": blocks, "entry": "step", "epoch0": COM_EPOCH0.copy()}


def com_exact(B, nb, seed=0):
    """Integer residuals (in the planted windows: small multiples of 2^-30, squares still exact); the two halves of base node 0 lie on coordinate axes with power-of-two lengths, mean = 0, std in {1, 2}: every cosine is exactly
    1, -1 or 0.  Planted by window index: zero vectors (the clamp gives 0 / 1e-8 = 0), vectors of length 2^-30 in both operands (each is divided by 1e-8: the
    term is fl(fl(2^-30 / 1e-8)^2), the sums round and the order mirror follows them), and a vector of length 2^-27 on an axis of std 2 (above eps only
    after un-standardising: cos = 1, where the standardised values would give 2^-27 / 1e-8 = 0.745).  Window 0 holds a tiny lin pair and such an ang pair."""
    rng = np.random.default_rng(4000 * seed + 10 * B + nb)
    pred = rng.integers(-8, 9, (B, nb, 6)).astype(np.float64)
    y = rng.integers(-8, 9, (B, nb, 6)).astype(np.float64)
    std = np.array([1.0, 2.0, 1.0, 2.0, 1.0, 2.0])
    w = np.arange(B)
    axis_p, axis_y = rng.integers(0, 3, (B, 2)), rng.integers(0, 3, (B, 2))
    axis_y[w % 3 != 1] = axis_p[w % 3 != 1]             # two thirds of the windows share the axis: +-1 is as common as 0
    for x, axis in ((pred, axis_p), (y, axis_y)):
        length = 2.0 ** rng.integers(0, 4, (B, 2)) * rng.choice([-1.0, 1.0], (B, 2))
        x[:, 0, :] = 0.0
        for h in range(2):
            x[w, 0, 3 * h + axis[:, h]] = length[:, h]
    pred[w % 7 == 4, 0, 0:3] = 0.0
    y[w % 7 == 5, 0, 3:6] = 0.0
    tiny = w % 5 == 0
    pred[tiny, 0, 0:3], y[tiny, 0, 0:3] = [TINY, 0.0, 0.0], [-TINY, 0.0, 0.0]
    edge = w % 9 == 0
    pred[edge, 0, 3:6], y[edge, 0, 3:6] = [EDGE, 0.0, 0.0], [2 * EDGE, 0.0, 0.0]              # ang x: std 2
    if B > 1:                                           # the last window's residuals are 3 in both halves, its cosines 1 and -1
        pred[-1, 0], y[-1, 0] = [4.0, 0.0, 0.0, 0.0, 2.0, 0.0], [1.0, 0.0, 0.0, 0.0, -1.0, 0.0]
    pred, y = pred.astype(np.float32), y.astype(np.float32)
    case = _com_case("exact", pred, y, B, nb, np.zeros(6), std)
    d = pred.astype(np.float64) - y
    assert all(Fraction(float(v)) ** 2 == Fraction(float(v * v)) for v in np.unique(np.abs(d)))      # every square is exact in fp64
    cos = com_cosines(pred, y, nb, case["mean"], case["std"])
    c2 = (TINY / EPS) * (-TINY / EPS)
    assert np.isin(cos, [0.0, 1.0, -1.0, c2]).all() and c2 != -1.0
    return case


def com_random(B, nb, seed=0):
    """Binade values (exact squares of the residuals: slots 0 and 1 by the order mirror's bits) under a random mean and a std in [0.5, 1.5]; also returns
    the per-window bound of the cosines, and refuses data whose bound exceeds 1e-13 in any window."""
    rng = np.random.default_rng(5000 * seed + 10 * B + nb + 3)
    pred, y = _binade(rng, (B, nb, 6)), _binade(rng, (B, nb, 6))
    pred[-1, -1, 2], y[-1, -1, 2], pred[-1, -1, 5], y[-1, -1, 5] = 1.2345678, -2.3456789, 3.4567891, -1.1234567
    assert_binade_residuals(pred.astype(np.float64) - y)
    case = _com_case("random", pred, y, B, nb, rng.standard_normal(6), rng.uniform(0.5, 1.5, 6))
    case["window_bound"] = com_window_bound(pred, y, nb, case["mean"], case["std"])
    assert float(case["window_bound"].max()) <= COM_WINDOW_LIMIT, "com_random: a window's cosine is too ill-conditioned for this seed"
    return case


def com_expected(case, damage=None):
    """{"batch": [8], "epoch": [8], "cos_bound": [2]} (cos_bound: 0 on exact data), or None."""
    B, nb, nt, blocks = case["B"], case["nb"], case["nt"], case["blocks"]
    exact = case["kind"] == "exact"
    pred, y = case["pred"], case["y"]
    d = pred.astype(np.float64) - y.astype(np.float64)
    kw, dtype = {}, np.float64
    keep = np.ones(B, dtype=bool)
    if damage == "drop_last_element":
        keep[-1] = False
    elif damage == "drop_partial":
        if blocks == 1:
            return None
        kw["skip_block"] = blocks - 1
        keep = block_of(B, nt, blocks) != blocks - 1
    elif damage == "stale_partial":
        if blocks == MET_BLOCKS:
            return None
    elif damage == "fp32_sums":
        if exact:
            return None
        dtype = np.float32
    elif damage == "cosine_on_base_1" and nb == 1:
        return None
    elif damage == "no_eps_clamp" and not exact:
        return None                                  # (com_random keeps clear of the clamp)
    d = d * keep[:, None, None]
    stale = STALE if damage == "stale_partial" else (None,) * 4
    lin = order_sum((d[:, :, :3] ** 2).reshape(B, nb * 3).astype(dtype), nt, blocks, dtype, stale=stale[0], **kw)
    ang = order_sum((d[:, :, 3:] ** 2).reshape(B, nb * 3).astype(dtype), nt, blocks, dtype, stale=stale[1], **kw)
    args = dict(base=1 if damage == "cosine_on_base_1" else 0, standardised=damage == "cosine_standardised", clamp=damage != "no_eps_clamp")
    if exact or damage is not None:
        cos = com_cosines(pred, y, nb, case["mean"], case["std"], dtype=dtype, **args) * keep[:, None].astype(dtype)
        c = [order_sum(cos[:, h], nt, blocks, dtype, stale=stale[2 + h], **kw) for h in range(2)]
    else:
        cos = com_cosines(pred, y, nb, case["mean"].astype(EXT), case["std"].astype(EXT), dtype=EXT)
        c = [np.float64(cos[:, h].sum()) for h in range(2)]
    n3, nB = 3.0 * nb * B, np.float64(B)
    if damage == "n_minus_1":
        n3, nB = 3.0 * nb * B - 1, np.float64(B - 1)
    v = np.array([lin, ang, n3, n3, c[0], c[1], nB, 0.0])
    if damage == "lin_ang_swapped":
        v = v[[1, 0, 2, 3, 5, 4, 6, 7]]
    bound = np.zeros(2) if exact else case["window_bound"].sum(axis=0) + gamma(B + 4) * B
    return {"batch": (BATCH_FILL + v) if damage == "batch_accumulated" else v, "epoch": v if damage == "epoch_overwritten" else case["epoch0"] + v,
            "cos_bound": bound}


def com_check(case, batch, epoch):
    """None, or what is wrong: every slot bit for bit, but the cosine sums of random data within the sum of the windows' bounds + gamma_(B + 4) * B."""
    want = com_expected(case)
    exact = case["kind"] == "exact"
    for got, key in ((batch, "batch"), (epoch, "epoch")):
        if got is None:
            continue
        got = np.asarray(got, dtype=np.float64)
        sl = list(range(8)) if exact else [0, 1, 2, 3, 6, 7]
        d = first_bit_mismatch(got[sl], want[key][sl], f"{key}{sl}")
        if d:
            return d
        if not exact:
            for h in range(2):
                slack = want["cos_bound"][h] + (U * abs(want[key][4 + h]) if key == "epoch" else 0.0)
                if not abs(got[4 + h] - want[key][4 + h]) <= slack:
                    return f"{key}[{4 + h}] = {got[4 + h]!r} is {abs(got[4 + h] - want[key][4 + h]):.3e} from {want[key][4 + h]!r}, the bound is {slack:.3e}"
    return None


def com_ratio(case, batch):
    want = com_expected(case)
    return max(abs(float(batch[4 + h]) - want["batch"][4 + h]) / want["cos_bound"][h] for h in range(2))


# ---------------------------------------------------------------------------------------------------
# GRF rotation
# ---------------------------------------------------------------------------------------------------
GRF_B = [1, 255, 256, 257, 1000]
GRF_DAMAGES = ("forward_rotation", "scalar_first", "unnormalised", "drop_last_element", "fp32_sums")


def rotation_matrices(quat, scalar_first=False, normalise=True, dtype=np.float64, majorant=False):
    """R(q / |q|) [B][3][3] of scalar-last quaternions in the kernel's formulas; majorant: every term of every entry in absolute value."""
    q = np.asarray(quat, dtype=dtype).reshape(-1, 4)
    if scalar_first:
        q = q[:, [1, 2, 3, 0]]
    if normalise:
        q = q / np.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3])[:, None]
    if majorant:
        q = np.abs(q)
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    s = 1 if majorant else -1
    one, two = dtype(1.0), dtype(2.0)
    R = [[one + s * two * (y * y + z * z), two * (x * y + s * z * w), two * (x * z + y * w)],
         [two * (x * y + z * w), one + s * two * (x * x + z * z), two * (y * z + s * x * w)],
         [two * (x * z + s * y * w), two * (y * z + x * w), one + s * two * (x * x + y * y)]]
    return np.stack([np.stack(r, axis=-1) for r in R], axis=1)


def grf_rotate(quat, body, forward=False, dtype=np.float64, **kw):
    """world [B][12] = R^T f per foot (forward: R f, the damage)."""
    R = rotation_matrices(quat, dtype=dtype, **kw)
    f = np.asarray(body, dtype=dtype).reshape(-1, 4, 3)
    if forward:
        R = R.transpose(0, 2, 1)
    out = (R[:, None, 0, :] * f[:, :, 0:1] + R[:, None, 1, :] * f[:, :, 1:2]) + R[:, None, 2, :] * f[:, :, 2:3]
    return out.reshape(-1, 12)


def ulp32(x):
    _, e = np.frexp(np.abs(np.asarray(x, dtype=np.float64)))
    return np.ldexp(1.0, np.maximum(e - 1, -126) - 23)


def grf_bound(case):
    A = rotation_matrices(case["quat"], majorant=True)
    f = np.abs(case["body"].astype(np.float64)).reshape(-1, 4, 3)
    return 0.5 * ulp32(case["want"]) + 16 * U * np.einsum("nji,nfj->nfi", A, f).reshape(-1, 12)


_UNIT = [(0, 0, 0, 1), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0)] + [(a, b, c, d) for a in (1, -1) for b in (1, -1) for c in (1, -1) for d in (1, -1)]


def grf_exact(B, seed=0):
    """Quaternions whose norm is a power of two and whose matrix is a signed permutation: the identity, the three half turns about the axes, and the sixteen
    (+-1, +-1, +-1, +-1) (norm 2: thirds of a turn about a diagonal, a signed CYCLIC permutation, so R != R^T), each also scaled by 2 and by -1.  The forces
    are distinct in every component and sign-asymmetric: the output is a signed copy of input bits.  Window 0 is (2, 2, 2, -2)."""
    rng = np.random.default_rng(6000 * seed + B)
    pick = np.array(_UNIT, dtype=np.float64)[(np.arange(B) * 7 + 19) % len(_UNIT)]
    quat = (pick * np.array([1.0, 2.0, -1.0])[np.arange(B) % 3][:, None]).astype(np.float32)
    quat[0] = [2, 2, 2, -2]
    body = (rng.uniform(1.0, 50.0, (B, 12)) * np.tile([1.0, -1.0, 1.0, 1.0, 1.0, -1.0], 2)).astype(np.float32)
    want = grf_rotate(quat, body)
    R = rotation_matrices(quat)
    assert np.isin(R, [0.0, 1.0, -1.0]).all() and (np.abs(R).sum(axis=1) == 1).all() and (np.abs(R).sum(axis=2) == 1).all()
    assert (np.sort(np.abs(want), axis=1) == np.sort(np.abs(body.astype(np.float64)), axis=1)).all()
    return {"kind": "exact", "quat": quat, "body": body, "B": B, "want": want}


def grf_random(B, seed=0):
    """Random quaternions (not normalised) and forces scaled by 30; `want` in extended precision."""
    rng = np.random.default_rng(7000 * seed + B + 1)
    quat, body = rng.standard_normal((B, 4)).astype(np.float32), (rng.standard_normal((B, 12)) * 30.0).astype(np.float32)
    assert (np.linalg.norm(quat.astype(np.float64), axis=1) > 1e-3).all()
    return {"kind": "random", "quat": quat, "body": body, "B": B, "want": grf_rotate(quat, body, dtype=EXT)}


def grf_expected(case, damage=None):
    """fp32 [B][12], or None."""
    q, f = case["quat"], case["body"]
    if damage is None:
        return np.asarray(case["want"], dtype=np.float64).astype(np.float32)
    if damage == "fp32_sums":
        return None if case["kind"] == "exact" else grf_rotate(q, f, dtype=np.float32)
    if damage == "drop_last_element":
        out = grf_expected(case).copy()
        out[-1, -1] = -7.5                           # (the sentinel the output buffer was filled with)
        return out
    out = grf_rotate(q, f, forward=damage == "forward_rotation", scalar_first=damage == "scalar_first", normalise=damage != "unnormalised")
    return out.astype(np.float32)


def grf_check(case, got):
    got = np.asarray(got, dtype=np.float32).reshape(-1, 12)
    if case["kind"] == "exact":
        want = grf_expected(case)
        bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))
        if bad[0].size:
            i, j = int(bad[0][0]), int(bad[1][0])
            return f"world[{i}][{j}] = {got[i, j]!r}, the reference has {want[i, j]!r} ({bad[0].size} differ)"
        return None
    err, bound = np.abs(got.astype(EXT) - case["want"]).astype(np.float64), grf_bound(case)
    if not (err <= bound).all():
        i, j = np.unravel_index(int(np.argmax(err / bound)), err.shape)
        return f"world[{i}][{j}] = {got[i, j]!r} is {err[i, j]:.3e} from {float(case['want'][i, j])!r}, the bound is {bound[i, j]:.3e}"
    return None


# ---------------------------------------------------------------------------------------------------
DAMAGES = {"reg": REG_DAMAGES, "cls": CLS_DAMAGES, "com": COM_DAMAGES, "grf": GRF_DAMAGES}


def damaged(name, family, case):
    """What a kernel with the defect `name` would leave for `case` (the dictionary / array of the family's `*_expected`), or None where the defect cannot
    show in that case by construction (one workgroup has no partial to drop, a full grid no stale one, exact data no fp32 rounding, one base node no node 1)."""
    assert name in DAMAGES[family], name
    return {"reg": reg_expected, "cls": cls_expected, "com": com_expected, "grf": grf_expected}[family](case, name)


# ---------------------------------------------------------------------------------------------------
# the cases tests/test_metrics_exact_gpu.py runs (tests/test_metrics_reference.py holds the checkers against every one of them)
# ---------------------------------------------------------------------------------------------------
CE_K = 0          # the per-term allowance for the device's exp / log in `ce_bound`, in u: tests/test_metrics_exact_gpu.py states the measurement behind it
# one zeroed-once scratch serves these calls in a row: 64 workgroups, then 1, then 2, then 64 (elements for "reg", windows for "cls" / "com")
SCRATCH_SEQUENCE = {"reg": [262149, 100, 5000, 263000], "cls": [16400, 100, 300, 16390], "com": [16400, 100, 300, 16390]}
SCRATCH_COM_NB = 2
GRAPH_ITEMS = {"reg": 8193, "cls": 513, "com": 513}          # the captured step: three workgroups, so that the ticket is drawn and reset inside the graph


def all_cases():
    """(family, key) of every case; key = (maker name, size, ..., seed)."""
    out = []
    for seed in (0, 1):
        for kind in ("exact_reg", "binade_reg"):
            out += [("reg", (kind, n, "step", seed)) for n in REG_N] + [("reg", (kind, n, "acc", seed)) for n in REG_ACC_N]
        out += [("cls", ("cls_case", B, "step", seed)) for B in CLS_B] + [("cls", ("cls_case", B, "acc", seed)) for B in CLS_ACC_B]
        out += [("com", (kind, B, nb, seed)) for kind in ("com_exact", "com_random") for B in COM_B for nb in COM_NB]
    out += [("grf", (kind, B, 0)) for kind in ("grf_exact", "grf_random") for B in GRF_B]
    for k, n in enumerate(SCRATCH_SEQUENCE["reg"] + [GRAPH_ITEMS["reg"]] * 3):
        out.append(("reg", ("exact_reg", n, "step", 10 + k)))
    for k, B in enumerate(SCRATCH_SEQUENCE["cls"] + [GRAPH_ITEMS["cls"]] * 3):
        out.append(("cls", ("cls_case", B, "step", 20 + k)))
        out.append(("com", ("com_exact", B, SCRATCH_COM_NB, 10 + k)))
    return out


def build_case(family, key):
    maker = globals()[key[0]]
    return maker(*key[1:-1], seed=key[-1])


def check(family, case, result):
    """The family's checker on a result in the layout of its `*_expected`."""
    if family == "reg":
        return reg_check(case, result["batch"] if case["entry"] == "step" else None, result["epoch"])
    if family == "cls":
        step = case["entry"] == "step"
        return cls_check(case, result["ce_b"] if step else None, result["counts_b"] if step else None, result["ce_e"], result["counts_e"], CE_K)
    if family == "com":
        return com_check(case, result["batch"], result["epoch"])
    return grf_check(case, result)


def expected(family, case):
    return {"reg": reg_expected, "cls": cls_expected, "com": com_expected, "grf": grf_expected}[family](case)
