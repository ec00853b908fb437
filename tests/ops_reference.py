"""Host-side references, data and checkers for the stand-alone operators (csrc/mshgnn_ops.hip behind ops.py / nn.py): test infrastructure, no GPU.

Two kinds of data, two checkers, one rule for choosing between them:
  * exact data (`exact_operands`, `aggregate_case`, `colsum_case`): integer-valued fp32 operands (features, weights, biases, a pre-existing C in
    [-4, 4]; 'mean' scales that are powers of two) with a host proof, in fp64, that for EVERY output element the sum of the absolute values of its terms
    stays below 2^24 units of the terms' grid.  Every partial sum of every summation order is then an fp32 value: an fp32 FMA chain, split-K partial
    sums and two-stage column sums must give the fp64 result BIT FOR BIT (`first_mismatch`, no tolerance).  A case that does not close RAISES; nothing
    is rescaled silently.
  * random fp32 data under the derived per-element bound (`elementwise_bound`, `within_bound`):
        |got - ref| <= gamma_n (|A| |B|^T + |bias| + |C_in|),   gamma_n = n u / (1 - n u),   u = 2^-24,
    n the number of roundings on the element's path (K products-and-adds + split-K partial sums + bias + accumulate; aggregation: in-degree adds, for
    'mean' one more for fl32(1 / deg) and one for the scale product; column sums: M).  The bound holds for any summation order, fused or not (Higham,
    Accuracy and Stability of Numerical Algorithms, section 3.1), so it is derived, not measured.  Operands are drawn in fp32, the reference is evaluated
    in fp64 from those same fp32 values, the comparison is per element -- no normalisation by the tensor's maximum -- and an element whose bound is 0
    must be exactly 0.
  * The rule: gamma_n grows with n, so for long reductions the bound cannot see one dropped term (K = 131073: gamma_n = 8e-3).  `damaged_gemm` /
    `damaged_aggregate` / `damaged_colsum` build deliberately wrong results, and tests/test_ops_reference.py demands that the checker of every case of
    the GPU tables below rejects every one of them; a case the bound cannot police has to be an exact-data case.

The tables at the end (GEMM_*, AGG_*, COLSUM_*) are the cases of tests/test_ops_exact_gpu.py; the host tests iterate over the same objects.
"""
from functools import lru_cache

import torch

U = 2.0 ** -24
LIMIT = 2.0 ** 24
INT_RANGE = 4


class DoesNotClose(ValueError):
    """An exact-data case whose sums of |terms| reach 2^24 grid units: it cannot serve as a bit-exact reference."""


def gamma(n):
    """gamma_n = n u / (1 - n u) for an int or a tensor of ints (n u < 1 asserted)."""
    n = torch.as_tensor(n, dtype=torch.float64)
    assert bool((n * U < 1).all()), "n u >= 1: no bound"
    return n * U / (1 - n * U)


def _ints(g, shape, lo=-INT_RANGE, hi=INT_RANGE):
    return torch.randint(lo, hi + 1, shape, generator=g).to(torch.float32)


def _require_closure(sum_abs, grid_exp, what):
    """sum_abs: fp64 tensor of sums of |terms|; every one must be < 2^24 units of 2^grid_exp."""
    worst = float(sum_abs.max()) if sum_abs.numel() else 0.0
    if not worst < LIMIT * 2.0 ** grid_exp:
        raise DoesNotClose(f"{what}: a sum of |terms| {worst} reaches 2^24 units of 2^{grid_exp}")
    return worst / (LIMIT * 2.0 ** grid_exp)


# ---------------------------------------------------------------------------------------------------
# GEMM  C[m, n] (+)= sum_k A[m, k] B[n, k] (+ bias[n])
# ---------------------------------------------------------------------------------------------------
@lru_cache(maxsize=3)
def _gemm_base(M, N, K, seed, exact):
    g = torch.Generator().manual_seed(seed * 1000003 + M * 7919 + N * 104729 + K)
    if exact:
        A, B, bias, C = _ints(g, (M, K)), _ints(g, (N, K)), _ints(g, (N,)), _ints(g, (M, N))
        A[A == 0], B[B == 0], bias[bias == 0] = 3.0, -2.0, 3.0      # (no zeros: every product and every bias entry is a term whose loss shows)
    else:
        A, B = torch.randn(M, K, generator=g, dtype=torch.float32), torch.randn(N, K, generator=g, dtype=torch.float32)
        bias, C = torch.randn(N, generator=g, dtype=torch.float32), torch.randn(M, N, generator=g, dtype=torch.float32)
    A64, B64 = A.double(), B.double()
    prod = A64 @ B64.t()
    absprod = A64.abs() @ B64.abs().t()
    return A, B, bias, C, prod, absprod


def gemm_operands(M, N, K, seed=1, exact=True, bias=False, accumulate=False, splits=1):
    """Operands (fp32, logical shapes A [M, K], B [N, K], bias [N] | None, C_in [M, N] | None), the fp64 reference `ref`, the sums of |terms| `sum_abs`
    and, for random data, the per-element `bound` with n = K + splits + bias + accumulate.  exact=True: integer data, closure proven or DoesNotClose."""
    A, B, b, C, prod, absprod = _gemm_base(M, N, K, seed, exact)
    ref, sum_abs = prod.clone(), absprod.clone()
    if bias:
        ref += b.double()
        sum_abs += b.double().abs()
    if accumulate:
        ref += C.double()
        sum_abs += C.double().abs()
    case = dict(M=M, N=N, K=K, A=A, B=B, bias=b if bias else None, C_in=C if accumulate else None, ref=ref, sum_abs=sum_abs, exact=exact, splits=splits)
    if exact:
        case["closure"] = _require_closure(sum_abs, 0, f"gemm {M} x {N} x {K}")
        assert torch.equal(ref.float().double(), ref)      # (an integer below 2^24: the cast of the reference to fp32 is exact)
        case["bound"] = None
    else:
        case["n"] = K + splits + int(bias) + int(accumulate)
        case["bound"] = elementwise_bound(A.double().abs(), B.double().abs(), case["n"], b if bias else None, C if accumulate else None, absprod=absprod)
    return case


def exact_operands(M, N, K, seed=1, bias=False, accumulate=False):
    """Integer-valued fp32 GEMM operands with the host proof that every output element's sum_k |a| |b| + |bias| + |C_in| < 2^24 (raises DoesNotClose)."""
    return gemm_operands(M, N, K, seed, True, bias, accumulate)


def elementwise_bound(absA, absB, n_adds, abs_bias=None, abs_c=None, absprod=None):
    """gamma_n (|A| |B|^T + |bias| + |C_in|) in fp64: absA [M, K], absB [N, K] (absolute values are taken here as well), n_adds an int or a per-row /
    per-element tensor broadcastable to [M, N]."""
    s = absprod.clone() if absprod is not None else absA.double().abs() @ absB.double().abs().t()
    if abs_bias is not None:
        s = s + abs_bias.double().abs()
    if abs_c is not None:
        s = s + abs_c.double().abs()
    return gamma(n_adds) * s


def within_bound(got, ref, bound, where=None):
    """None when every element of `got` lies within `bound` of `ref` (bound 0: equal; a NaN never passes), else a description of the first few
    offenders: index, got, want, error, bound, and `where(index)` (the tile / wave / K chunk of the element)."""
    got = got.detach().double().cpu().reshape(ref.shape)
    bad = ~((got - ref).abs() <= bound)
    return _describe(bad, got, ref, where, bound)


def first_mismatch(got, ref, where=None):
    """None when `got` (fp32 / any float) equals the fp64 `ref` bit for bit after .double() (-0.0 == +0.0), else the first few (index, got, want)."""
    got = got.detach().double().cpu().reshape(ref.shape)
    if torch.equal(got, ref):
        return None
    bad = ~(got == ref)
    return _describe(bad, got, ref, where, None)


def _describe(bad, got, ref, where, bound):
    if not bool(bad.any()):
        return None
    idx = bad.nonzero()
    out = [f"{idx.shape[0]} of {ref.numel()} elements wrong"]
    for i in idx[:4]:
        t = tuple(int(v) for v in i)
        s = f"{t}: got {float(got[t])!r}, want {float(ref[t])!r}"
        if bound is not None:
            b = bound if bound.dim() == 0 else bound.expand(ref.shape)[t]
            s += f", bound {float(b):.3e}"
        if where is not None:
            s += f" [{where(t)}]"
        out.append(s)
    return "; ".join(out)


def gemm_where(K, splits):
    """Where a C element sits in k_op_gemm's tiling: 64 x 64 workgroup tile, 32 x 32 wave tile, and the K chunking of the launch."""
    kchunk = max(16, (-(-max(K, 1) // splits) + 15) // 16 * 16)

    def f(t):
        m, n = t
        return (f"tile ({m // 64}, {n // 64}), wave ({(m % 64) // 32}, {(n % 64) // 32}), lane column {n % 32}; {splits} K chunk(s) of {kchunk}, "
                f"{-(-K // 16)} K tile(s), last one {K % 16 or 16} wide")
    return f


GEMM_DAMAGES = ("drop_one_k", "drop_last_k_tile", "shift_row_tile", "bias_twice", "stale_element")


def damaged_gemm(case, kind):
    """A deliberately wrong result for `case` (fp64), or None where the damage does not exist for this case (no K, no bias, a single row):
      drop_one_k: one output element misses one of its K products -- the one of median magnitude among its non-zero ones, so that a checker has to see
                  a TYPICAL term, not the largest;   drop_last_k_tile: every element misses the products of the last 16-wide K tile;
      shift_row_tile: the rows of the last 64-row tile are the rows one further down (cyclically within the tile);   bias_twice;
      stale_element: one element still holds what the buffer held before the call (C_in when accumulating, else the NaN the tests poison with)."""
    M, N, K = case["M"], case["N"], case["K"]
    A, B, ref = case["A"].double(), case["B"].double(), case["ref"]
    bad = ref.clone()
    if kind == "drop_one_k":
        if K == 0:
            return None
        for m, n in ((M // 2, N // 2), (M - 1, N - 1), (0, 0)):
            terms = A[m] * B[n]
            nz = terms.abs().nonzero()[:, 0]
            if nz.numel():
                k = nz[terms[nz].abs().argsort()[nz.numel() // 2]]
                bad[m, n] -= terms[k]
                break
        else:
            return None
    elif kind == "drop_last_k_tile":
        if K == 0:
            return None
        k0 = (K - 1) // 16 * 16
        bad -= A[:, k0:] @ B[:, k0:].t()
    elif kind == "shift_row_tile":
        if M < 2:
            return None
        r0 = (M - 1) // 64 * 64
        if M - r0 < 2:
            r0 = max(0, r0 - 64)
        bad[r0:M] = ref[r0:M].roll(-1, 0)
    elif kind == "bias_twice":
        if case["bias"] is None:
            return None
        bad += case["bias"].double()
    elif kind == "stale_element":
        if case["C_in"] is None:
            bad[M - 1, N - 1] = float("nan")
        else:
            d = (case["C_in"].double() - ref).abs()
            m, n = divmod(int(d.argmax()), N)
            bad[m, n] = case["C_in"].double()[m, n]
    else:
        raise KeyError(kind)
    return None if torch.equal(bad, ref) else bad      # (e.g. rows of zeros shifted onto rows of zeros at K == 0: not a wrong result)


def reject(case_ref, bound, bad, where=None):
    """True when the case's checker (bit equality for exact data: bound None) rejects the result `bad`."""
    return (first_mismatch(bad, case_ref, where) if bound is None else within_bound(bad, case_ref, bound, where)) is not None


# ---------------------------------------------------------------------------------------------------
# aggregation  out[r, :] = sum_{e in row r} scale[e] x[col[e], :]
# ---------------------------------------------------------------------------------------------------
def make_graph(n_src, n_dst, seed, mode="random", hub=0):
    """A multigraph as (src, dst) int64 [E] in no particular order.  mode 'random': about 3 edges per destination with repeated edges, every fourth
    destination and the last one without any; 'pow2': every destination has in-degree 1, 2, 4 or 8 (or 0: every fourth and the last one), so 1 / deg and
    every product with it are exact.  hub > 0: destination 0 additionally receives `hub` edges."""
    g = torch.Generator().manual_seed(seed * 7907 + n_src * 31 + n_dst)
    if mode == "pow2":
        deg = 2 ** torch.randint(0, 4, (n_dst,), generator=g)
    else:
        deg = torch.randint(1, 6, (n_dst,), generator=g)
    deg[3::4] = 0
    if n_dst > 1:
        deg[-1] = 0
    if hub:
        deg[0] = hub
    dst = torch.repeat_interleave(torch.arange(n_dst), deg)
    src = torch.randint(0, n_src, (dst.numel(),), generator=g)
    if mode != "pow2" and dst.numel() > 1:      # a repeated edge
        src[1], dst[1] = src[0], dst[0]
    p = torch.randperm(dst.numel(), generator=g)
    return src[p], dst[p]


def csr_by(key, other, n_rows):
    """CSR of the edges grouped by `key` (stable): rowptr int32 [n_rows + 1], col int32 [E] (the `other` end), and the edge permutation."""
    o = torch.sort(key, stable=True).indices
    deg = torch.bincount(key, minlength=n_rows)
    rowptr = torch.cat([deg.new_zeros(1), deg.cumsum(0)]).to(torch.int32)
    return rowptr, other[o].to(torch.int32), o


def aggregate_case(n_src, n_rows, width, seed=1, exact=True, mean=False, scale="none", hub=0):
    """x fp32 [n_src, width], a CSR by destination, an edge scale (None | 'mean': fl32(1 / max(deg, 1)) | 'pow2': a random power of two per edge), the
    fp64 reference (PyG's: sum, then for 'mean' the division in fp64) and either the closure proof or the bound with n = deg (+ 2 with a scale)."""
    src, dst = make_graph(n_src, n_rows, seed, "pow2" if (exact and mean) else "random", hub)
    g = torch.Generator().manual_seed(seed + 17)
    x = _ints(g, (n_src, width)) if exact else torch.randn(n_src, width, generator=g, dtype=torch.float32)
    rowptr, col, o = csr_by(dst, src, n_rows)
    deg = torch.bincount(dst, minlength=n_rows)
    sc = None
    if mean:
        sc = (1.0 / deg.clamp(min=1).to(torch.float32))[dst][o].contiguous()
    elif scale == "pow2":
        sc = (2.0 ** -torch.randint(0, 4, (dst.numel(),), generator=g).double()).float()
    x64 = x.double()
    w64 = torch.ones(dst.numel(), dtype=torch.float64) if sc is None or mean else sc.double()
    rows = dst[o]
    ref = torch.zeros(n_rows, width, dtype=torch.float64).index_add(0, rows, x64[col.long()] * w64[:, None])
    sum_abs = torch.zeros(n_rows, width, dtype=torch.float64).index_add(0, rows, x64[col.long()].abs() * w64[:, None])
    if mean:
        d = deg.clamp(min=1).double()[:, None]
        ref, sum_abs = ref / d, sum_abs / d
    case = dict(n_src=n_src, n_rows=n_rows, width=width, x=x, rowptr=rowptr, col=col, scale=sc, src=src, dst=dst, deg=deg, ref=ref, exact=exact, mean=mean)
    if exact:
        grid = 0
        if sc is not None:
            assert bool((torch.frexp(sc)[0] == 0.5).all()), "an exact case needs power-of-two scales"
            grid = int(torch.log2(sc.double().min())) if sc.numel() else 0
        case["closure"] = _require_closure(sum_abs, grid, f"aggregate {n_rows} x {width}")
        assert torch.equal(ref.float().double(), ref)
        case["bound"] = None
    else:
        case["bound"] = gamma((deg + (2 if sc is not None else 0)).clamp(min=1))[:, None] * sum_abs
    return case


AGG_DAMAGES = ("drop_one_edge", "stale_element", "shift_row_group")


def damaged_aggregate(case, kind):
    bad = _damaged_aggregate(case, kind)
    return None if bad is None or torch.equal(bad, case["ref"]) else bad      # (a damage that leaves the right result is none)


def _damaged_aggregate(case, kind):
    """drop_one_edge: one destination misses one in-edge (the edge whose contribution to its widest column is of median size);  stale_element: one element
    of a row WITHOUT edges keeps the poison instead of +0.0 (no such row: of the last row);  shift_row_group: the last group of 8 rows is shifted by one."""
    ref = case["ref"]
    bad = ref.clone()
    n_rows = case["n_rows"]
    if kind == "drop_one_edge":
        rp = case["rowptr"].long()
        d = rp[1:] - rp[:-1]
        busy = d.argsort(descending=True, stable=True)[:int((d > 0).sum())]      # the destination of highest in-degree first: the hardest one to police
        if busy.numel() == 0:
            return None
        x64 = case["x"].double()
        for r in busy.tolist()[:8]:
            contrib = x64[case["col"][rp[r]:rp[r + 1]].long()]
            if case["scale"] is not None:
                contrib = contrib * case["scale"][rp[r]:rp[r + 1]].double()[:, None]
            mag = contrib.abs().amax(1)
            nz = mag.nonzero()[:, 0]
            if nz.numel():
                e = nz[mag[nz].argsort()[nz.numel() // 2]]
                bad[r] -= contrib[e]
                return bad
        return None
    if kind == "stale_element":
        empty = (case["deg"] == 0).nonzero()[:, 0]
        bad[int(empty[0]) if empty.numel() else n_rows - 1, -1] = float("nan")
        return bad
    if kind == "shift_row_group":
        r0 = (n_rows - 1) // 8 * 8
        if n_rows - r0 < 2:
            r0 = max(0, r0 - 8)
        if n_rows - r0 < 2 or torch.equal(ref[r0:].roll(-1, 0), ref[r0:]):
            return None
        bad[r0:] = ref[r0:].roll(-1, 0)
        return bad
    raise KeyError(kind)


# ---------------------------------------------------------------------------------------------------
# column sums  out[n] = sum_m X[m, n]
# ---------------------------------------------------------------------------------------------------
@lru_cache(maxsize=4)
def colsum_case(M, N, seed=1, exact=True):
    g = torch.Generator().manual_seed(seed * 31 + M * 1009 + N)
    X = _ints(g, (M, N)) if exact else torch.randn(M, N, generator=g, dtype=torch.float32)
    ref, sum_abs = X.double().sum(0), X.double().abs().sum(0)
    case = dict(M=M, N=N, X=X, ref=ref, exact=exact, bound=None)
    if exact:
        case["closure"] = _require_closure(sum_abs, 0, f"colsum {M} x {N}")
    else:
        case["bound"] = gamma(max(M, 1)) * sum_abs
    return case


COLSUM_DAMAGES = ("drop_one_row", "drop_last_block", "stale_element")


def damaged_colsum(case, kind):
    bad = _damaged_colsum(case, kind)
    return None if bad is None or torch.equal(bad, case["ref"]) else bad


def _damaged_colsum(case, kind):
    """drop_one_row: every column misses one row (of median magnitude in column 0's non-zero entries);  drop_last_block: the rows of the last 512-row block
    are missing;  stale_element: the last column keeps the poison."""
    X, M = case["X"].double(), case["M"]
    bad = case["ref"].clone()
    if kind == "stale_element":
        bad[-1] = float("nan")
        return bad
    if M == 0:
        return None
    if kind == "drop_one_row":
        nz = X[:, 0].abs().nonzero()[:, 0]
        if nz.numel() == 0:
            return None
        r = nz[X[nz, 0].abs().argsort()[nz.numel() // 2]]
        bad[0] -= X[r, 0]
        return bad
    if kind == "drop_last_block":
        r0 = (M - 1) // 512 * 512
        return bad - X[r0:].sum(0)
    raise KeyError(kind)


# ---------------------------------------------------------------------------------------------------
# closure proofs of the autograd operators (ops._Linear, ops._GraphConv): every GEMM, aggregation and column sum of forward and backward
# ---------------------------------------------------------------------------------------------------
def _lsb(t):
    """Exponent of the finest dyadic grid holding every element of t (0 for an all-zero or empty tensor: it adds no term)."""
    from tests.exact_data import lsb_exponent
    e = lsb_exponent(t) if t is not None and t.numel() else float("inf")
    return 0 if e == float("inf") else e


def prove_linear(x, W, b, g, what="linear", worst=None):
    """y = x W^T + b, dx = g W, dW = g^T x, db = column sums of g (fp64 tensors, x [rows, in], g [rows, out]): raises DoesNotClose unless every sum of
    |terms| stays below 2^24 units of its terms' grid.  `worst`: a dict that keeps the largest fraction of the limit seen, per operation."""
    x, W, g = x.detach().double(), W.detach().double(), g.detach().double()
    sums = [("forward", x.abs() @ W.abs().t() + (b.detach().double().abs() if b is not None else 0.0), min(_lsb(x) + _lsb(W), _lsb(b) if b is not None else 0)),
            ("dx", g.abs() @ W.abs(), _lsb(g) + _lsb(W)),
            ("dW", g.abs().t() @ x.abs(), _lsb(g) + _lsb(x)),
            ("db", g.abs().sum(0), _lsb(g))]
    for name, s, grid in sums:
        frac = _require_closure(s, grid, f"{what} {name}")
        if worst is not None:
            worst[name] = max(worst.get(name, 0.0), frac)


def prove_graph_conv(xs, xd, Wr, b, Wo, src, dst, mean, g, what="graph_conv", worst=None):
    """out = lin_rel(aggr x_src) + lin_root(x_dst) and its backward as ops._GraphConv evaluates them: the aggregation, y = agg W_rel^T + b accumulated with
    x_dst W_root^T (one fp32 element receives all of these terms), d agg = g W_rel, its transposed aggregation, dx_dst, dW_rel = g^T agg, db, dW_root.
    'mean' needs power-of-two in-degrees (1 / deg and every product with it exact).  Returns the fp64 aggregate."""
    xs, xd, Wr, Wo, g = (t.detach().double() for t in (xs, xd, Wr, Wo, g))
    n_src, n_dst = xs.shape[0], xd.shape[0]
    w_e = torch.ones(dst.numel(), dtype=torch.float64)
    if mean:
        deg = torch.bincount(dst, minlength=n_dst).clamp(min=1)
        if not bool((deg & (deg - 1) == 0).all()):
            raise DoesNotClose(f"{what}: 'mean' over an in-degree that is not a power of two rounds")
        w_e = (1.0 / deg.double())[dst]
    agg = torch.zeros(n_dst, xs.shape[1], dtype=torch.float64).index_add(0, dst, xs[src] * w_e[:, None])
    agg_abs = torch.zeros(n_dst, xs.shape[1], dtype=torch.float64).index_add(0, dst, xs[src].abs() * w_e[:, None])
    dagg = g.abs() @ Wr.abs()
    e_s = _lsb(w_e)
    sums = [("aggregate", agg_abs, _lsb(xs) + e_s),
            ("forward", agg.abs() @ Wr.abs().t() + (b.detach().double().abs() if b is not None else 0.0) + xd.abs() @ Wo.abs().t(),
             min(_lsb(agg) + _lsb(Wr), _lsb(b) if b is not None else 0, _lsb(xd) + _lsb(Wo))),
            ("d agg", dagg, _lsb(g) + _lsb(Wr)),
            ("dx_src", torch.zeros(n_src, xs.shape[1], dtype=torch.float64).index_add(0, src, dagg[dst] * w_e[:, None]), _lsb(g) + _lsb(Wr) + e_s),
            ("dx_dst", g.abs() @ Wo.abs(), _lsb(g) + _lsb(Wo)),
            ("dW_rel", g.abs().t() @ agg.abs(), _lsb(g) + _lsb(agg)),
            ("db", g.abs().sum(0), _lsb(g)),
            ("dW_root", g.abs().t() @ xd.abs(), _lsb(g) + _lsb(xd))]
    for name, s, grid in sums:
        frac = _require_closure(s, grid, f"{what} {name}")
        if worst is not None:
            worst[name] = max(worst.get(name, 0.0), frac)
    return agg


class _RecLinear(torch.autograd.Function):
    """x W^T + b in fp64 that proves, in its backward (when the gradient is known), the closure of the four fp32 products ops._Linear runs for it."""
    @staticmethod
    def forward(ctx, x, W, b, what, worst):
        ctx.save_for_backward(x, W, b)
        ctx.what, ctx.worst = what, worst
        return x @ W.t() + b

    @staticmethod
    def backward(ctx, g):
        x, W, b = ctx.saved_tensors
        prove_linear(x, W, b, g, ctx.what, ctx.worst.setdefault(ctx.what, {}))
        return g @ W, g.t() @ x, g.sum(0), None, None


class _RecGraphConv(torch.autograd.Function):
    """One GraphConv call in fp64 (aggregate, lin_rel, + lin_root) that proves the closure of every fp32 operation ops._GraphConv runs for it."""
    @staticmethod
    def forward(ctx, xs, xd, Wr, b, Wo, ei, mean, what, worst):
        src, dst = ei[0], ei[1]
        w = (1.0 / torch.bincount(dst, minlength=xd.shape[0]).clamp(min=1).double())[dst] if mean else torch.ones(dst.numel(), dtype=torch.float64)
        agg = torch.zeros(xd.shape[0], xs.shape[1], dtype=torch.float64).index_add(0, dst, xs[src] * w[:, None])
        ctx.save_for_backward(xs, xd, Wr, b, Wo, agg, w)
        ctx.ei, ctx.mean, ctx.what, ctx.worst = ei, mean, what, worst
        return agg @ Wr.t() + b + xd @ Wo.t()

    @staticmethod
    def backward(ctx, g):
        xs, xd, Wr, b, Wo, agg, w = ctx.saved_tensors
        src, dst = ctx.ei[0], ctx.ei[1]
        prove_graph_conv(xs, xd, Wr, b, Wo, src, dst, ctx.mean, g, ctx.what, ctx.worst.setdefault(ctx.what, {}))
        gxs = torch.zeros_like(xs).index_add(0, src, (g @ Wr)[dst] * w[:, None])
        return gxs, g @ Wo, g.t() @ agg, g.sum(0), g.t() @ xd, None, None, None, None


def operator_algebra(spec, params, x_dict, edge_index_dict, B, gout):
    """models._forward_operators restated on the host in fp64 -- the same Linear / GraphConv calls in the same grouping (per relation lin_rel(agg) +
    lin_root(x_dst), then the sum over the relations of a destination type; plain relu as the activation) -- with every call proving its own fp32 closure
    for forward and backward under the output gradient `gout` (DoesNotClose otherwise).  The model itself runs in fp64 tensors: the sums over relations,
    the residual, the activation and the +-1 masks are fp64 torch operations between the operator calls and round nothing.
    Returns (out [B * n_out * d], {parameter: gradient | None}, {call: {operation: largest sum of |terms| as a fraction of the fp32 limit}})."""
    from morphsym_hgnn_amd.spec import rel_key
    from oracle import ms_hgnn_oracle as orc
    from tests import helpers
    cfg = helpers.oracle_config(spec)
    P = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    worst = {}
    x = {}
    for t, m in spec.input_masks().items():
        v = x_dict[t]
        x[t] = (v.view(-1, m.shape[0], v.shape[1]) * m.to(v.dtype).unsqueeze(0)).reshape(v.shape)
    x = {t: torch.relu(_RecLinear.apply(v, P[f"encoder.lins.{t}.weight"], P[f"encoder.lins.{t}.bias"], f"encoder.{t}", worst)) for t, v in x.items()}
    for l in range(spec.num_layers):
        outs = {}
        for et in spec.edge_types:
            et = tuple(et)
            if et not in edge_index_dict:
                continue
            p = f"convs.{l}.convs.{rel_key(et)}."
            o = _RecGraphConv.apply(x[et[0]], x[et[2]], P[p + "lin_rel.weight"], P[p + "lin_rel.bias"], P[p + "lin_root.weight"], edge_index_dict[et],
                                    orc.relation_aggr(cfg, et) == "mean", f"layer {l} {rel_key(et)}", worst)
            outs.setdefault(et[2], []).append(o)
        h = {}
        for d, xs in outs.items():
            acc = xs[0]
            for t in xs[1:]:
                acc = acc + t
            h[d] = acc
        if spec.kind in ("mi", "s4_com") or not spec.has_base_transform:
            x = {k: torch.relu(v) for k, v in h.items()}
            continue
        new = {}
        for k, v in h.items():
            if k == "base":
                t1 = torch.relu(_RecLinear.apply(v, P["base_transform.0.weight"], P["base_transform.0.bias"], f"base_transform.0 (layer {l})", worst))
                new[k] = _RecLinear.apply(t1, P["base_transform.2.weight"], P["base_transform.2.bias"], f"base_transform.2 (layer {l})", worst)
            else:
                new[k] = torch.relu(v)
        x = {k: new[k] + x[k] if (k in x and x[k].shape == new[k].shape) else new[k] for k in new}
    out = _RecLinear.apply(x[spec.out_type], P["decoder.weight"], P["decoder.bias"], "decoder", worst)
    n_out = spec.num_nodes[spec.out_type]
    out = (out.view(B, n_out, -1) * spec.output_mask().to(out.dtype).unsqueeze(0)).reshape(-1)
    out.backward(gout.reshape(-1))
    return out.detach(), {k: v.grad for k, v in P.items()}, worst


# ---------------------------------------------------------------------------------------------------
# the GPU tables (tests/test_ops_exact_gpu.py runs them, tests/test_ops_reference.py polices them)
# ---------------------------------------------------------------------------------------------------
GEMM_EDGE_MN = [1, 31, 32, 33, 63, 64, 65, 129]
GEMM_EDGE_K = [0, 1, 15, 16, 17, 33, 900]
# split-K: (M, N) -> {K: the number of splits the case is NAMED for}; from the rule tiles < 512 && K >= 2048 -> min(ceil(1024 / tiles), K / 512, 256)
# worked by hand: 1 and 1 tiles (1024 / 1), 2 x 8 = 16 tiles (64), 3 x 2 = 6 tiles (171).  K = 70000 at 136 splits: chunks of 528, chunks 133..135 empty.
GEMM_SPLITK = {
    (1, 1): {2047: 1, 2048: 4, 2049: 4, 3000: 5, 70000: 136, 131073: 256},
    (64, 64): {2047: 1, 2048: 4, 2049: 4, 3000: 5, 70000: 136, 131073: 256},
    (128, 450): {2047: 1, 2048: 4, 2049: 4, 3000: 5, 70000: 64, 131073: 64},
    (129, 65): {2047: 1, 2048: 4, 2049: 4, 3000: 5, 70000: 136, 131073: 171},
}
GEMM_LAYOUTS = ["row", "col", "pad", "view"]
GEMM_STRIDE_SHAPES = [(65, 33, 50, 1), (65, 33, 2500, 4)]                       # (M, N, K, splits): a ragged shape, a split-K shape
GEMM_UNIT_SHAPES = [(1, 33, 50, 1), (65, 1, 50, 1), (65, 33, 1, 1), (1, 1, 1, 1), (1, 33, 2500, 4), (65, 1, 2500, 4)]      # M == 1, N == 1, K == 1
# random fp32 data, K <= 2048: test_linear_matches_reference's forward shapes, the ragged ones, one split-K point
GEMM_RANDOM = [(1, 5, 7, 1), (50, 128, 450, 1), (3000, 128, 900, 1), (257, 3, 128, 1), (70000, 128, 128, 1), (65, 33, 50, 1), (129, 65, 33, 1),
               (63, 31, 17, 1), (65, 33, 2048, 4)]


def gemm_variants():
    return [(b, a) for b in (False, True) for a in (False, True)]


def all_gemm_cases():
    """(M, N, K, exact, splits) of every GEMM the GPU file runs, without repetition; each is run (and policed) with and without bias / accumulate."""
    seen = []
    for K in GEMM_EDGE_K:
        for M in GEMM_EDGE_MN:
            for N in GEMM_EDGE_MN:
                seen.append((M, N, K, True, 1))
    for (M, N), ks in GEMM_SPLITK.items():
        for K, s in ks.items():
            seen.append((M, N, K, True, s))
    for M, N, K, s in GEMM_STRIDE_SHAPES + GEMM_UNIT_SHAPES:
        seen.append((M, N, K, True, s))
    for M, N, K, s in GEMM_RANDOM:
        seen.append((M, N, K, False, s))
    return list(dict.fromkeys(seen))


AGG_ROWS = [1, 7, 8, 9, 1000]
AGG_WIDTHS = [1, 31, 32, 33, 450, 900]
AGG_HUB = 100000          # one destination with this many in-edges ('add': exact; 'mean': random data under the bound)
AGG_HUB_POW2 = 131072     # ... and with a power-of-two in-degree ('mean': exact)
AGG_KINDS = [      # (name, exact, mean, scale)
    ("add_exact", True, False, "none"), ("scaled_exact", True, False, "pow2"), ("mean_exact", True, True, "none"),
    ("add_random", False, False, "none"), ("mean_random", False, True, "none"),
]


def all_aggregate_cases():
    """Keyword arguments of aggregate_case for every aggregation the GPU file runs through the C-ABI."""
    out = []
    for name, exact, mean, scale in AGG_KINDS:
        for r in AGG_ROWS:
            for w in AGG_WIDTHS:
                out.append(dict(n_src=max(3, r // 2 + 5), n_rows=r, width=w, exact=exact, mean=mean, scale=scale))
    out.append(dict(n_src=50, n_rows=9, width=33, exact=True, mean=False, scale="none", hub=AGG_HUB))
    out.append(dict(n_src=50, n_rows=9, width=33, exact=True, mean=True, scale="none", hub=AGG_HUB_POW2))
    # (no random-data hub: gamma_100002 = 6e-3 of the row's sum of |terms| hides one edge of 1e5 -- the host controls refuse such a case, the exact ones carry it)
    return out


COLSUM_M = [0, 1, 511, 512, 513, 70000]
COLSUM_N = [1, 255, 256, 257, 900]


COLSUM_RANDOM_MAX_M = 513      # random data: gamma_70000 = 4e-3 of a column's sum of |x| hides a whole dropped row (the host controls refuse it); 70000 rows are exact only


def all_colsum_cases():
    return [(M, N, exact) for exact in (True, False) for M in COLSUM_M for N in COLSUM_N if exact or M <= COLSUM_RANDOM_MAX_M]
