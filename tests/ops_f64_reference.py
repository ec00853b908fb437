"""Host-side references, data and checkers for the fp64 stand-alone operators (csrc/mshgnn_ops.hip behind ops.compute_dtype("f64")): test
infrastructure, no GPU.  The discipline is tests/ops_reference.py's with u = 2^-53; its shape tables are reused by import.

Three data families for the GEMM, each stored as int64 tensors on a dyadic grid (value = int * 2^exp, exact in fp64):
  * wide_sum: integer operands of magnitude in [R / 2, R], odd, R = floor(sqrt(2^52 / K)) capped at 2^20 (bias and a pre-existing C: odd integers up to
    2^20).  Every partial sum of every summation order is an integer below 2^53 (proved per case: `_require_closure`) and the results lie far above 2^24,
    so the expected value is the exact integer product -- evaluated with fp64 matmul, which cannot round on such data; tests/test_ops_f64_reference.py
    checks it against int64 matmul -- and ANY fp32 accumulation is wrong.  The operands themselves are fp32 values (<= 2^20): this family cannot see
    operands narrowed to fp32; the next one does.
  * wide_operand: A holds odd integers in [2^25, 2^26) (26 significant bits), B one such entry per output column and zeros elsewhere: every sum has ONE
    term, a 52-bit product, exact.  Any narrowing of an operand to fp32 is wrong.  It cannot see a dropped k where B is zero; wide_sum does.
  * random: dyadic values int * 2^-20, |int| < 2^25.  The reference is exact in int64 arithmetic (units of 2^-40; K < 8192 so that it fits) and the checker
    evaluates got - exact without ever rounding the reference (`dyadic_error`: the reference as two limbs).  Bound, per element:
        gamma_{2K+4}(u) (sum_k |a||b| + |bias| + |C_in|),   gamma_n = n u / (1 - n u),   u = 2^-53.
    No term passes through more than K + splits + 3 roundings when the MFMA fuses product and add, 2K + splits + 3 when it rounds them separately, and no
    split-K case here has more than K splits: 2K + 4 covers both without knowing how v_mfma_f64_16x16x4_f64 rounds internally.
A GPU case is one (shape, bias, accumulate) run on EVERY family the table gives it; its checker is the conjunction.  `damaged_gemm64` builds the wrong
results a broken kernel would give (operands rounded to fp32, accumulation in fp32, one dropped k, a dropped last K tile, a dropped split-K partial, bias
added twice, a stale element, a shifted row tile); tests/test_ops_f64_reference.py demands, for every case of the GPU matrix, that each of them is a
different result on at least one exact family (there the checker is bit equality) and lies outside the bound on the random family where that runs.

Aggregation (`aggregate_case64`) and column sums (`colsum_case64`) follow the same pattern; their data are described at the builders.
"""
from functools import lru_cache
from math import isqrt

import torch

from tests import ops_reference as opr
from tests.ops_reference import (AGG_HUB, AGG_HUB_POW2, AGG_ROWS, AGG_WIDTHS, COLSUM_M, COLSUM_N, GEMM_EDGE_K, GEMM_EDGE_MN, GEMM_LAYOUTS,  # noqa: F401
                                 GEMM_SPLITK, GEMM_STRIDE_SHAPES, GEMM_UNIT_SHAPES, DoesNotClose)

U = 2.0 ** -53
LIMIT = 2.0 ** 53
FAMILIES = ("wide_sum", "wide_operand", "random")
RANDOM_EXP = -20            # the grid of the random family
RANDOM_MAX_K = 8191         # 2^13 products of two 25-bit integers stay below 2^63


def gamma(n):
    n = torch.as_tensor(n, dtype=torch.float64)
    assert bool((n * U < 1).all()), "n u >= 1: no bound"
    return n * U / (1 - n * U)


def _require_closure(sum_abs, grid_exp, what):
    """sum_abs: fp64 tensor of sums of |terms|; every one must be < 2^53 units of 2^grid_exp (then no partial sum of any order rounds in fp64)."""
    worst = float(sum_abs.max()) if sum_abs.numel() else 0.0
    if not worst < LIMIT * 2.0 ** grid_exp:
        raise DoesNotClose(f"{what}: a sum of |terms| {worst} reaches 2^53 units of 2^{grid_exp}")
    return worst / (LIMIT * 2.0 ** grid_exp)


def _odd(g, shape, R):
    """Odd int64 of magnitude in [R / 2, R] (R >= 4), random sign: never zero, never a multiple of a large power of two."""
    lo = max(1, R // 2)
    v = torch.randint(lo, R, shape, generator=g, dtype=torch.int64) | 1
    s = torch.randint(0, 2, shape, generator=g, dtype=torch.int64) * 2 - 1
    return v * s


def wide_sum_range(K):
    return min(2 ** 20, isqrt(2 ** 52 // max(K, 1)))


@lru_cache(maxsize=4)
def _gemm_base(M, N, K, seed, family):
    g = torch.Generator().manual_seed(seed * 1000003 + M * 7919 + N * 104729 + K + 17 * FAMILIES.index(family))
    if family == "wide_sum":
        R = wide_sum_range(K)
        A, B, bias, C, e = _odd(g, (M, K), R), _odd(g, (N, K), R), _odd(g, (N,), 2 ** 20), _odd(g, (M, N), 2 ** 20), 0
    elif family == "wide_operand":
        A = _odd(g, (M, K), 2 ** 26)
        B = torch.zeros(N, K, dtype=torch.int64)
        if K:
            B[torch.arange(N), torch.randint(0, K, (N,), generator=g)] = _odd(g, (N,), 2 ** 26)
        bias, C, e = _odd(g, (N,), 2 ** 20), _odd(g, (M, N), 2 ** 20), 0
    else:
        assert K <= RANDOM_MAX_K
        draw = lambda shape: torch.randint(-(2 ** 25) + 1, 2 ** 25, shape, generator=g, dtype=torch.int64)
        A, B, e = draw((M, K)), draw((N, K)), RANDOM_EXP
        bias, C = draw((N,)) * 2 ** 20, draw((M, N)) * 2 ** 20          # in the units of the products, 2^-40
    return A, B, bias, C, e


@lru_cache(maxsize=3)
def _gemm_products(M, N, K, seed, family):
    """(A, B, A B^T, |A| |B|^T) in fp64 for an exact family, computed once for the four (bias, accumulate) variants of a shape."""
    Ai, Bi, _, _, e = _gemm_base(M, N, K, seed, family)
    A, B = Ai.double(), Bi.double()
    return A, B, A @ B.t(), A.abs() @ B.abs().t()


def gemm_case(M, N, K, family, seed=1, bias=False, accumulate=False, splits=1):
    """Operands as fp64 tensors (A [M, K], B [N, K], bias [N] | None, C_in [M, N] | None; exact images of the int64 draws), the fp64 reference `ref`
    (exact families: THE result; random: the exact result rounded once, for building damaged results only), `sum_abs`, and for the random family the exact
    reference as two limbs (`ref_hi`, `ref_lo`: exact = ref_hi 2^-20 + ref_lo 2^-40) and the per-element `bound`."""
    Ai, Bi, bi, Ci, e = _gemm_base(M, N, K, seed, family)
    s1, s2 = 2.0 ** e, 2.0 ** (2 * e)
    A, B = Ai.double() * s1, Bi.double() * s1
    b, C = (bi.double() * s2 if bias else None), (Ci.double() * s2 if accumulate else None)
    case = dict(M=M, N=N, K=K, A=A, B=B, bias=b, C_in=C, family=family, exact=family != "random", splits=splits)
    if family != "random":
        A, B, ref, sum_abs = _gemm_products(M, N, K, seed, family)
        case.update(A=A, B=B)
        ref, sum_abs = ref.clone(), sum_abs.clone()
        if bias:
            ref, sum_abs = ref + b, sum_abs + b.abs()
        if accumulate:
            ref, sum_abs = ref + C, sum_abs + C.abs()
        case["closure"] = _require_closure(sum_abs, 0, f"gemm {family} {M} x {N} x {K}")
        case.update(ref=ref, sum_abs=sum_abs, bound=None)
        return case
    ref_i, abs_i = Ai @ Bi.t(), Ai.abs() @ Bi.abs().t()               # int64: exact
    if bias:
        ref_i, abs_i = ref_i + bi, abs_i + bi.abs()
    if accumulate:
        ref_i, abs_i = ref_i + Ci, abs_i + Ci.abs()
    hi = ref_i >> 20                                                    # floor: lo in [0, 2^20)
    lo = ref_i - (hi << 20)
    sum_abs = abs_i.double() * s2 * (1 + 2 * U)                         # (the int64 -> fp64 conversion may round down by one part in 2^53)
    case.update(ref=hi.double() * 2.0 ** -20 + lo.double() * s2, ref_hi=hi.double(), ref_lo=lo.double(), sum_abs=sum_abs, bound=gamma(2 * K + 4) * sum_abs)
    return case


def dyadic_error(got, ref_hi, ref_lo):
    """got - (ref_hi 2^-20 + ref_lo 2^-40) for fp64 `got`, |ref_hi| < 2^53 and 0 <= ref_lo < 2^20: got 2^20 is exact, the first difference is exact whenever
    got is within a factor two of the reference (Sterbenz) and otherwise large, the second rounds once -- a relative error of 2^-53 on the error itself."""
    got = got.detach().double().cpu().reshape(ref_hi.shape)
    return ((got * 2.0 ** 20 - ref_hi) - ref_lo * 2.0 ** -20) * 2.0 ** -20


def gemm_failure(case, got, where=None):
    """None when `got` passes the case's checker: bit equality on the exact families, the bound around the unrounded reference on the random one."""
    if case["exact"]:
        return opr.first_mismatch(got, case["ref"], where)
    got = got.detach().double().cpu().reshape(case["ref"].shape)
    bad = ~(dyadic_error(got, case["ref_hi"], case["ref_lo"]).abs() <= case["bound"])
    return opr._describe(bad, got, case["ref"], where, case["bound"])


def kchunk(K, splits):
    return max(16, (-(-max(K, 1) // splits) + 15) // 16 * 16)


GEMM_DAMAGES = opr.GEMM_DAMAGES + ("operands_f32", "accumulate_f32", "drop_split_partial")


def damaged_gemm64(case, kind):
    """A deliberately wrong fp64 result for `case`, or None where the damage does not exist or gives the right result on this data:
      the five of ops_reference.damaged_gemm (one dropped k, a dropped last K tile, a shifted row tile, bias twice, a stale element);
      operands_f32: A and B rounded to fp32 before an otherwise exact product;
      accumulate_f32: the mildest form of an fp32 accumulator -- the exact result rounded to fp32 once;
      drop_split_partial: the products of the middle non-empty K chunk of a split-K launch are missing."""
    if kind in opr.GEMM_DAMAGES:
        return opr.damaged_gemm(case, kind)
    ref, A, B = case["ref"], case["A"], case["B"]
    if kind == "operands_f32":
        if case["K"] == 0:
            return None
        bad = ref - A @ B.t() + A.float().double() @ B.float().double().t()
    elif kind == "accumulate_f32":
        bad = ref.float().double()
    elif kind == "drop_split_partial":
        if case["splits"] < 2:
            return None
        kc = kchunk(case["K"], case["splits"])
        z = (-(-case["K"] // kc)) // 2
        bad = ref - A[:, z * kc:(z + 1) * kc] @ B[:, z * kc:(z + 1) * kc].t()
    else:
        raise KeyError(kind)
    return None if torch.equal(bad, ref) else bad


# the GPU matrix ------------------------------------------------------------------------------------------------------------------------------------
GEMM_WGRAD = (70000, 128, 128, 1)          # the weight-gradient shape of a 70000-row batch as a plain product (exact families only)
# random data: the forward shapes of a Linear at small batch, the ragged ones, one split-K point (K <= RANDOM_MAX_K)
GEMM_RANDOM = [(1, 5, 7, 1), (50, 128, 450, 1), (257, 3, 128, 1), (65, 33, 50, 1), (129, 65, 33, 1), (63, 31, 17, 1), (65, 33, 2048, 4), (65, 33, 2500, 4)]


def families_of(M, N, K):
    """The families a shape runs on: both exact ones always, the random one where the table lists the shape."""
    return ("wide_sum", "wide_operand") + (("random",) if any((M, N, K) == c[:3] for c in GEMM_RANDOM) else ())


def all_gemm_shapes():
    """(M, N, K, splits) of every GEMM the GPU file runs, without repetition; each runs with and without bias / accumulate on `families_of` it."""
    seen = [(M, N, K, 1) for K in GEMM_EDGE_K for M in GEMM_EDGE_MN for N in GEMM_EDGE_MN]
    seen += [(M, N, K, s) for (M, N), ks in GEMM_SPLITK.items() for K, s in ks.items()]
    seen += list(GEMM_STRIDE_SHAPES) + list(GEMM_UNIT_SHAPES) + [GEMM_WGRAD] + list(GEMM_RANDOM)
    return list(dict.fromkeys(seen))


# ---------------------------------------------------------------------------------------------------
# aggregation  out[r, :] = sum_{e in row r} scale[e] x[col[e], :]
# ---------------------------------------------------------------------------------------------------
AGG_KINDS = [      # (name, exact, mean, scale)
    ("add_exact", True, False, "none"), ("scaled_exact", True, False, "wide"), ("mean_exact", True, True, "none"),
    ("add_random", False, False, "none"), ("mean_random", False, True, "none"),
]
WIDE_SCALE = (2.0 ** 30 + 1) * 2.0 ** -30      # 31 significant bits: not an fp32 value; times a 14-bit integer it is exact in fp64


def aggregate_case64(n_src, n_rows, width, seed=1, exact=True, mean=False, scale="none", hub=0):
    """The graphs of ops_reference (make_graph: repeated edges, destinations without edges, an optional hub) with fp64 data:
      add_exact / mean_exact: odd integers of magnitude up to R = min(2^44, 2^52 / largest in-degree) ('mean': power-of-two in-degrees, scale 2^-j):
        exact in fp64 in any order, wrong under any fp32 accumulation;
      scaled_exact: x odd integers below 2^14, edge scales (2^30 + 1) 2^-(30 + j), j in 0..3 -- the products are exact 45-bit values, the sums close,
        and the scale is no fp32 value: an edge scale narrowed to fp32 is wrong;
      add_random: dyadic x = int 2^-20, |int| < 2^25 -- sums of such values never round in fp64 either, so this checks bit equality too;
      mean_random: the same x over in-degrees 1..5, scale fl64(1 / deg).  Reference: the exact sum (an fp64 value) divided once by deg in fp64, within u of
        the true mean; bound gamma_{deg+3} sum |x| / deg (1 / deg, the product and the add of each edge, one more for the reference's own rounding)."""
    src, dst = opr.make_graph(n_src, n_rows, seed, "pow2" if (exact and mean) else "random", hub)
    g = torch.Generator().manual_seed(seed + 29)
    deg = torch.bincount(dst, minlength=n_rows)
    rowptr, col, o = opr.csr_by(dst, src, n_rows)
    maxdeg = max(1, int(deg.max()) if deg.numel() else 1)
    if not exact:
        x = torch.randint(-(2 ** 25) + 1, 2 ** 25, (n_src, width), generator=g, dtype=torch.int64).double() * 2.0 ** RANDOM_EXP
        grid = RANDOM_EXP
    elif scale == "wide":
        x, grid = _odd(g, (n_src, width), 2 ** 14).double(), -33
    else:
        x, grid = _odd(g, (n_src, width), min(2 ** 44, 2 ** 52 // maxdeg)).double(), 0
    sc = None
    if mean:
        sc = (1.0 / deg.clamp(min=1).double())[dst][o].contiguous()
        if exact:
            grid -= int(torch.log2(deg.clamp(min=1).double().max()))
    elif scale == "wide":
        sc = WIDE_SCALE * 2.0 ** -torch.randint(0, 4, (dst.numel(),), generator=g).double()
    rows = dst[o]
    w = sc[:, None] if sc is not None and not (mean and not exact) else 1.0
    ref = torch.zeros(n_rows, width, dtype=torch.float64).index_add(0, rows, x[col.long()] * w)
    sum_abs = torch.zeros(n_rows, width, dtype=torch.float64).index_add(0, rows, x[col.long()].abs() * w)
    case = dict(n_src=n_src, n_rows=n_rows, width=width, x=x, rowptr=rowptr, col=col, scale=sc, src=src, dst=dst, deg=deg, exact=exact, mean=mean, bound=None)
    case["closure"] = _require_closure(sum_abs, grid, f"aggregate {n_rows} x {width}")      # (mean_random: the plain sums, which the reference divides)
    if mean and not exact:
        d = deg.clamp(min=1).double()[:, None]
        ref, sum_abs = ref / d, sum_abs / d
        case["bound"] = gamma((deg + 3).clamp(min=1))[:, None] * sum_abs
    case["ref"] = ref
    return case


AGG_DAMAGES = opr.AGG_DAMAGES + ("scale_f32", "accumulate_f32")


def damaged_aggregate64(case, kind):
    if kind in opr.AGG_DAMAGES:
        return opr.damaged_aggregate(case, kind)
    ref = case["ref"]
    if kind == "accumulate_f32":
        bad = ref.float().double()
    elif kind == "scale_f32":
        if case["scale"] is None or case["scale"].numel() == 0:
            return None
        rows = torch.repeat_interleave(torch.arange(case["n_rows"]), (case["rowptr"][1:] - case["rowptr"][:-1]).long())
        bad = torch.zeros_like(ref).index_add(0, rows, case["x"][case["col"].long()] * case["scale"].float().double()[:, None])
        if torch.equal(case["scale"].float().double(), case["scale"]):
            return None
    else:
        raise KeyError(kind)
    return None if torch.equal(bad, ref) else bad


def all_aggregate_cases():
    out = []
    for name, exact, mean, scale in AGG_KINDS:
        for r in AGG_ROWS:
            for w in AGG_WIDTHS:
                out.append(dict(n_src=max(3, r // 2 + 5), n_rows=r, width=w, exact=exact, mean=mean, scale=scale))
    out.append(dict(n_src=50, n_rows=9, width=33, exact=True, mean=False, scale="none", hub=AGG_HUB))
    out.append(dict(n_src=50, n_rows=9, width=33, exact=True, mean=True, scale="none", hub=AGG_HUB_POW2))
    return out


# ---------------------------------------------------------------------------------------------------
# column sums  out[n] = sum_m X[m, n]
# ---------------------------------------------------------------------------------------------------
@lru_cache(maxsize=4)
def colsum_case64(M, N, seed=1, wide=True):
    """wide: odd integers up to min(2^44, 2^52 / M) -- exact in any order, wrong under fp32 accumulation; else dyadic int 2^-20, |int| < 2^25, whose sums
    never round in fp64 either: both are checked for bit equality."""
    g = torch.Generator().manual_seed(seed * 31 + M * 1009 + N + 5)
    if wide:
        X, grid = _odd(g, (M, N), min(2 ** 44, 2 ** 52 // max(M, 1))).double(), 0
    else:
        X, grid = torch.randint(-(2 ** 25) + 1, 2 ** 25, (M, N), generator=g, dtype=torch.int64).double() * 2.0 ** RANDOM_EXP, RANDOM_EXP
    ref, sum_abs = X.sum(0), X.abs().sum(0)
    case = dict(M=M, N=N, X=X, ref=ref, exact=True, bound=None)
    case["closure"] = _require_closure(sum_abs, grid, f"colsum {M} x {N}")
    return case


COLSUM_DAMAGES = opr.COLSUM_DAMAGES + ("accumulate_f32",)


def damaged_colsum64(case, kind):
    if kind in opr.COLSUM_DAMAGES:
        return opr.damaged_colsum(case, kind)
    if kind == "accumulate_f32":
        bad = case["ref"].float().double()
        return None if torch.equal(bad, case["ref"]) else bad
    raise KeyError(kind)


def all_colsum_cases():
    return [(M, N, wide) for wide in (True, False) for M in COLSUM_M for N in COLSUM_N]


# ---------------------------------------------------------------------------------------------------
# closure proofs of the autograd operators under the "f64" compute dtype (the fp32 proofs of ops_reference with the fp64 limit)
# ---------------------------------------------------------------------------------------------------
def prove_linear64(x, W, b, g, what="linear"):
    """y = x W^T + b, dx = g W, dW = g^T x, db = column sums of g: every sum of |terms| below 2^53 units of its grid, and the forward result beyond what
    an fp32 accumulator holds (some element of y is no fp32 value)."""
    x, W, g = x.detach().double(), W.detach().double(), g.detach().double()
    sums = [("forward", x.abs() @ W.abs().t() + (b.detach().double().abs() if b is not None else 0.0), min(opr._lsb(x) + opr._lsb(W), opr._lsb(b) if b is not None else 0)),
            ("dx", g.abs() @ W.abs(), opr._lsb(g) + opr._lsb(W)),
            ("dW", g.abs().t() @ x.abs(), opr._lsb(g) + opr._lsb(x)),
            ("db", g.abs().sum(0), opr._lsb(g))]
    for name, s, grid in sums:
        _require_closure(s, grid, f"{what} {name}")


def prove_graph_conv64(xs, xd, Wr, b, Wo, src, dst, mean, g, what="graph_conv"):
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
    e_s = opr._lsb(w_e)
    lsb = opr._lsb
    sums = [("aggregate", agg_abs, lsb(xs) + e_s),
            ("forward", agg.abs() @ Wr.abs().t() + (b.detach().double().abs() if b is not None else 0.0) + xd.abs() @ Wo.abs().t(),
             min(lsb(agg) + lsb(Wr), lsb(b) if b is not None else 0, lsb(xd) + lsb(Wo))),
            ("d agg", dagg, lsb(g) + lsb(Wr)),
            ("dx_src", torch.zeros(n_src, xs.shape[1], dtype=torch.float64).index_add(0, src, dagg[dst] * w_e[:, None]), lsb(g) + lsb(Wr) + e_s),
            ("dx_dst", g.abs() @ Wo.abs(), lsb(g) + lsb(Wo)),
            ("dW_rel", g.abs().t() @ agg.abs(), lsb(g) + lsb(agg)),
            ("db", g.abs().sum(0), lsb(g)),
            ("dW_root", g.abs().t() @ xd.abs(), lsb(g) + lsb(xd))]
    for name, s, grid in sums:
        _require_closure(s, grid, f"{what} {name}")
    return agg


def wide_ints(g, shape, bits):
    """Odd integers of magnitude in [2^(bits-1), 2^bits) as fp64: the data of the autograd tests."""
    return _odd(g, shape, 2 ** bits).double()
