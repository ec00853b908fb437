"""The stand-alone operators (csrc/mshgnn_ops.hip: k_op_gemm, k_op_splitk_sum, k_op_aggregate, k_op_colsum1/2 behind mshgnn_op_gemm / _aggregate /
_colsum; ops.py: gemm, colsum, _Linear, Csr, _GraphConv; nn.py) ELEMENT BY ELEMENT: on integer / dyadic data every fp32 FMA chain, split-K partial sum and
column sum is exact in any order, so the result must be the fp64 reference's bits (`ops_reference.first_mismatch`, no tolerance; the host proves closure
first and refuses a case that does not close); on random fp32 data every element must lie within the derived bound gamma_n sum |terms| of the fp64 value
of the same fp32 operands (`ops_reference.within_bound`, n the roundings of that element's own path).  tests/test_ops_reference.py shows on the host that
these checkers accept torch's fp32 CPU results and reject a dropped K element, a dropped K tile, a shifted row tile, a doubled bias, a dropped edge and a
stale element for every case run here.  Every output buffer is larger than the result and NaN-filled: rows >= M and columns in [N, ldc) must still be NaN,
everything inside finite.  A failure prints the first (row, column, got, want) and the tile / wave / K chunk they sit in.

What tests/test_ops_gpu.py (max |got - ref| / max |ref| < 1e-4 over a whole tensor) left unreached, and what reaches it now:
  * a wrong small element, a dropped term among 900                      -> every assertion here is per element
  * split-K with bias (forward K >= 2048), split-K with accumulate (k_op_splitk_sum's accumulate branch), ldc > N, empty trailing K chunks (K = 70000 at
    136 splits: chunks 133..135), the 256-split cap                      -> test_gemm_split_k_is_exact (the split count is asserted per case)
  * K == 0, K tiles that end ragged, M / N on both sides of 32 and 64    -> test_gemm_edges_are_exact
  * strided views (sAm != 1 && sAk != 1), padded pitches, column-major operands in all 16 pairs, M == 1 / N == 1 / K == 1 (the a_kc / b_kc staging
    choice when both strides are 1)                                      -> test_gemm_every_stride_pair_is_exact, test_gemm_unit_dimensions_are_exact
  * the error returns (ldc < N, no workspace, negative sizes, null operands, > 65535 row tiles), M == 0 / N == 0 -> test_gemm_error_returns_launch_nothing
  * aggregate / colsum with ldx != width, ldo != width, widths off 32, row counts off 8 / around OC_RB = 512, a destination of 100000 in-edges, rows
    without edges written as +0.0                                         -> test_aggregate_*, test_colsum_*
  * Csr from int32 / int64 / non-contiguous edge_index, its by-source view, out-of-range indices, an edge_index edited in place -> test_csr_*
  * autograd: every gradient of Linear / GraphConv / HeteroConv bit for bit, split-K weight gradients (3000 and 70000 rows), zero rows, E == 0, every
    subset of requires_grad                                                -> test_linear_autograd_*, test_graph_conv_*, test_hetero_conv_*
  * the operator-by-operator model path (models._forward_operators) against the oracle bit for bit -> test_operator_model_path_is_the_oracle_bit_for_bit
Found by these tests and fixed with them: mshgnn_op_gemm refused K == 0 with null A / B (what an empty tensor's data_ptr() is), so the backward of a Linear
over zero rows raised instead of giving dW = 0.

Matrix: GEMM M, N in {1, 31, 32, 33, 63, 64, 65, 129} x K in {0, 1, 15, 16, 17, 33, 900}; split-K K in {2047, 2048, 2049, 3000, 70000, 131073} at
1 x 1, 64 x 64, 128 x 450, 129 x 65, each x bias x accumulate x (ldc == N, ldc > N); 16 stride pairs at 65 x 33 x 50 and 65 x 33 x 2500; random data at
K <= 2048.  Aggregate rows {1, 7, 8, 9, 1000} x widths {1, 31, 32, 33, 450, 900} x (add, power-of-two edge scales, mean over power-of-two degrees: exact;
add and mean on random data).  Column sums M in {0, 1, 511, 512, 513, 70000} x N in {1, 255, 256, 257, 900}.
Not covered, and why:
  * `edge_weight`: GraphConv refuses it (NotImplementedError; the models never pass one).
  * GEMMs past 65535 row tiles: refused by mshgnn_op_gemm (the refusal is tested).
  * bf16 operands: the operators have none (tensors of another dtype are cast to fp32 and back; that cast is tested).
  * random data on reductions longer than 2048 (GEMM), 513 rows (column sums) or a 100000-edge destination: the bound cannot see one dropped term there
    (tests/test_ops_reference.py demonstrates it), so those shapes run on exact data only.
"""
import ctypes as C
import itertools

import pytest
import torch

from morphsym_hgnn_amd import engine as eng
from morphsym_hgnn_amd import ops
from tests import ops_reference as opr
from tests.test_ops_gpu import _ref_nn

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _require_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (there is no CPU fallback to fall through to)")


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _place(mat, layout):
    """A logical fp32 [R, K] host matrix in device memory as `layout`; returns (buffer, stride of the row index, stride of k).  Everything the layout
    leaves between the elements is NaN: a kernel that reads outside (r < R, k < K) poisons its result."""
    R, K = mat.shape
    if layout == "row":
        return mat.contiguous().to(DEV), K, 1
    if layout == "col":
        return mat.t().contiguous().to(DEV), 1, R
    if layout == "pad":
        buf = _nan(R, K + 5)
        buf[:, :K] = mat.to(DEV)
        return buf, K + 5, 1
    if layout == "view":      # every other column of a wider matrix: both strides != 1
        buf = _nan(R, 2 * K + 1)
        buf[:, 0:2 * K:2] = mat.to(DEV)
        return buf, 2 * K + 1, 2
    raise KeyError(layout)


def _splits(M, N, K):
    s = C.c_int32(-1)
    need = eng.load_library().mshgnn_op_gemm_workspace(M, N, K, C.byref(s))
    assert (need > 0) == (s.value > 1) and (need == 0 or need == s.value * M * N * 4)
    return s.value


def _check_frame(wide, r0, r1, c0, c1, what):
    """Outside [r0, r1) x [c0, c1) the NaN fill is untouched; inside everything is finite."""
    host = wide.cpu()
    outside = torch.ones_like(host, dtype=torch.bool)
    outside[r0:r1, c0:c1] = False
    assert bool(torch.isnan(host[outside]).all()), f"{what}: wrote outside its {r1 - r0} x {c1 - c0} result"
    inside = host[r0:r1, c0:c1]
    assert bool(torch.isfinite(inside).all()), f"{what}: {int((~torch.isfinite(inside)).sum())} elements of the result were not written (or are not finite)"
    return inside


def _gemm(case, placed=None, la="row", lb="row", wide_ldc=False, what=""):
    """ops.gemm on `case` (ops_reference.gemm_operands) into a NaN frame; returns the failure description or None."""
    M, N, K = case["M"], case["N"], case["K"]
    (A, sAm, sAk), (B, sBn, sBk) = placed if placed is not None else (_place(case["A"], la), _place(case["B"], lb))
    bias = case["bias"].to(DEV) if case["bias"] is not None else None
    off = 1 if wide_ldc else 0
    wide = _nan(M + 2, N + (4 if wide_ldc else 0))
    out = wide[:M, off:off + N]
    if case["C_in"] is not None:
        out.copy_(case["C_in"])
    assert _splits(M, N, K) == case["splits"], f"{what}: takes {_splits(M, N, K)} K split(s), the case is named for {case['splits']}"
    r = ops.gemm(A, sAm, sAk, B, sBn, sBk, M, N, K, bias=bias, out=out, accumulate=case["C_in"] is not None)
    torch.cuda.synchronize()
    assert r.data_ptr() == out.data_ptr()
    inside = _check_frame(wide, 0, M, off, off + N, what)
    where = opr.gemm_where(K, case["splits"])
    d = opr.first_mismatch(inside, case["ref"], where) if case["exact"] else opr.within_bound(inside, case["ref"], case["bound"], where)
    return None if d is None else f"{what}: {d}"


# ---------------------------------------------------------------------------------------------------
# 2. mshgnn_op_gemm
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", opr.GEMM_EDGE_K)
def test_gemm_edges_are_exact(K):
    """Every M, N on both sides of the 32-row wave tile and the 64-row workgroup tile at K around the 16-wide K tile (K == 0: bias / C_in alone), with and
    without bias and accumulate, into ldc == N and ldc > N; row-major operands (K == 0: also null ones, what an empty tensor hands over, and padded ones)."""
    _require_gpu()
    bad = []
    for M, N in itertools.product(opr.GEMM_EDGE_MN, opr.GEMM_EDGE_MN):
        for i, (bias, acc) in enumerate(opr.gemm_variants()):
            case = opr.gemm_operands(M, N, K, exact=True, bias=bias, accumulate=acc)
            for lay in (("row", "row"), ("pad", "pad")) if K == 0 else (("row", "row"),):
                d = _gemm(case, la=lay[0], lb=lay[1], wide_ldc=bool((i + M + N) & 1), what=f"{M} x {N} x {K} bias={bias} accumulate={acc} {lay}")
                if d:
                    bad.append(d)
    assert not bad, "\n".join(bad[:10])


@pytest.mark.parametrize("K", sorted(opr.GEMM_SPLITK[(1, 1)]))
@pytest.mark.parametrize("M,N", sorted(opr.GEMM_SPLITK))
def test_gemm_split_k_is_exact(M, N, K):
    """Around the split threshold (K = 2047: one chunk; 2048 / 2049: four), chunks that end inside a K tile (3000 / 5 -> 608), empty trailing chunks
    (70000 / 136 -> 528: chunks 133..135 start past K), the 256-split cap (131073 at one tile) -- each with and without bias (k_op_splitk_sum adds it once),
    with and without accumulate (into an integer C), into ldc == N and ldc > N.  The number of splits is asserted from mshgnn_op_gemm_workspace."""
    _require_gpu()
    splits = opr.GEMM_SPLITK[(M, N)][K]
    bad = []
    placed = None
    for bias, acc in opr.gemm_variants():
        case = opr.gemm_operands(M, N, K, exact=True, bias=bias, accumulate=acc, splits=splits)
        placed = placed or (_place(case["A"], "row"), _place(case["B"], "row"))
        for wide in (False, True):
            d = _gemm(case, placed=placed, wide_ldc=wide, what=f"{M} x {N} x {K} ({splits} splits) bias={bias} accumulate={acc} ldc{'>' if wide else '='}N")
            if d:
                bad.append(d)
    assert not bad, "\n".join(bad[:10])


@pytest.mark.parametrize("M,N,K,splits", opr.GEMM_STRIDE_SHAPES)
def test_gemm_every_stride_pair_is_exact(M, N, K, splits):
    """A and B each row-major, column-major, row-major at a padded pitch and as a view with both strides != 1 (NaN between the elements): all 16 pairs,
    with bias and accumulate into ldc > N, and plain."""
    _require_gpu()
    bad = []
    for bias, acc, wide in ((True, True, True), (False, False, False)):
        case = opr.gemm_operands(M, N, K, exact=True, bias=bias, accumulate=acc, splits=splits)
        for la, lb in itertools.product(opr.GEMM_LAYOUTS, opr.GEMM_LAYOUTS):
            d = _gemm(case, la=la, lb=lb, wide_ldc=wide, what=f"{M} x {N} x {K} A {la} B {lb} bias={bias} accumulate={acc}")
            if d:
                bad.append(d)
    assert not bad, "\n".join(bad[:10])


@pytest.mark.parametrize("M,N,K,splits", opr.GEMM_UNIT_SHAPES)
def test_gemm_unit_dimensions_are_exact(M, N, K, splits):
    """M == 1, N == 1, K == 1: a row-major and a column-major operand then have the SAME strides in one of the indices, and the staging map is whatever
    the a_kc / b_kc rule picks -- every layout pair must still read the right elements."""
    _require_gpu()
    bad = []
    case = opr.gemm_operands(M, N, K, exact=True, bias=True, accumulate=True, splits=splits)
    for la, lb in itertools.product(opr.GEMM_LAYOUTS, opr.GEMM_LAYOUTS):
        d = _gemm(case, la=la, lb=lb, wide_ldc=True, what=f"{M} x {N} x {K} A {la} B {lb}")
        if d:
            bad.append(d)
    assert not bad, "\n".join(bad[:10])


@pytest.mark.parametrize("M,N,K,splits", opr.GEMM_RANDOM)
def test_gemm_random_data_is_within_the_elementwise_bound(M, N, K, splits):
    """Random fp32 operands (the shapes of test_linear_matches_reference's forward products, the ragged ones, one split-K point): every element within
    gamma_n (|A| |B|^T + |bias| + |C_in|), n = K + splits + bias + accumulate."""
    _require_gpu()
    bad = []
    for bias, acc in opr.gemm_variants():
        case = opr.gemm_operands(M, N, K, exact=False, bias=bias, accumulate=acc, splits=splits)
        for la, lb in (("row", "row"), ("row", "col"), ("col", "col")):      # y = x W^T, dx = dy W, dW = dy^T x
            d = _gemm(case, la=la, lb=lb, wide_ldc=acc, what=f"{M} x {N} x {K} A {la} B {lb} bias={bias} accumulate={acc}")
            if d:
                bad.append(d)
    assert not bad, "\n".join(bad[:10])


def test_gemm_error_returns_launch_nothing():
    """ldc < N, a split-K shape without a workspace, negative sizes, a null operand, more than 65535 row tiles: -1 (MSHGNN_EINVAL) and a message;
    M == 0 or N == 0: OK.  None of them launches: the NaN-filled C is untouched."""
    _require_gpu()
    lib = eng.load_library()
    A, B, Cb, ws = (torch.ones(64 * 64, dtype=torch.float32, device=DEV) for _ in range(4))
    Cb.fill_(float("nan"))

    def call(M, N, K, a=A, b=B, c=Cb, ldc=None, w=None):
        rc = lib.mshgnn_op_gemm(a.data_ptr() if a is not None else None, K, 1, b.data_ptr() if b is not None else None, K, 1, None,
                                c.data_ptr() if c is not None else None, N if ldc is None else ldc, M, N, K, 0, w.data_ptr() if w is not None else None, _stream())
        torch.cuda.synchronize()
        return rc

    for what, kw in [("ldc < N", dict(M=8, N=8, K=8, ldc=7)), ("no split-K workspace", dict(M=1, N=1, K=4096)), ("negative M", dict(M=-1, N=8, K=8)),
                     ("negative N", dict(M=8, N=-1, K=8)), ("negative K", dict(M=8, N=8, K=-1)), ("null A", dict(M=8, N=8, K=8, a=None)),
                     ("null B", dict(M=8, N=8, K=8, b=None)), ("null C", dict(M=8, N=8, K=8, c=None)),
                     ("more than 65535 row tiles", dict(M=65536 * 64, N=1, K=1))]:
        assert call(**kw) == -1, what
        assert lib.mshgnn_last_error().decode().startswith("mshgnn_op_gemm"), (what, lib.mshgnn_last_error())
    assert _splits(1, 1, 4096) > 1
    assert call(M=0, N=8, K=8) == 0 and call(M=8, N=0, K=8) == 0 and call(M=0, N=0, K=0, a=None, b=None, c=None) == 0
    assert bool(torch.isnan(Cb).all()), "an error return (or an empty product) wrote"
    assert call(M=1, N=1, K=4096, w=ws) == 0 and float(Cb[0]) == 4096.0 and bool(torch.isnan(Cb[1:]).all())      # (the same call with its workspace runs)


# ---------------------------------------------------------------------------------------------------
# 3. mshgnn_op_aggregate, Csr, mshgnn_op_colsum
# ---------------------------------------------------------------------------------------------------
def _aggregate_abi(case, ldx_pad, ldo_pad, what):
    lib = eng.load_library()
    n_rows, W = case["n_rows"], case["width"]
    xb = _nan(case["n_src"], W + ldx_pad)
    xb[:, :W] = case["x"].to(DEV)
    rowptr, col = case["rowptr"].to(DEV), case["col"].to(DEV)
    scale = case["scale"].to(DEV) if case["scale"] is not None else None
    wide = _nan(n_rows + 1, W + ldo_pad)
    rc = lib.mshgnn_op_aggregate(xb.data_ptr(), W + ldx_pad, rowptr.data_ptr(), col.data_ptr() if col.numel() else None, scale.data_ptr() if scale is not None and scale.numel() else None,
                                 wide.data_ptr(), W + ldo_pad, n_rows, W, _stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.mshgnn_last_error()
    inside = _check_frame(wide, 0, n_rows, 0, W, what)
    empty = case["deg"] == 0
    z = inside[empty]
    assert torch.count_nonzero(z) == 0 and not bool(torch.signbit(z).any()), f"{what}: a row without edges is not +0.0"
    where = lambda t: f"row group {t[0] // 8}, lane {t[1] % 32}, column pass {t[1] // 32}, in-degree {int(case['deg'][t[0]])}"
    d = opr.first_mismatch(inside, case["ref"], where) if case["exact"] else opr.within_bound(inside, case["ref"], case["bound"], where)
    return None if d is None else f"{what}: {d}"


@pytest.mark.parametrize("name,exact,mean,scale", opr.AGG_KINDS)
def test_aggregate_every_row_count_and_width(name, exact, mean, scale):
    """n_rows around the 8 rows of a workgroup, widths around the 32 lanes of a row, x and out at their own and at wider pitches (pads stay NaN), rows
    without edges (+0.0), repeated edges; scale NULL, an array of powers of two, 'mean' over power-of-two in-degrees: exact; other degrees: the bound."""
    _require_gpu()
    bad = []
    for kw in opr.all_aggregate_cases():
        if (kw["exact"], kw["mean"], kw["scale"]) != (exact, mean, scale) or kw.get("hub"):
            continue
        case = opr.aggregate_case(**kw)
        for ldx_pad, ldo_pad in ((0, 0), (3, 0), (0, 5), (1, 7)):
            d = _aggregate_abi(case, ldx_pad, ldo_pad, f"{name} {kw['n_rows']} x {kw['width']} ldx +{ldx_pad} ldo +{ldo_pad}")
            if d:
                bad.append(d)
    assert not bad, "\n".join(bad[:10])


@pytest.mark.parametrize("mean", [False, True])
def test_aggregate_a_destination_of_very_high_in_degree_is_exact(mean):
    """One destination with 100000 in-edges ('add') / 131072 ('mean': 1 / deg a power of two): one lane walks them all, in CSR order."""
    _require_gpu()
    kw = [k for k in opr.all_aggregate_cases() if k.get("hub") and k["mean"] == mean]
    assert len(kw) == 1
    case = opr.aggregate_case(**kw[0])
    assert int(case["deg"][0]) == kw[0]["hub"] >= 100000
    d = _aggregate_abi(case, 2, 3, f"hub of {kw[0]['hub']} edges, mean={mean}")
    assert d is None, d


def _edge_index_forms(src, dst):
    ei = torch.stack([src, dst])
    return {"int64": ei.to(DEV), "int32": ei.to(torch.int32).to(DEV), "non-contiguous": torch.stack([src, dst], dim=1).to(DEV).t()}


@pytest.mark.parametrize("mean", [False, True])
def test_csr_views_from_every_edge_index_form(mean):
    """ops.Csr from an int64, an int32 and a non-contiguous edge_index: the by-destination view aggregates to the reference, and the by-source view (the
    backward's) is its transpose: b[s] = sum over the edges out of s of scale(dst) g[dst].  Exact data."""
    _require_gpu()
    case = opr.aggregate_case(n_src=300, n_rows=1000, width=33, exact=True, mean=mean)
    src, dst = case["src"], case["dst"]
    g = opr._ints(torch.Generator().manual_seed(5), (1000, 33))
    w = (1.0 / case["deg"].clamp(min=1).double())[dst] if mean else torch.ones(dst.numel(), dtype=torch.float64)
    ref_b = torch.zeros(300, 33, dtype=torch.float64).index_add(0, src, g.double()[dst] * w[:, None])
    opr._require_closure(torch.zeros(300, 33, dtype=torch.float64).index_add(0, src, g.double().abs()[dst] * w[:, None]), opr._lsb(w), "by-source view")
    forms = _edge_index_forms(src, dst)
    assert not forms["non-contiguous"].is_contiguous() and forms["int32"].dtype == torch.int32
    for name, ei in forms.items():
        csr = ops.Csr(ei, 300, 1000, mean)
        f = ops._aggregate(case["x"].to(DEV), csr.f_rowptr, csr.f_col, csr.f_scale, 1000)
        b = ops._aggregate(g.to(DEV), csr.b_rowptr, csr.b_col, csr.b_scale, 300)
        torch.cuda.synchronize()
        d = opr.first_mismatch(f, case["ref"])
        assert d is None, f"{name} forward view: {d}"
        d = opr.first_mismatch(b, ref_b)
        assert d is None, f"{name} by-source view: {d}"


def test_csr_refuses_indices_outside_the_node_ranges():
    _require_gpu()
    for ei, what in [([[0, 5], [0, 1]], "source == n_src"), ([[0, 1], [0, 4]], "destination == n_dst"), ([[0, -1], [0, 1]], "negative source"),
                     ([[0, 1], [-1, 1]], "negative destination")]:
        for dt in (torch.int64, torch.int32):
            with pytest.raises(IndexError):
                ops.csr_of(torch.tensor(ei, dtype=dt, device=DEV), 5, 4, False)
    x = torch.ones(5, 8, device=DEV)
    with pytest.raises(IndexError):
        ops.graph_conv((x, x[:4]), torch.tensor([[0, 7], [0, 1]], device=DEV), torch.ones(8, 8, device=DEV), None, torch.ones(8, 8, device=DEV))


def test_csr_cache_sees_an_in_place_edit_of_the_edge_index():
    """The cache key carries the tensor's version: the same edge_index tensor edited in place between two calls gives the NEW graph's result."""
    _require_gpu()
    g = torch.Generator().manual_seed(11)
    xs, xd, Wr, Wo, b = opr._ints(g, (30, 8)), opr._ints(g, (20, 8)), opr._ints(g, (8, 8)), opr._ints(g, (8, 8)), opr._ints(g, (8,))
    ei = torch.stack([torch.randint(0, 30, (50,), generator=g), torch.randint(0, 20, (50,), generator=g)])
    eg = ei.to(DEV)

    def ref(e):
        agg = torch.zeros(20, 8, dtype=torch.float64).index_add(0, e[1], xs.double()[e[0]])
        return agg @ Wr.double().t() + b.double() + xd.double() @ Wo.double().t()

    def run():
        return ops.graph_conv((xs.to(DEV), xd.to(DEV)), eg, Wr.to(DEV), b.to(DEV), Wo.to(DEV), "add")

    assert opr.first_mismatch(run(), ref(ei)) is None
    ptr = eg.data_ptr()
    ei[1, :25] = (ei[1, :25] + 7) % 20
    ei[0, 25:] = (ei[0, 25:] + 3) % 30
    eg[1, :25] = ei[1, :25].to(DEV)
    eg[0, 25:] = ei[0, 25:].to(DEV)
    assert eg.data_ptr() == ptr and not torch.equal(ref(ei), ref(torch.stack([ei[0], (ei[1] + 1) % 20])))
    d = opr.first_mismatch(run(), ref(ei))
    assert d is None, f"after an in-place edit the OLD graph's CSR was served: {d}"


@pytest.mark.parametrize("exact", [True, False])
def test_colsum_every_row_count_and_width(exact):
    """M around OC_RB = 512 rows per first-stage block (0 rows: zeros; 70000: 137 blocks, exact data only), N around the 256 threads of a block, X at its
    own pitch and a wider one through the C-ABI, and through ops.colsum; out is N + 3 long and keeps its NaN tail."""
    _require_gpu()
    lib = eng.load_library()
    bad = []
    for M, N, ex in opr.all_colsum_cases():
        if ex != exact:
            continue
        case = opr.colsum_case(M, N, exact=exact)
        where = lambda t: f"column block {t[0] // 256}, thread {t[0] % 256}; {-(-M // 512)} row block(s), last one {M % 512 or 512} rows"
        for pad in (0, 3):
            xb = _nan(M + 1, N + pad)
            xb[:M, :N] = case["X"].to(DEV)
            out = _nan(N + 3)
            ws = torch.full((max(1, lib.mshgnn_op_colsum_workspace(M, N)),), 0xFF, dtype=torch.uint8, device=DEV)
            rc = lib.mshgnn_op_colsum(xb.data_ptr(), N + pad, out.data_ptr(), M, N, ws.data_ptr(), _stream())
            torch.cuda.synchronize()
            assert rc == 0, lib.mshgnn_last_error()
            assert bool(torch.isnan(out[N:]).all()) and bool(torch.isfinite(out[:N]).all()), (M, N, pad)
            d = opr.first_mismatch(out[:N], case["ref"], where) if exact else opr.within_bound(out[:N], case["ref"], case["bound"], where)
            if d:
                bad.append(f"{M} x {N} ldx +{pad}: {d}")
        got = ops.colsum(case["X"].to(DEV))
        d = opr.first_mismatch(got, case["ref"], where) if exact else opr.within_bound(got, case["ref"], case["bound"], where)
        if d:
            bad.append(f"ops.colsum {M} x {N}: {d}")
    assert not bad, "\n".join(bad[:10])


# ---------------------------------------------------------------------------------------------------
# 4. the autograd surface, exact
# ---------------------------------------------------------------------------------------------------
def _same_bits(got, ref64, what, bad):
    """got (any float dtype, device) == the fp64 reference cast to got's dtype (fp32 / fp64: the cast is exact, asserted; bf16: one rounding to nearest even
    of an exact value on both sides)."""
    if got.dtype != torch.bfloat16:
        assert torch.equal(ref64.float().double(), ref64), f"{what}: the reference is not an fp32 value"
    d = opr.first_mismatch(got, ref64.to(got.dtype).double().reshape(got.shape))
    if d:
        bad.append(f"{what}: {d}")


LINEAR_CASES = [(rows, three_d, bias, dt) for rows in (0, 5, 3000) for three_d in (False, True) for bias in (True, False)
                for dt in (torch.float64, torch.float32, torch.bfloat16)] + [(70000, False, True, torch.float32), (70000, True, False, torch.float64)]


@pytest.mark.parametrize("rows,three_d,bias,dt", LINEAR_CASES)
def test_linear_autograd_is_exact(rows, three_d, bias, dt):
    """ops.linear through nn.Linear: 2-D and 3-D input, with and without bias, fp64 / fp32 / bf16 tensors in and the same dtype out, zero rows (dW = 0,
    db = 0), and 3000 / 70000 rows, where dW = dy^T x runs split-K (asserted): output, dx, dW, db are the restated PyG Linear's fp64 bits."""
    _require_gpu()
    from morphsym_hgnn_amd import nn as pnn
    ref = _ref_nn()
    in_f, out_f = 33, 65
    g = torch.Generator().manual_seed(rows + 3 * three_d + bias)
    shape = (rows, in_f) if not three_d else ((rows // 100, 100, in_f) if rows >= 100 else ((1, rows, in_f) if rows else (0, 4, in_f)))
    x, W, b = opr._ints(g, shape).double(), opr._ints(g, (out_f, in_f)).double(), opr._ints(g, (out_f,)).double()
    gy = opr._ints(g, shape[:-1] + (out_f,)).double()
    worst = {}
    opr.prove_linear(x.reshape(-1, in_f), W, b if bias else None, gy.reshape(-1, out_f), worst=worst)
    if rows >= 3000:
        assert _splits(out_f, in_f, rows) > 1, "the weight gradient of this case is meant to run split-K"
    r = ref.Linear(in_f, out_f, bias=bias).double()
    m = pnn.Linear(in_f, out_f, bias=bias).to(dt).to(DEV)
    with torch.no_grad():
        for mod in (r, m):
            mod.weight.copy_(W)
            if bias:
                mod.bias.copy_(b)
    xr = x.clone().requires_grad_(True)
    xg = x.to(dt).to(DEV).requires_grad_(True)
    yr, y = r(xr), m(xg)
    assert y.dtype == dt and y.shape == yr.shape
    yr.backward(gy)
    y.backward(gy.to(dt).to(DEV))
    bad = []
    _same_bits(y, yr.detach(), "y", bad)
    _same_bits(xg.grad, xr.grad, "dx", bad)
    _same_bits(m.weight.grad, r.weight.grad, "dW", bad)
    if bias:
        _same_bits(m.bias.grad, r.bias.grad, "db", bad)
    assert xg.grad.dtype == dt and m.weight.grad.dtype == dt
    assert not bad, "\n".join(bad)


def _graph_conv_setup(aggr, n_src, n_dst, E_mode, seed, in_s=33, in_d=17, out_f=40):
    g = torch.Generator().manual_seed(seed)
    if E_mode == "none":
        src = dst = torch.zeros(0, dtype=torch.int64)
    else:
        src, dst = opr.make_graph(n_src, n_dst, seed, "pow2" if aggr == "mean" else "random")
    t = dict(xs=opr._ints(g, (n_src, in_s)), xd=opr._ints(g, (n_dst, in_d)), Wr=opr._ints(g, (out_f, in_s)), b=opr._ints(g, (out_f,)),
             Wo=opr._ints(g, (out_f, in_d)), gy=opr._ints(g, (n_dst, out_f)))
    t = {k: v.double() for k, v in t.items()}
    opr.prove_graph_conv(t["xs"], t["xd"], t["Wr"], t["b"], t["Wo"], src, dst, aggr == "mean", t["gy"])
    return t, torch.stack([src, dst])


def _set_graph_conv(mod, t):
    with torch.no_grad():
        mod.lin_rel.weight.copy_(t["Wr"]); mod.lin_rel.bias.copy_(t["b"]); mod.lin_root.weight.copy_(t["Wo"])


GRAPH_CONV_CASES = [(aggr, ns, nd, mode) for aggr in ("add", "mean") for ns, nd, mode in
                    [(12, 9, "edges"), (5, 9, "none"), (2000, 3000, "edges"), (3000, 3000, "edges"), (40000, 70000, "edges")]]


@pytest.mark.parametrize("aggr,n_src,n_dst,mode", GRAPH_CONV_CASES)
def test_graph_conv_autograd_is_exact(aggr, n_src, n_dst, mode):
    """ops.graph_conv through nn.GraphConv, bipartite (n_src != n_dst) and square, 'add' on a multigraph and 'mean' over power-of-two in-degrees, destinations
    without in-edges (every fourth and the last one), E == 0, and 3000 / 70000 destinations, where both weight gradients run split-K (asserted): the output
    and the gradients of x_src, x_dst, lin_rel.weight, lin_rel.bias, lin_root.weight are the restated PyG GraphConv's fp64 bits."""
    _require_gpu()
    from morphsym_hgnn_amd import nn as pnn
    ref = _ref_nn()
    t, ei = _graph_conv_setup(aggr, n_src, n_dst, mode, seed=n_src + n_dst)
    if n_dst >= 3000:
        assert _splits(40, 33, n_dst) > 1 and _splits(40, 17, n_dst) > 1
    r = ref.GraphConv((33, 17), 40, aggr=aggr).double()
    m = pnn.GraphConv((33, 17), 40, aggr=aggr).double().to(DEV)
    _set_graph_conv(r, t); _set_graph_conv(m, t)
    a = [t[k].clone().requires_grad_(True) for k in ("xs", "xd")]
    c = [t[k].to(DEV).requires_grad_(True) for k in ("xs", "xd")]
    yr, y = r((a[0], a[1]), ei), m((c[0], c[1]), ei.to(DEV))
    yr.backward(t["gy"]); y.backward(t["gy"].to(DEV))
    bad = []
    _same_bits(y, yr.detach(), "out", bad)
    _same_bits(c[0].grad, a[0].grad, "dx_src", bad)
    _same_bits(c[1].grad, a[1].grad, "dx_dst", bad)
    for k in ("lin_rel.weight", "lin_rel.bias", "lin_root.weight"):
        _same_bits(m.get_parameter(k).grad, r.get_parameter(k).grad, "d" + k, bad)
    if mode != "none":
        assert float(a[0].grad.abs().max()) > 0 and float(r.lin_rel.weight.grad.abs().max()) > 0
    assert not bad, "\n".join(bad)


def test_graph_conv_every_subset_of_requires_grad():
    """The five inputs of _GraphConv (x_src, x_dst, lin_rel.weight, lin_rel.bias, lin_root.weight) under each of the 32 requires_grad patterns: the gradients
    asked for are the same bits as with all five, the others are None, nothing raises."""
    _require_gpu()
    t, ei = _graph_conv_setup("mean", 12, 9, "edges", seed=4)
    names = ["xs", "xd", "Wr", "b", "Wo"]
    eg = ei.to(DEV)

    def run(mask):
        leaves = [t[k].to(DEV).requires_grad_(bool(f)) for k, f in zip(names, mask)]
        y = ops.graph_conv((leaves[0], leaves[1]), eg, leaves[2], leaves[3], leaves[4], "mean")
        if any(mask):
            y.backward(t["gy"].to(DEV))
        else:
            assert not y.requires_grad
        return y.detach(), [l.grad for l in leaves]

    y_all, g_all = run((1,) * 5)
    assert all(g is not None for g in g_all)
    for mask in itertools.product((0, 1), repeat=5):
        y, gs = run(mask)
        assert torch.equal(y, y_all), mask
        for k, f, g, ga in zip(names, mask, gs, g_all):
            assert (g is not None) == bool(f), (mask, k)
            if f:
                assert torch.equal(g, ga), (mask, k)


@pytest.mark.parametrize("n", [9, 3000])
def test_hetero_conv_sums_three_relations_into_one_destination_type_exactly(n):
    """nn.HeteroConv with three relations (two source types, 'add' and 'mean') into one destination type and one into another: every output and every
    gradient equal the restated PyG HeteroConv's fp64 bits (the sums over the relations are exact: integer / dyadic terms far below 2^24)."""
    _require_gpu()
    from morphsym_hgnn_amd import nn as pnn
    ref = _ref_nn()
    H = 32
    rels = [("a", "r1", "c"), ("b", "r2", "c"), ("c", "r3", "c"), ("c", "r4", "a")]
    aggr = {"r1": "add", "r2": "mean", "r3": "add", "r4": "mean"}
    sizes = {"a": n + 3, "b": 7, "c": n}
    g = torch.Generator().manual_seed(n)
    x = {k: opr._ints(g, (v, H)).double() for k, v in sizes.items()}
    ei, P = {}, {}
    for s, rname, d in rels:
        src, dst = opr.make_graph(sizes[s], sizes[d], len(ei) + n, "pow2" if aggr[rname] == "mean" else "random")
        ei[(s, rname, d)] = torch.stack([src, dst])
        P[(s, rname, d)] = dict(Wr=opr._ints(g, (H, H)).double(), b=opr._ints(g, (H,)).double(), Wo=opr._ints(g, (H, H)).double())
    gy = {k: opr._ints(g, (sizes[k], H)).double() for k in ("c", "a")}
    for et in rels:
        opr.prove_graph_conv(x[et[0]], x[et[2]], P[et]["Wr"], P[et]["b"], P[et]["Wo"], ei[et][0], ei[et][1], aggr[et[1]] == "mean", gy[et[2]], what=str(et))

    def build(nnmod):
        hc = nnmod.HeteroConv({et: nnmod.GraphConv(H, H, aggr=aggr[et[1]]) for et in rels}, aggr="sum").double()
        for et in rels:
            conv = hc.convs["<" + "___".join(et) + ">"] if nnmod is ref else hc.convs[et]
            _set_graph_conv(conv, P[et])
        return hc

    r, m = build(ref), build(pnn).to(DEV)
    xr = {k: v.clone().requires_grad_(True) for k, v in x.items()}
    xg = {k: v.to(DEV).requires_grad_(True) for k, v in x.items()}
    yr, y = r(xr, ei), m(xg, {k: v.to(DEV) for k, v in ei.items()})
    assert set(y) == set(yr) == {"c", "a"}
    sum(((yr[k] * gy[k]).sum() for k in yr)).backward()
    sum(((y[k] * gy[k].to(DEV)).sum() for k in y)).backward()
    bad = []
    for k in yr:
        _same_bits(y[k], yr[k].detach(), f"out[{k}]", bad)
    for k in x:
        _same_bits(xg[k].grad, xr[k].grad, f"dx[{k}]", bad)
    for (kd, pd), (ks, ps) in zip(sorted(m.named_parameters()), sorted(r.named_parameters())):
        assert kd == ks
        _same_bits(pd.grad, ps.grad, "d" + kd, bad)
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------------------------------------------
# 5. the operator-by-operator model path against the oracle, bit for bit
# ---------------------------------------------------------------------------------------------------
class ReluByAnotherName(torch.nn.Module):
    """Computes relu (gradient 0 at 0, as the oracle's) without being an nn.ReLU: models.py then takes the operator path."""

    def forward(self, x):
        return torch.relu(x)


MODEL_FAMILIES = ["a1c2_L3", "a1c2_L5", "mck4_cls_L5", "mi_L5", "solok4_com_L4", "solos4_com_L5"]
MODEL_CASES = [(m, B) for m in MODEL_FAMILIES for B in (17, 1000)]      # (the seeds are the table's: tests/test_exact_data.py proves the operator algebra closes for each)


@pytest.mark.parametrize("model,B", MODEL_CASES)
def test_operator_model_path_is_the_oracle_bit_for_bit(model, B):
    """models._forward_operators (chosen because the activation is not an nn.ReLU) on the rounding-free cases of tests/exact_data.py, the table and
    reference of tests/test_exact_gpu.py: A1-C2 at 3 and 5 layers (base as a destination, base_transform, residual), MiniCheetah-K4 classification (the
    gt / gs mean relations; logits), MI-HGNN (no symmetry, no residual), Solo K4 and S4 centroidal momentum (decoder on the base nodes, the [B, n_base, 6]
    and window-major output shapes), at 17 and 1000 windows.  The output and every parameter gradient of (out * gout).sum().backward() are the oracle's
    bits; where the oracle's gradient is None / exact zero the module's is None or exact zero.  At 1000 windows the weight-gradient GEMMs reduce over
    1000 n_t rows: split-K, asserted for the widest type."""
    _require_gpu()
    from tests import test_exact_families_gpu  # noqa: F401  (adds the families to the table)
    from tests import test_exact_gpu as gx
    from tests.test_models import _build
    spec, case, ref, _ = gx._reference(model, B)
    s = gx.MODELS[model]["spec"]
    m = _build(dict(kind=s[0], cfg=s[2], hidden=s[3], layers=s[4], regression=s[5], grf=s[6] if len(s) > 6 else 3), spec, activation_fn=ReluByAnotherName())
    m = m.double().to(DEV)
    assert not m._fused_activation
    x = {k: v.to(DEV) for k, v in case["x"].items()}
    ei = {k: v.to(DEV) for k, v in spec.topology.edge_index_dict(B).items()}
    with torch.no_grad():
        m(x_dict={k: v.clone() for k, v in x.items()}, edge_index_dict=ei)      # lazy encoder, spec
    m.load_state_dict(case["params"])
    out = m(x_dict=x, edge_index_dict=ei)
    assert out.dtype == torch.float64
    bad = []
    _same_bits(out.reshape(-1), ref["out"], "out", bad)
    (out.reshape(-1) * ref["gout"].to(DEV)).sum().backward()
    for k, p in m.named_parameters():
        r = ref["grads"].get(k)
        if r is None or float(r.abs().max()) == 0.0:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, f"{k}: the oracle's gradient is zero, the module's is not"
        else:
            assert p.grad is not None, k
            _same_bits(p.grad, r, "d" + k, bad)
    if B >= 1000:
        n_t = max(spec.num_nodes.values())
        assert _splits(spec.hidden, spec.hidden, B * n_t) > 1, "the weight-gradient GEMMs of this batch are meant to run split-K"
    assert not bad, "\n".join(bad[:10])
