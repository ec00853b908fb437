"""The fp64 stand-alone operators (csrc/mshgnn_ops.hip: k_op_gemm_f64 on v_mfma_f64_16x16x4_f64 and the double instantiations of k_op_splitk_sum, k_op_aggregate,
k_op_colsum1/2 behind mshgnn_op_gemm_f64 / _aggregate_f64 / _colsum_f64; ops.compute_dtype("f64")) ELEMENT BY ELEMENT, on the matrix of
tests/test_ops_exact_gpu.py with the data of tests/ops_f64_reference.py:
  * wide_sum (integers whose sums reach 2^52: wrong under any fp32 accumulation) and wide_operand (26-bit operands, one term per sum: wrong under any
    narrowing of an operand) must be the exact integer result BIT FOR BIT; dyadic random data must lie within gamma_{2K+4}(2^-53) sum |terms| of the
    unrounded reference.  tests/test_ops_f64_reference.py proves on the host that these checkers reject every damaged variant for every case run here.
  * test_layout_probe runs first: one 16 x 16 x 4 product of distinct small integers -- a wrong operand or accumulator map of the f64 MFMA shows there as
    a permutation, before the tiling, the staging and split-K enter.
  * every output sits in a NaN frame that must stay NaN (sentinels behind every output), a second run must give the same bits, a refused call must leave
    its outputs untouched.
  * autograd: ops.linear and ops.graph_conv ('add' and 'mean') under compute_dtype("f64") on wide integer data -- output and all five gradients are the
    integer algebra's bits; under the default mode the same calls give the fp32 route's bits, compared against a fresh process in which the mode was
    never touched.
"""
import ctypes as C
import itertools
import os
import subprocess
import sys

import pytest
import torch

from morphsym_hgnn_amd import engine as eng
from morphsym_hgnn_amd import ops
from tests import ops_f64_reference as r64
from tests import ops_reference as opr

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _require_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (there is no CPU fallback to fall through to)")


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float64, device=DEV)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _place(mat, layout):
    """A logical fp64 [R, K] host matrix in device memory as `layout`: (buffer, stride of the row index, stride of k); everything between the elements
    is NaN, so a kernel that reads outside (r < R, k < K) poisons its result."""
    R, K = mat.shape
    if layout == "row":
        return mat.contiguous().to(DEV), K, 1
    if layout == "col":
        return mat.t().contiguous().to(DEV), 1, R
    if layout == "pad":
        buf = _nan(R, K + 5)
        buf[:, :K] = mat.to(DEV)
        return buf, K + 5, 1
    if layout == "view":
        buf = _nan(R, 2 * K + 1)
        buf[:, 0:2 * K:2] = mat.to(DEV)
        return buf, 2 * K + 1, 2
    raise KeyError(layout)


def _splits(M, N, K):
    lib = eng.load_library()
    s, s32 = C.c_int32(-1), C.c_int32(-1)
    need = lib.mshgnn_op_gemm_f64_workspace(M, N, K, C.byref(s))
    lib.mshgnn_op_gemm_workspace(M, N, K, C.byref(s32))
    assert s.value == s32.value, "the fp64 GEMM splits K by the fp32 operator's rule"
    assert (need > 0) == (s.value > 1) and (need == 0 or need == s.value * M * N * 8)
    return s.value


def _check_frame(wide, r0, r1, c0, c1, what):
    host = wide.cpu()
    outside = torch.ones_like(host, dtype=torch.bool)
    outside[r0:r1, c0:c1] = False
    assert bool(torch.isnan(host[outside]).all()), f"{what}: wrote outside its {r1 - r0} x {c1 - c0} result"
    inside = host[r0:r1, c0:c1]
    assert bool(torch.isfinite(inside).all()), f"{what}: {int((~torch.isfinite(inside)).sum())} elements of the result were not written (or are not finite)"
    return inside


def _gemm(case, placed=None, la="row", lb="row", wide_ldc=False, what="", twice=False):
    """ops.gemm under the f64 mode on `case` (ops_f64_reference.gemm_case) into a NaN frame; the failure description or None."""
    M, N, K = case["M"], case["N"], case["K"]
    (A, sAm, sAk), (B, sBn, sBk) = placed if placed is not None else (_place(case["A"], la), _place(case["B"], lb))
    bias = case["bias"].to(DEV) if case["bias"] is not None else None
    off = 1 if wide_ldc else 0
    assert _splits(M, N, K) == case["splits"], f"{what}: takes {_splits(M, N, K)} K split(s), the case is named for {case['splits']}"
    runs = []
    for _ in range(2 if twice else 1):
        wide = _nan(M + 2, N + (4 if wide_ldc else 0))
        out = wide[:M, off:off + N]
        if case["C_in"] is not None:
            out.copy_(case["C_in"])
        with ops.compute_dtype("f64"):
            r = ops.gemm(A, sAm, sAk, B, sBn, sBk, M, N, K, bias=bias, out=out, accumulate=case["C_in"] is not None)
        torch.cuda.synchronize()
        assert r.data_ptr() == out.data_ptr() and r.dtype == torch.float64
        runs.append(_check_frame(wide, 0, M, off, off + N, what))
    if twice and not torch.equal(runs[0], runs[1]):
        return f"{what}: two runs differ"
    d = r64.gemm_failure(case, runs[0], opr.gemm_where(K, case["splits"]))
    return None if d is None else f"{what} [{case['family']}]: {d}"


# ---------------------------------------------------------------------------------------------------
# 1. the operand maps of the f64 MFMA
# ---------------------------------------------------------------------------------------------------
def test_layout_probe():
    """C = A B^T for A [16, 4], B [16, 4] of distinct small integers (A: 1 + 4 m + k, B: 101 + 4 n + k): one MFMA's worth.  Every element of the exact
    result identifies its (row, column) and the four k it summed; a wrong lane map gives a permuted or mixed matrix, and the message names the map."""
    _require_gpu()
    A = (1 + torch.arange(64, dtype=torch.float64)).view(16, 4)
    B = (101 + torch.arange(64, dtype=torch.float64)).view(16, 4)
    want = A @ B.t()
    assert len(set(want.flatten().tolist())) > 200      # (nearly) every element distinct: a permutation cannot hide
    with ops.compute_dtype("f64"):
        got = ops.gemm(A.to(DEV), 4, 1, B.to(DEV), 4, 1, 16, 16, 4).cpu()
    if not torch.equal(got, want):
        hint = "rows permuted: the C/D map (col = lane & 15, row = (lane >> 4) + 4 reg) is off" if torch.equal(got.sort(0).values, want.sort(0).values) else \
               "the transpose: A and B operands swapped" if torch.equal(got, want.t()) else "neither a row permutation nor the transpose: the A / B k map (k = lane >> 4) or the staging"
        pytest.fail(f"16 x 16 x 4 probe: {opr.first_mismatch(got, want)} -- {hint}")


# ---------------------------------------------------------------------------------------------------
# 2. mshgnn_op_gemm_f64
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", r64.GEMM_EDGE_K)
def test_gemm_edges_are_exact(K):
    """Every M, N on both sides of the 16-row MFMA block, the 32-row wave tile and the 64-row workgroup tile at K around the 4-wide MFMA step and the 16-wide
    K tile (K == 0: bias / C_in alone, also from padded operands), with and without bias and accumulate, ldc == N and ldc > N, both exact families."""
    _require_gpu()
    bad = []
    for M, N in itertools.product(r64.GEMM_EDGE_MN, r64.GEMM_EDGE_MN):
        for i, (bias, acc) in enumerate(opr.gemm_variants()):
            for fam in ("wide_sum", "wide_operand"):
                case = r64.gemm_case(M, N, K, fam, bias=bias, accumulate=acc)
                for lay in (("row", "row"), ("pad", "pad")) if K == 0 else (("row", "row"),):
                    d = _gemm(case, la=lay[0], lb=lay[1], wide_ldc=bool((i + M + N) & 1), what=f"{M} x {N} x {K} bias={bias} accumulate={acc} {lay}")
                    if d:
                        bad.append(d)
    assert not bad, "\n".join(bad[:10])


@pytest.mark.parametrize("K", sorted(r64.GEMM_SPLITK[(1, 1)]))
@pytest.mark.parametrize("M,N", sorted(r64.GEMM_SPLITK))
def test_gemm_split_k_is_exact(M, N, K):
    """Around the split threshold, chunks that end inside a K tile, empty trailing chunks, the 256-split cap -- with and without bias (added once, by the
    fixed-order sum) and accumulate, ldc == N and ldc > N; the split count is asserted, and equal to the fp32 operator's.  Two runs, equal bits."""
    _require_gpu()
    splits = r64.GEMM_SPLITK[(M, N)][K]
    bad = []
    for fam in ("wide_sum", "wide_operand"):
        placed = None
        for bias, acc in opr.gemm_variants():
            case = r64.gemm_case(M, N, K, fam, bias=bias, accumulate=acc, splits=splits)
            placed = placed or (_place(case["A"], "row"), _place(case["B"], "row"))
            d = _gemm(case, placed=placed, wide_ldc=bias != acc, twice=bias and acc, what=f"{M} x {N} x {K} ({splits} splits) bias={bias} accumulate={acc}")
            if d:
                bad.append(d)
    assert not bad, "\n".join(bad[:10])


@pytest.mark.parametrize("M,N,K,splits", r64.GEMM_STRIDE_SHAPES)
def test_gemm_every_stride_pair_is_exact(M, N, K, splits):
    """A and B each row-major, column-major, padded and as a view with both strides != 1 (NaN between the elements): all 16 pairs -- the staging rule that
    reads along the contiguous index serves x W^T, dY W and dY^T X -- with bias and accumulate into ldc > N, and plain."""
    _require_gpu()
    bad = []
    for fam in ("wide_sum", "wide_operand"):
        for bias, acc, wide in ((True, True, True), (False, False, False)):
            case = r64.gemm_case(M, N, K, fam, bias=bias, accumulate=acc, splits=splits)
            for la, lb in itertools.product(r64.GEMM_LAYOUTS, r64.GEMM_LAYOUTS):
                d = _gemm(case, la=la, lb=lb, wide_ldc=wide, what=f"{M} x {N} x {K} A {la} B {lb} bias={bias} accumulate={acc}")
                if d:
                    bad.append(d)
    assert not bad, "\n".join(bad[:10])


@pytest.mark.parametrize("M,N,K,splits", r64.GEMM_UNIT_SHAPES)
def test_gemm_unit_dimensions_are_exact(M, N, K, splits):
    """M == 1, N == 1, K == 1: row- and column-major operands share strides and the staging map is whatever the rule picks; every layout pair is exact."""
    _require_gpu()
    bad = []
    for fam in ("wide_sum", "wide_operand"):
        case = r64.gemm_case(M, N, K, fam, bias=True, accumulate=True, splits=splits)
        for la, lb in itertools.product(r64.GEMM_LAYOUTS, r64.GEMM_LAYOUTS):
            d = _gemm(case, la=la, lb=lb, wide_ldc=True, what=f"{M} x {N} x {K} A {la} B {lb}")
            if d:
                bad.append(d)
    assert not bad, "\n".join(bad[:10])


def test_gemm_weight_gradient_shape_is_exact():
    """70000 x 128 x 128 (1094 row tiles: the grid's y extent far past one wave of workgroups), exact families only, as y = x W^T and as dW = dY^T X
    (128 x 128 x 70000: column-major operands, split-K)."""
    _require_gpu()
    M, N, K, _ = r64.GEMM_WGRAD
    bad = []
    for fam in ("wide_sum", "wide_operand"):
        d = _gemm(r64.gemm_case(M, N, K, fam, bias=True), twice=True, what=f"{M} x {N} x {K}")
        if d:
            bad.append(d)
    s = _splits(128, 128, 70000)
    assert s > 1
    d = _gemm(r64.gemm_case(128, 128, 70000, "wide_sum", splits=s), la="col", lb="col", twice=True, what="128 x 128 x 70000 dY^T X")
    if d:
        bad.append(d)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("M,N,K,splits", r64.GEMM_RANDOM)
def test_gemm_random_data_is_within_the_elementwise_bound(M, N, K, splits):
    """Dyadic random operands: every element within gamma_{2K+4}(2^-53) (|A| |B|^T + |bias| + |C_in|) of the UNROUNDED reference (int64 arithmetic), in the
    three layouts of a Linear's products."""
    _require_gpu()
    bad = []
    for bias, acc in opr.gemm_variants():
        case = r64.gemm_case(M, N, K, "random", bias=bias, accumulate=acc, splits=splits)
        for la, lb in (("row", "row"), ("row", "col"), ("col", "col")):
            d = _gemm(case, la=la, lb=lb, wide_ldc=acc, what=f"{M} x {N} x {K} A {la} B {lb} bias={bias} accumulate={acc}")
            if d:
                bad.append(d)
    assert not bad, "\n".join(bad[:10])


def test_gemm_error_returns_launch_nothing():
    """Every MSHGNN_EINVAL refusal of the fp32 entry point, on the fp64 one: -1, a message, and the NaN-filled C untouched; M == 0 / N == 0: OK, nothing written."""
    _require_gpu()
    lib = eng.load_library()
    A, B, Cb, ws = (torch.ones(64 * 64, dtype=torch.float64, device=DEV) for _ in range(4))
    Cb.fill_(float("nan"))

    def call(M, N, K, a=A, b=B, c=Cb, ldc=None, w=None):
        rc = lib.mshgnn_op_gemm_f64(a.data_ptr() if a is not None else None, K, 1, b.data_ptr() if b is not None else None, K, 1, None,
                                    c.data_ptr() if c is not None else None, N if ldc is None else ldc, M, N, K, 0, w.data_ptr() if w is not None else None, _stream())
        torch.cuda.synchronize()
        return rc

    for what, kw in [("ldc < N", dict(M=8, N=8, K=8, ldc=7)), ("no split-K workspace", dict(M=1, N=1, K=4096)), ("negative M", dict(M=-1, N=8, K=8)),
                     ("negative N", dict(M=8, N=-1, K=8)), ("negative K", dict(M=8, N=8, K=-1)), ("null A", dict(M=8, N=8, K=8, a=None)),
                     ("null B", dict(M=8, N=8, K=8, b=None)), ("null C", dict(M=8, N=8, K=8, c=None)),
                     ("more than 65535 row tiles", dict(M=65536 * 64, N=1, K=1))]:
        assert call(**kw) == -1, what
        assert lib.mshgnn_last_error().decode().startswith("mshgnn_op_gemm_f64"), (what, lib.mshgnn_last_error())
    assert call(M=0, N=8, K=8) == 0 and call(M=8, N=0, K=8) == 0 and call(M=0, N=0, K=0, a=None, b=None, c=None) == 0
    assert bool(torch.isnan(Cb).all()), "an error return (or an empty product) wrote"
    assert call(M=1, N=1, K=4096, w=ws) == 0 and float(Cb[0]) == 4096.0 and bool(torch.isnan(Cb[1:]).all())
    with ops.compute_dtype("f64"), pytest.raises(TypeError):      # the Python surface refuses an fp32 buffer under the f64 mode instead of misreading it
        ops.gemm(A.float(), 8, 1, B, 8, 1, 8, 8, 8)


# ---------------------------------------------------------------------------------------------------
# 3. mshgnn_op_aggregate_f64, the Csr scales, mshgnn_op_colsum_f64
# ---------------------------------------------------------------------------------------------------
def _aggregate_abi(case, ldx_pad, ldo_pad, what):
    lib = eng.load_library()
    n_rows, W = case["n_rows"], case["width"]
    xb = _nan(case["n_src"], W + ldx_pad)
    xb[:, :W] = case["x"].to(DEV)
    rowptr, col = case["rowptr"].to(DEV), case["col"].to(DEV)
    scale = case["scale"].to(DEV) if case["scale"] is not None else None
    runs = []
    for _ in range(2):
        wide = _nan(n_rows + 1, W + ldo_pad)
        rc = lib.mshgnn_op_aggregate_f64(xb.data_ptr(), W + ldx_pad, rowptr.data_ptr(), col.data_ptr() if col.numel() else None,
                                         scale.data_ptr() if scale is not None and scale.numel() else None, wide.data_ptr(), W + ldo_pad, n_rows, W, _stream())
        torch.cuda.synchronize()
        assert rc == 0, lib.mshgnn_last_error()
        runs.append(_check_frame(wide, 0, n_rows, 0, W, what))
    assert torch.equal(runs[0], runs[1]), f"{what}: two runs differ"
    inside = runs[0]
    z = inside[case["deg"] == 0]
    assert torch.count_nonzero(z) == 0 and not bool(torch.signbit(z).any()), f"{what}: a row without edges is not +0.0"
    where = lambda t: f"row group {t[0] // 8}, lane {t[1] % 32}, column pass {t[1] // 32}, in-degree {int(case['deg'][t[0]])}"
    d = opr.first_mismatch(inside, case["ref"], where) if case["bound"] is None else opr.within_bound(inside, case["ref"], case["bound"], where)
    return None if d is None else f"{what}: {d}"


@pytest.mark.parametrize("name,exact,mean,scale", r64.AGG_KINDS)
def test_aggregate_every_row_count_and_width(name, exact, mean, scale):
    """The fp32 matrix (row counts around the 8 rows of a workgroup, widths around the 32 lanes of a row, own and wider pitches, rows without edges,
    repeated edges) on fp64 data: wide integers, 31-bit edge scales, 'mean' over power-of-two degrees and dyadic data: exact; 'mean' over other degrees: the bound."""
    _require_gpu()
    bad = []
    for kw in r64.all_aggregate_cases():
        if (kw["exact"], kw["mean"], kw["scale"]) != (exact, mean, scale) or kw.get("hub"):
            continue
        case = r64.aggregate_case64(**kw)
        for ldx_pad, ldo_pad in ((0, 0), (1, 7)):
            d = _aggregate_abi(case, ldx_pad, ldo_pad, f"{name} {kw['n_rows']} x {kw['width']} ldx +{ldx_pad} ldo +{ldo_pad}")
            if d:
                bad.append(d)
    assert not bad, "\n".join(bad[:10])


@pytest.mark.parametrize("mean", [False, True])
def test_aggregate_a_destination_of_very_high_in_degree_is_exact(mean):
    _require_gpu()
    kw = [k for k in r64.all_aggregate_cases() if k.get("hub") and k["mean"] == mean]
    assert len(kw) == 1
    case = r64.aggregate_case64(**kw[0])
    assert int(case["deg"][0]) == kw[0]["hub"] >= 100000 and float(case["ref"][0].abs().max()) > 2.0 ** 30
    d = _aggregate_abi(case, 2, 3, f"hub of {kw[0]['hub']} edges, mean={mean}")
    assert d is None, d


def test_aggregate_and_colsum_refusals_leave_their_outputs_untouched():
    _require_gpu()
    lib = eng.load_library()
    x, out = torch.ones(64, dtype=torch.float64, device=DEV), _nan(64)
    rp = torch.zeros(9, dtype=torch.int32, device=DEV)
    for kw in (dict(n=-1, w=8), dict(n=8, w=-1), dict(n=8, w=8, rp=None), dict(n=8, w=8, out=None)):
        rc = lib.mshgnn_op_aggregate_f64(x.data_ptr(), 8, None if "rp" in kw else rp.data_ptr(), None, None, None if "out" in kw else out.data_ptr(), 8, kw["n"], kw["w"], _stream())
        assert rc == -1 and lib.mshgnn_last_error().decode().startswith("mshgnn_op_aggregate_f64"), kw
    ws = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    for kw in (dict(M=-1, N=8), dict(M=8, N=-1), dict(M=8, N=8, out=None), dict(M=8, N=8, X=None), dict(M=8, N=8, ws=None)):
        rc = lib.mshgnn_op_colsum_f64(None if "X" in kw else x.data_ptr(), 8, None if "out" in kw else out.data_ptr(), kw["M"], kw["N"], None if "ws" in kw else ws.data_ptr(), _stream())
        assert rc == -1 and lib.mshgnn_last_error().decode().startswith("mshgnn_op_colsum_f64"), kw
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()), "a refused call wrote"
    assert lib.mshgnn_op_aggregate_f64(None, 8, None, None, None, None, 8, 0, 8, _stream()) == 0 and lib.mshgnn_op_colsum_f64(None, 8, None, 8, 0, None, _stream()) == 0


@pytest.mark.parametrize("mean", [False, True])
def test_csr_scales_follow_the_compute_dtype(mean):
    """ops.Csr hands the fp64 kernels 1 / deg divided in fp64 (in-degrees 1..5: 1 / 3 and 1 / 5 are no fp32 values) for both views, and keeps handing the
    fp32 kernels the fp32 scales it always built."""
    _require_gpu()
    case = r64.aggregate_case64(n_src=300, n_rows=1000, width=33, exact=False, mean=mean)
    ei = torch.stack([case["src"], case["dst"]]).to(DEV)
    csr = ops.Csr(ei, 300, 1000, mean)
    f32 = (None, None) if not mean else (csr.f_scale.clone(), csr.b_scale.clone())
    f, b = csr.scales(torch.float64)
    if not mean:
        assert f is None and b is None and csr.scales(torch.float32) == (None, None)
    else:
        inv = 1.0 / case["deg"].clamp(min=1).double()
        rows = torch.repeat_interleave(torch.arange(1000), case["deg"])
        assert f.dtype == torch.float64 and torch.equal(f.cpu(), inv[rows]) and torch.equal(b.cpu(), inv[csr.b_col.cpu().long()])
        assert not torch.equal(f.float().double(), f)
        s32 = csr.scales(torch.float32)
        assert s32[0] is csr.f_scale and torch.equal(s32[0], f32[0]) and torch.equal(s32[1], f32[1]) and s32[0].dtype == torch.float32
    got = ops._aggregate(case["x"].to(DEV), csr.f_rowptr, csr.f_col, f, 1000)
    d = opr.first_mismatch(got, case["ref"]) if case["bound"] is None else opr.within_bound(got, case["ref"], case["bound"])
    assert d is None, d


@pytest.mark.parametrize("wide", [True, False])
def test_colsum_every_row_count_and_width(wide):
    """M around the 512 rows of a first-stage block (0 rows: zeros; 70000: 137 blocks), N around the 256 threads of a block, X at its own pitch and a wider
    one through the C-ABI, and through ops.colsum; out is N + 3 long and keeps its NaN tail; bit equality on both data kinds."""
    _require_gpu()
    lib = eng.load_library()
    bad = []
    for M, N, w in r64.all_colsum_cases():
        if w != wide:
            continue
        case = r64.colsum_case64(M, N, wide=wide)
        where = lambda t: f"column block {t[0] // 256}, thread {t[0] % 256}; {-(-M // 512)} row block(s), last one {M % 512 or 512} rows"
        for pad in (0, 3):
            xb = _nan(M + 1, N + pad)
            xb[:M, :N] = case["X"].to(DEV)
            out = _nan(N + 3)
            need = lib.mshgnn_op_colsum_f64_workspace(M, N)
            assert need == -(-M // 512) * N * 8
            ws = torch.full((max(1, need),), 0xFF, dtype=torch.uint8, device=DEV)
            rc = lib.mshgnn_op_colsum_f64(xb.data_ptr(), N + pad, out.data_ptr(), M, N, ws.data_ptr(), _stream())
            torch.cuda.synchronize()
            assert rc == 0, lib.mshgnn_last_error()
            assert bool(torch.isnan(out[N:]).all()) and bool(torch.isfinite(out[:N]).all()), (M, N, pad)
            d = opr.first_mismatch(out[:N], case["ref"], where)
            if d:
                bad.append(f"{M} x {N} ldx +{pad}: {d}")
        with ops.compute_dtype("f64"):
            a, b = ops.colsum(case["X"].to(DEV)), ops.colsum(case["X"].to(DEV))
        d = opr.first_mismatch(a, case["ref"], where)
        if d or not torch.equal(a, b):
            bad.append(f"ops.colsum {M} x {N}: {d or 'two runs differ'}")
    assert not bad, "\n".join(bad[:10])


# ---------------------------------------------------------------------------------------------------
# 4. the autograd surface under the mode
# ---------------------------------------------------------------------------------------------------
def _linear_data():
    """3000 x 33 -> 65 with bias on 20-bit odd integers: y reaches 2^45, dW = dY^T X runs split-K over 3000 rows and reaches 2^51."""
    g = torch.Generator().manual_seed(64)
    t = dict(x=r64.wide_ints(g, (3000, 33), 20), W=r64.wide_ints(g, (65, 33), 20), b=r64.wide_ints(g, (65,), 20), gy=r64.wide_ints(g, (3000, 65), 20))
    r64.prove_linear64(t["x"], t["W"], t["b"], t["gy"])
    return t


def _graph_conv_data(aggr):
    """2000 sources, 3000 destinations, 33 / 17 -> 40 on 16-bit odd integers ('mean': power-of-two in-degrees); both weight gradients run split-K."""
    g = torch.Generator().manual_seed(65 + (aggr == "mean"))
    src, dst = opr.make_graph(2000, 3000, 7, "pow2" if aggr == "mean" else "random")
    t = dict(xs=r64.wide_ints(g, (2000, 33), 16), xd=r64.wide_ints(g, (3000, 17), 16), Wr=r64.wide_ints(g, (40, 33), 16), b=r64.wide_ints(g, (40,), 16),
             Wo=r64.wide_ints(g, (40, 17), 16), gy=r64.wide_ints(g, (3000, 40), 16))
    r64.prove_graph_conv64(t["xs"], t["xd"], t["Wr"], t["b"], t["Wo"], src, dst, aggr == "mean", t["gy"])
    return t, torch.stack([src, dst])


def _run_linear(t):
    leaves = {k: t[k].to(DEV).requires_grad_(True) for k in ("x", "W", "b")}
    y = ops.linear(leaves["x"], leaves["W"], leaves["b"])
    y.backward(t["gy"].to(DEV))
    return dict(y=y.detach().cpu(), **{"d" + k: v.grad.cpu() for k, v in leaves.items()})


def _run_graph_conv(t, ei, aggr):
    leaves = {k: t[k].to(DEV).requires_grad_(True) for k in ("xs", "xd", "Wr", "b", "Wo")}
    y = ops.graph_conv((leaves["xs"], leaves["xd"]), ei.to(DEV), leaves["Wr"], leaves["b"], leaves["Wo"], aggr)
    y.backward(t["gy"].to(DEV))
    return dict(y=y.detach().cpu(), **{"d" + k: v.grad.cpu() for k, v in leaves.items()})


def _default_mode_run(path):
    """What a process that never touches the compute dtype gets from the calls below on fp64 tensors (run by test_default_mode_is_untouched in a child)."""
    assert ops.get_compute_dtype() == "f32"
    res = {"linear." + k: v for k, v in _run_linear(_linear_data()).items()}
    for aggr in ("add", "mean"):
        t, ei = _graph_conv_data(aggr)
        res.update({f"{aggr}.{k}": v for k, v in _run_graph_conv(t, ei, aggr).items()})
    torch.save(res, path)


def test_linear_autograd_is_the_integer_algebra():
    _require_gpu()
    t = _linear_data()
    assert _splits(65, 33, 3000) > 1
    with ops.compute_dtype("f64"):
        leaves = {k: t[k].to(DEV).requires_grad_(True) for k in ("x", "W", "b")}
        y = ops.linear(leaves["x"], leaves["W"], leaves["b"])
    assert ops.get_compute_dtype() == "f32"
    # fp64 contiguous operands are used as they are: what the backward saved is the caller's storage
    assert y.grad_fn.saved_tensors[0].data_ptr() == leaves["x"].data_ptr() and y.grad_fn.saved_tensors[1].data_ptr() == leaves["W"].data_ptr()
    y.backward(t["gy"].to(DEV))      # OUTSIDE the block: the backward runs in its forward's arithmetic
    want = dict(y=t["x"] @ t["W"].t() + t["b"], dx=t["gy"] @ t["W"], dW=t["gy"].t() @ t["x"], db=t["gy"].sum(0))
    got = dict(y=y.detach(), dx=leaves["x"].grad, dW=leaves["W"].grad, db=leaves["b"].grad)
    assert float(want["dW"].abs().max()) > 2.0 ** 45 and not torch.equal(want["y"].float().double(), want["y"])
    bad = [f"{k}: {d}" for k in want for d in [opr.first_mismatch(got[k], want[k])] if d]
    assert all(v.dtype == torch.float64 for v in got.values()) and not bad, "\n".join(bad)
    # any other floating dtype is widened (exact) and the result comes back in the caller's dtype
    x32 = torch.randn(5, 33, device=DEV)
    with ops.compute_dtype("f64"):
        y32 = ops.linear(x32, leaves["W"].detach(), None)
    assert y32.dtype == torch.float32 and torch.equal(y32, (x32.double() @ leaves["W"].detach().t()).float())


@pytest.mark.parametrize("aggr", ["add", "mean"])
def test_graph_conv_autograd_is_the_integer_algebra(aggr):
    _require_gpu()
    t, ei = _graph_conv_data(aggr)
    assert _splits(40, 33, 3000) > 1 and _splits(40, 17, 3000) > 1
    with ops.compute_dtype("f64"):
        got = _run_graph_conv(t, ei, aggr)
    src, dst = ei[0], ei[1]
    w = (1.0 / torch.bincount(dst, minlength=3000).clamp(min=1).double())[dst] if aggr == "mean" else torch.ones(dst.numel(), dtype=torch.float64)
    agg = torch.zeros(3000, 33, dtype=torch.float64).index_add(0, dst, t["xs"][src] * w[:, None])
    gy = t["gy"]
    want = dict(y=agg @ t["Wr"].t() + t["b"] + t["xd"] @ t["Wo"].t(), dxs=torch.zeros(2000, 33, dtype=torch.float64).index_add(0, src, (gy @ t["Wr"])[dst] * w[:, None]),
                dxd=gy @ t["Wo"], dWr=gy.t() @ agg, db=gy.sum(0), dWo=gy.t() @ t["xd"])
    assert float(want["dWr"].abs().max()) > 2.0 ** 32 and not torch.equal(want["y"].float().double(), want["y"])
    bad = [f"{k}: {d}" for k in want for d in [opr.first_mismatch(got[k], want[k])] if d]
    assert not bad, "\n".join(bad)


def test_default_mode_is_untouched():
    """After this process has used the f64 mode, the default mode computes what a process that never touched the mode computes -- today's route: fp64 tensors
    cast to fp32, the fp32 kernels, the results cast back -- bit for bit, forward and every gradient of linear and of graph_conv ('add', 'mean').  The
    reference run is a fresh child process (its own GPU context, one at a time)."""
    _require_gpu()
    import tempfile
    with ops.compute_dtype("f64"):      # this process has touched the mode, and run fp64 kernels
        first = _run_linear(_linear_data())
    assert ops.get_compute_dtype() == "f32"
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "default_mode.pt")
        code = f"import sys; sys.path.insert(0, {ROOT!r}); from tests.test_ops_f64_exact_gpu import _default_mode_run; _default_mode_run({path!r})"
        subprocess.run([sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", code], check=True, cwd=ROOT, timeout=300)
        child = torch.load(path)
    here = {"linear." + k: v for k, v in _run_linear(_linear_data()).items()}
    for aggr in ("add", "mean"):
        t, ei = _graph_conv_data(aggr)
        here.update({f"{aggr}.{k}": v for k, v in _run_graph_conv(t, ei, aggr).items()})
    assert here.keys() == child.keys() and len(here) == 4 + 6 + 6
    for k in here:
        assert here[k].dtype == torch.float64 and torch.equal(here[k], child[k]), f"{k}: the default mode no longer computes what an untouched process computes"
    assert not torch.equal(here["linear.y"], first["y"]) and torch.equal(here["linear.y"].float().double(), here["linear.y"])      # (fp32 values; the f64 mode's differ)
