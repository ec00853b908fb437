"""Host tests of tests/ops_reference.py, the checkers of tests/test_ops_exact_gpu.py (no GPU):
  (a) torch's own fp32 CPU matmul / index_add / column sum passes the checker of every case of the GPU tables -- bit equality on exact data, the derived
      per-element bound on random data -- so the checkers are not too tight for a correct implementation;
  (b) negative controls: for every case of the GPU tables, every damaged result ops_reference can build for it (one K element dropped from one output,
      the last K tile dropped, a 64-row tile shifted by one row, the bias added twice, one edge dropped from the busiest destination, a stale element,
      a dropped row / 512-row block of a column sum) is REJECTED by the checker that case uses.  No case is exempt: a random-data case whose bound cannot
      see a dropped term fails here and has to become an exact-data case (that is why 70000-row column sums and the 100000-edge destination are exact
      only);
  (c) a case that does not close in fp32 is refused, never rescaled; the bound itself (gamma_n, zero bounds, NaN) behaves as documented.
"""
import pytest
import torch

from tests import ops_reference as opr


def _variants(exact):
    return opr.gemm_variants()


def _gemm_ids(c):
    return f"{c[0]}x{c[1]}x{c[2]}-{'exact' if c[3] else 'random'}-s{c[4]}"


GEMM_CASES = opr.all_gemm_cases()
SMALL = [c for c in GEMM_CASES if c[0] * c[1] * c[2] <= 200000]
LARGE = [c for c in GEMM_CASES if c[0] * c[1] * c[2] > 200000]


def _police_gemm(M, N, K, exact, splits):
    applied = set()
    for bias, acc in opr.gemm_variants():
        case = opr.gemm_operands(M, N, K, exact=exact, bias=bias, accumulate=acc, splits=splits)
        where = opr.gemm_where(K, splits)
        # (a) torch's fp32 matmul on the CPU
        got = case["A"] @ case["B"].t()
        if bias:
            got = got + case["bias"]
        if acc:
            got = got + case["C_in"]
        assert not opr.reject(case["ref"], case["bound"], got, where), (M, N, K, bias, acc, opr.within_bound(got, case["ref"], case["bound"] if case["bound"] is not None else torch.tensor(0.0), where))
        # (b) every damage is rejected
        for kind in opr.GEMM_DAMAGES:
            bad = opr.damaged_gemm(case, kind)
            if bad is None:
                continue
            applied.add(kind)
            assert opr.reject(case["ref"], case["bound"], bad, where), f"gemm {M} x {N} x {K} bias={bias} accumulate={acc}: the checker accepts '{kind}'"
    assert "stale_element" in applied and "bias_twice" in applied
    if K >= 1:
        assert "drop_one_k" in applied and "drop_last_k_tile" in applied, (M, N, K, applied)
        if M >= 2 and N * K >= 15:      # (two rows of a 2 x 1 x 1 product may be equal: shifting them is no damage)
            assert "shift_row_tile" in applied, (M, N, K, applied)


def test_gemm_small_cases_torch_passes_and_every_damage_is_rejected():
    for c in SMALL:
        _police_gemm(*c)


@pytest.mark.parametrize("case", LARGE, ids=_gemm_ids)
def test_gemm_case_torch_passes_and_every_damage_is_rejected(case):
    _police_gemm(*case)


def test_split_k_table_matches_the_documented_rule():
    """The splits each split-K case is named for, against the rule stated in the issue / csrc/mshgnn_ops.hip -- restated here once, so that a typo in the
    hand-worked table does not go to the GPU."""
    for (M, N), ks in opr.GEMM_SPLITK.items():
        tiles = -(-M // 64) * -(-N // 64)
        for K, s in ks.items():
            want = min(-(-1024 // tiles), K // 512, 256) if tiles < 512 and K >= 2048 else 1
            assert s == max(1, want), (M, N, K, s, want)
    # the named sub-cases exist: one split next to four, a chunk that ends inside a K tile, empty trailing chunks, the 256 cap
    assert opr.GEMM_SPLITK[(1, 1)][2047] == 1 and opr.GEMM_SPLITK[(1, 1)][2048] == 4 and opr.GEMM_SPLITK[(1, 1)][131073] == 256
    kchunk = (-(-70000 // 136) + 15) // 16 * 16
    assert kchunk == 528 and 133 * kchunk > 70000 and 132 * kchunk < 70000
    assert (-(-3000 // 5) + 15) // 16 * 16 == 608 and 3000 % 608 % 16 != 0


@pytest.mark.parametrize("kw", opr.all_aggregate_cases(), ids=lambda kw: f"{kw['n_rows']}x{kw['width']}-{'exact' if kw['exact'] else 'random'}-{'mean' if kw['mean'] else kw['scale']}-hub{kw.get('hub', 0)}")
def test_aggregate_case_torch_passes_and_every_damage_is_rejected(kw):
    case = opr.aggregate_case(**kw)
    x, rows = case["x"], torch.repeat_interleave(torch.arange(case["n_rows"]), (case["rowptr"][1:] - case["rowptr"][:-1]).long())
    msg = x[case["col"].long()]
    if case["scale"] is not None and not case["mean"]:
        msg = msg * case["scale"][:, None]
    got = torch.zeros(case["n_rows"], case["width"]).index_add(0, rows, msg)
    if case["mean"]:
        got = got / case["deg"].clamp(min=1).float()[:, None]      # PyG's order: sum, then divide
    assert not opr.reject(case["ref"], case["bound"], got), kw
    if case["mean"]:      # ... and the kernels' order: scale every edge by fl32(1 / deg), then sum
        got2 = torch.zeros(case["n_rows"], case["width"]).index_add(0, rows, x[case["col"].long()] * case["scale"][:, None])
        assert not opr.reject(case["ref"], case["bound"], got2), kw
    applied = set()
    for kind in opr.AGG_DAMAGES:
        bad = opr.damaged_aggregate(case, kind)
        if bad is None:
            continue
        applied.add(kind)
        assert opr.reject(case["ref"], case["bound"], bad), f"aggregate {kw}: the checker accepts '{kind}'"
    assert "stale_element" in applied
    if case["width"] >= 31 and int(case["deg"].sum()) > 0:
        assert "drop_one_edge" in applied, kw
    if kw.get("hub"):
        assert int(case["deg"][0]) == kw["hub"] and case["exact"]


@pytest.mark.parametrize("M,N,exact", opr.all_colsum_cases())
def test_colsum_case_torch_passes_and_every_damage_is_rejected(M, N, exact):
    case = opr.colsum_case(M, N, exact=exact)
    assert not opr.reject(case["ref"], case["bound"], case["X"].sum(0)), (M, N)
    applied = set()
    for kind in opr.COLSUM_DAMAGES:
        bad = opr.damaged_colsum(case, kind)
        if bad is None:
            continue
        applied.add(kind)
        assert opr.reject(case["ref"], case["bound"], bad), f"colsum {M} x {N}: the checker accepts '{kind}'"
    assert "stale_element" in applied and (M < 511 or {"drop_one_row", "drop_last_block"} <= applied)


def test_the_bound_cannot_police_long_random_reductions_which_is_why_they_are_exact():
    """The choice the tables make, shown rather than asserted away: on random data a dropped row of a 70000-row column sum stays inside gamma_M sum |x|."""
    case = opr.colsum_case(70000, 257, exact=False)
    assert not opr.reject(case["ref"], case["bound"], opr.damaged_colsum(case, "drop_one_row"))
    assert (70000, 257, False) not in opr.all_colsum_cases() and (70000, 257, True) in opr.all_colsum_cases()
    assert float(opr.gamma(131073 + 256)) > 7e-3


def test_a_case_that_does_not_close_is_refused():
    with pytest.raises(opr.DoesNotClose):
        opr._require_closure(torch.tensor([2.0 ** 24]), 0, "a sum that reaches 2^24")
    with pytest.raises(opr.DoesNotClose):
        opr._require_closure(torch.tensor([2.0 ** 21]), -3, "2^24 units of 2^-3")
    assert opr._require_closure(torch.tensor([2.0 ** 24 - 1]), 0, "the largest sum that closes") < 1.0
    opr._gemm_base.cache_clear()
    real = opr._ints
    try:      # entries of +-4096: the sum of a 4 x 4 x 8 product reaches 2^24 already
        opr._ints = lambda g, shape, lo=-4096, hi=4096: torch.full(shape, 4096.0)
        with pytest.raises(opr.DoesNotClose):
            opr.exact_operands(4, 4, 8, seed=99)
    finally:
        opr._ints = real
        opr._gemm_base.cache_clear()


def test_bound_semantics():
    ref = torch.tensor([[0.0, 1.0, -2.0]], dtype=torch.float64)
    bound = torch.tensor([[0.0, 1e-6, 1e-6]], dtype=torch.float64)
    assert opr.within_bound(torch.tensor([[0.0, 1.0 + 5e-7, -2.0]]), ref, bound) is None
    assert opr.within_bound(torch.tensor([[-0.0, 1.0, -2.0]]), ref, bound) is None
    d = opr.within_bound(torch.tensor([[1e-30, 1.0, -2.0]]), ref, bound)                  # a zero bound means exactly zero
    assert d is not None and "(0, 0)" in d
    assert opr.within_bound(torch.tensor([[0.0, float("nan"), -2.0]]), ref, bound) is not None
    assert opr.within_bound(torch.tensor([[0.0, 1.0, -2.0 - 3e-6]]), ref, bound) is not None
    assert opr.first_mismatch(torch.tensor([[0.0, 1.0, -2.0]]), ref) is None
    d = opr.first_mismatch(torch.tensor([[0.0, 1.0000001, -2.0]]), ref, opr.gemm_where(33, 1))
    assert d is not None and "(0, 1)" in d and "tile (0, 0)" in d and "last one 1 wide" in d
    assert abs(float(opr.gamma(1)) - 2.0 ** -24) < 1e-14 and float(opr.gamma(torch.tensor([2, 4]))[1]) > 4 * 2.0 ** -24
    # the bound of a GEMM is per element: a row of zeros in A gives zero bounds in that row of C
    b = opr.elementwise_bound(torch.tensor([[0.0, 0.0], [1.0, 2.0]]), torch.tensor([[3.0, 4.0]]), 2)
    assert float(b[0, 0]) == 0.0 and float(b[1, 0]) == float(opr.gamma(2)) * 11.0
