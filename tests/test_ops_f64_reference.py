"""Host tests of tests/ops_f64_reference.py, the checkers of tests/test_ops_f64_exact_gpu.py (no GPU):
  (a) the references are what they claim: on the exact families fp64 matmul equals int64 matmul (small shapes: int64 matmul is slow), and torch's own fp64
      CPU matmul / index_add / column sum passes the checker of every random-data case -- the bound is not too tight for a correct implementation;
  (b) negative controls, for every case of the GPU matrix: operands rounded to fp32, accumulation in fp32, one dropped k, a dropped last K tile, a dropped
      split-K partial, bias added twice, a stale element, a shifted row tile (aggregation: a dropped edge, an edge scale rounded to fp32; column sums: a
      dropped row, a dropped block) are REJECTED.  A GPU case runs on every family of its shape, so a damage counts as rejected when it is a different
      result on at least one exact family (bit equality sees any difference) -- and, where the shape also runs random data, it must ALSO lie outside the
      bound there.  A damage that no family of a shape can tell from the right result fails here: a defect of the case, not of the variant;
  (c) the fp32 kernels' results are rejected: torch's fp32 matmul of the same operands fails every case with K >= 1.
"""
import pytest
import torch

from tests import ops_f64_reference as r64
from tests import ops_reference as opr

SHAPES = r64.all_gemm_shapes()
SMALL = [c for c in SHAPES if c[0] * c[1] * max(c[2], 1) <= 200000]
LARGE = [c for c in SHAPES if c[0] * c[1] * max(c[2], 1) > 200000]


def _police_gemm(M, N, K, splits):
    fams = r64.families_of(M, N, K)
    for bias, acc in opr.gemm_variants():
        seen = set()
        for fam in fams:
            case = r64.gemm_case(M, N, K, fam, bias=bias, accumulate=acc, splits=splits)
            where = opr.gemm_where(K, splits)
            ok = case["A"] @ case["B"].t()
            if bias:
                ok = ok + case["bias"]
            if acc:
                ok = ok + case["C_in"]
            assert r64.gemm_failure(case, ok, where) is None, (M, N, K, fam, bias, acc, r64.gemm_failure(case, ok, where))
            if K >= 1:      # (c) what the fp32 operator computes from the same operands
                f32 = (case["A"].float() @ case["B"].float().t()).double()
                f32 = f32 + (case["bias"] if bias else 0.0) + (case["C_in"] if acc else 0.0)
                assert r64.gemm_failure(case, f32, where) is not None, f"gemm {fam} {M} x {N} x {K}: the checker accepts an fp32 product"
            for kind in r64.GEMM_DAMAGES:
                bad = r64.damaged_gemm64(case, kind)
                if bad is None:
                    continue
                assert r64.gemm_failure(case, bad, where) is not None, f"gemm {fam} {M} x {N} x {K} bias={bias} accumulate={acc}: the checker accepts '{kind}'"
                if case["exact"]:
                    seen.add(kind)
        want = set() if (K == 0 and acc and not bias) else {"stale_element"}      # (C (+)= nothing: the stale C_in IS the result)
        if bias:
            want.add("bias_twice")
        if K >= 1:      # (K == 0: the result is bias + C_in, integers below 2^21 -- fp32 values, nothing for an fp32 accumulator to lose)
            want |= {"drop_one_k", "drop_last_k_tile", "operands_f32", "accumulate_f32"}
            if M >= 2 and N * K >= 15:
                want.add("shift_row_tile")
        if splits > 1:
            want.add("drop_split_partial")
        assert want <= seen, f"gemm {M} x {N} x {K} bias={bias} accumulate={acc}: no exact family can tell {sorted(want - seen)} from the right result"


def test_gemm_small_shapes_every_damage_is_rejected():
    for c in SMALL:
        _police_gemm(*c)


@pytest.mark.parametrize("shape", LARGE, ids=lambda c: f"{c[0]}x{c[1]}x{c[2]}-s{c[3]}")
def test_gemm_shape_every_damage_is_rejected(shape):
    _police_gemm(*shape)


def test_exact_families_agree_with_int64_matmul():
    """The expected values of the exact families come from fp64 matmul, which cannot round on data that closes; here against int64 arithmetic."""
    for M, N, K, s in SMALL[::7] + [(65, 33, 2500, 4), (64, 64, 3000, 5)]:
        for fam in ("wide_sum", "wide_operand"):
            Ai, Bi, bi, Ci, e = r64._gemm_base(M, N, K, 1, fam)
            case = r64.gemm_case(M, N, K, fam, bias=True, accumulate=True, splits=s)
            want = Ai @ Bi.t() + bi + Ci
            assert int(want.abs().max()) < 2 ** 53 and torch.equal(case["ref"], want.double()) and torch.equal(case["ref"].long(), want), (M, N, K, fam)


def test_the_families_are_what_their_description_says():
    A, B, bias, C, _ = r64._gemm_base(33, 31, 900, 1, "wide_sum")
    R = r64.wide_sum_range(900)
    assert R == 2 ** 20 and int(A.abs().max()) <= R and int(A.abs().min()) >= R // 2 and bool((A % 2 == 1).all())
    assert r64.wide_sum_range(131073) ** 2 * 131073 <= 2 ** 52 < (r64.wide_sum_range(131073) + 1) ** 2 * 131073
    case = r64.gemm_case(33, 31, 900, "wide_sum")
    assert float(case["ref"].abs().min()) > 2.0 ** 24 and not torch.equal(case["ref"].float().double(), case["ref"])
    assert torch.equal(case["A"].float().double(), case["A"])      # fp32 operands: this family polices the accumulator, not the operands
    A, B, _, _, _ = r64._gemm_base(33, 31, 900, 1, "wide_operand")
    assert int(A.abs().min()) >= 2 ** 25 and int(A.abs().max()) < 2 ** 26 and bool(((B != 0).sum(1) == 1).all())
    assert not bool((A.double().float().double() == A.double()).any())      # 26 significant bits: no element is an fp32 value
    A, B, _, _, e = r64._gemm_base(65, 33, 2048, 1, "random")
    assert e == -20 and int(A.abs().max()) < 2 ** 25
    # the error of a result is taken against the unrounded reference: a result one ulp off an exactly representable reference shows as that ulp
    hi, lo = torch.tensor([3.0 * 2 ** 20], dtype=torch.float64), torch.tensor([0.0], dtype=torch.float64)
    assert float(r64.dyadic_error(torch.tensor([3.0 + 2.0 ** -51], dtype=torch.float64), hi, lo)) == 2.0 ** -51
    assert float(r64.dyadic_error(torch.tensor([3.0], dtype=torch.float64), hi, torch.tensor([1.0], dtype=torch.float64))) == -2.0 ** -40


def test_split_k_counts_are_the_fp32_operators():
    """mshgnn_op_gemm_f64_workspace defers to mshgnn_op_gemm_workspace's rule; the chunk length the damage uses is the launch's."""
    assert r64.kchunk(70000, 136) == 528 and r64.kchunk(3000, 5) == 608 and r64.kchunk(1, 1) == 16
    assert (65, 33, 2500, 4) in r64.GEMM_RANDOM and 2500 <= r64.RANDOM_MAX_K


_AGG_IDS = lambda kw: f"{kw['n_rows']}x{kw['width']}-{'exact' if kw['exact'] else 'random'}-{'mean' if kw['mean'] else kw['scale']}-hub{kw.get('hub', 0)}"


@pytest.mark.parametrize("kw", r64.all_aggregate_cases(), ids=_AGG_IDS)
def test_aggregate_case_torch_passes_and_every_damage_is_rejected(kw):
    case = r64.aggregate_case64(**kw)
    rows = torch.repeat_interleave(torch.arange(case["n_rows"]), (case["rowptr"][1:] - case["rowptr"][:-1]).long())
    msg = case["x"][case["col"].long()]
    if case["scale"] is not None:      # the kernels' order: scale every edge, then sum
        msg = msg * case["scale"][:, None]
    got = torch.zeros(case["n_rows"], case["width"], dtype=torch.float64).index_add(0, rows, msg)
    assert not opr.reject(case["ref"], case["bound"], got), kw
    applied = set()
    for kind in r64.AGG_DAMAGES:
        bad = r64.damaged_aggregate64(case, kind)
        if bad is None:
            continue
        applied.add(kind)
        assert opr.reject(case["ref"], case["bound"], bad), f"aggregate {kw}: the checker accepts '{kind}'"
    assert "stale_element" in applied
    if int(case["deg"].sum()) > 0:
        if kw["exact"]:      # (a sum of dyadic 26-bit values may happen to be an fp32 value; every shape also runs the wide data)
            assert "accumulate_f32" in applied, kw
        if case["width"] >= 31:
            assert "drop_one_edge" in applied, kw
        if kw["scale"] == "wide" or (kw["mean"] and bool((case["deg"] & (case["deg"] - 1) != 0).any())):
            assert "scale_f32" in applied, kw
    if kw.get("hub"):
        assert int(case["deg"][0]) == kw["hub"] and case["exact"]


@pytest.mark.parametrize("M,N,wide", r64.all_colsum_cases())
def test_colsum_case_torch_passes_and_every_damage_is_rejected(M, N, wide):
    case = r64.colsum_case64(M, N, wide=wide)
    assert not opr.reject(case["ref"], None, case["X"].sum(0)) and not opr.reject(case["ref"], None, case["X"].flip(0).sum(0)), (M, N)
    applied = set()
    for kind in r64.COLSUM_DAMAGES:
        bad = r64.damaged_colsum64(case, kind)
        if bad is None:
            continue
        applied.add(kind)
        assert opr.reject(case["ref"], None, bad), f"colsum {M} x {N}: the checker accepts '{kind}'"
    assert "stale_element" in applied and (M < 1 or "drop_one_row" in applied) and (M < 511 or "drop_last_block" in applied)
    if M >= 1 and wide:      # (a sum of dyadic 26-bit values may happen to be an fp32 value; every shape also runs the wide data)
        assert "accumulate_f32" in applied, (M, N, wide)      # no fp32 accumulator holds these column sums


def test_a_case_that_does_not_close_is_refused():
    with pytest.raises(opr.DoesNotClose):
        r64._require_closure(torch.tensor([2.0 ** 53]), 0, "a sum that reaches 2^53")
    with pytest.raises(opr.DoesNotClose):
        r64._require_closure(torch.tensor([2.0 ** 33]), -20, "2^53 units of 2^-20")
    assert r64._require_closure(torch.tensor([2.0 ** 53 - 1], dtype=torch.float64), 0, "the largest sum that closes") < 1.0
    assert abs(float(r64.gamma(1)) - 2.0 ** -53) < 1e-30
