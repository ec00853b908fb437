"""The rounding-free data of tests/test_exact_gpu.py, checked on the host: for every (model, batch size) the GPU file uses, check_exact proves bf16 closure,
fp32 closure and coverage (tests/exact_data.py) -- and the comparison the GPU file relies on flags a single-ulp change."""
import pytest
import torch

from tests import exact_data as xd
from tests import test_exact_gpu as gx

CASES = sorted({("a1c2_L3", B) for B in gx.BATCHES + gx.TWO_CALL_BATCHES + [200]} | set(gx.WIDE_CASES) | {("a1c2_h200_L3", B) for B in gx.PADDED_BATCHES}
               | {("mck4_cls_L3", B) for B in gx.CLS_BATCHES})


@pytest.mark.parametrize("model,B", CASES)
def test_exact_case_is_rounding_free_and_covering(model, B):
    spec, case, ref, stats = gx._reference.__wrapped__(model, B)
    assert stats["nonzero_gout"] > 0 and stats["zero_decisions"] > 0
    assert stats["fwd_sum_bound"] <= 1.0 and stats["bwd_sum_bound"] <= 1.0
    if spec.regression:      # the loss reference is the mean of squares over the chosen targets
        assert float(((ref["out"] - case["y"]) ** 2).mean()) == ref["loss"]


def test_comparison_flags_a_single_ulp():
    ref = torch.tensor([0.0, 1.5, -2.0 ** -14, 3.0], dtype=torch.float64)
    assert xd.first_difference(ref.float(), ref) is None
    assert xd.first_difference(torch.tensor([-0.0, 1.5, -2.0 ** -14, 3.0]), ref) is None      # -0.0 == 0.0
    for i in range(4):
        got = ref.float().clone()
        got[i] = torch.nextafter(got[i], torch.tensor(float("inf")))
        d = xd.first_difference(got, ref)
        assert d is not None and d.startswith("1 of 4") and f"({i},)" in d, d
    got = ref.to(torch.bfloat16).clone()
    got[1] = 1.5 - 2.0 ** -7      # one bf16 ulp below 1.5
    assert xd.first_difference(got, ref) is not None


def test_check_exact_refuses_a_rounding_case():
    """A case whose values do not close (inputs of a non-dyadic scale) is refused before it can be used as an exact reference."""
    import bench
    spec = bench.build_spec(3, "a1c2")
    case = xd.exact_case(spec, 4, 1, rel_scales=(1.0,))
    case["x"] = {t: v / 3.0 for t, v in case["x"].items()}
    case["y"] = None
    with pytest.raises(AssertionError):
        xd.check_exact(spec, case, gout=case["gout"])

