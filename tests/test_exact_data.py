"""The rounding-free data of tests/test_exact_gpu.py and tests/test_input_grad_exact_gpu.py, checked on the host: for every (model, batch size) the GPU
files use, check_exact proves bf16 closure, fp32 closure and coverage (tests/exact_data.py), for the second file also input-gradient closure and
coverage -- and the comparison the GPU files rely on flags a single-ulp change."""
import pytest
import torch

from tests import exact_data as xd
from tests import helpers
from tests import test_exact_gpu as gx
from tests import test_input_grad_exact_gpu as igx

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



@pytest.mark.parametrize("model,B", sorted(set(igx.CASES)))
def test_input_grad_case_is_rounding_free_and_covering(model, B):
    """(a)-(d) for every (model, batch) of tests/test_input_grad_exact_gpu.py, whose GPU references are the oracle alone."""
    spec, case = igx.exact_case(model, B)
    stats = {}
    ref = xd.check_exact(spec, case, stats=stats, input_grads=True)
    assert 0 < stats["xgrad_sum_bound"] <= 1.0
    _, need = spec.node_liveness()
    for t in spec.node_types:      # a non-zero dx only where the encoder computes the node
        dx = ref["xgrads"][t].view(B, spec.num_nodes[t], -1)
        assert set(i for i in range(spec.num_nodes[t]) if float(dx[:, i].abs().max()) > 0) <= set(need[0][t]), t


def test_enc_cover_changes_nothing_but_the_input_gradient():
    """The dense encoder columns of enc_cover multiply zero inputs: output, hidden states and parameter gradients are the plain case's."""
    spec = helpers.make_spec(*gx.MODELS["a1c2_L3"]["spec"])
    plain = xd.exact_case(spec, 17, gx.SEED, **gx.MODELS["a1c2_L3"]["knobs"])
    cover = xd.exact_case(spec, 17, gx.SEED, enc_cover=True, **gx.MODELS["a1c2_L3"]["knobs"])
    rp, rc = (xd.reference(spec, c, c["gout_mse"], input_grads=True) for c in (plain, cover))
    assert torch.equal(rp["out"], rc["out"]) and all(torch.equal(a, b) for a, b in zip(rp["hidden"], rc["hidden"]))
    for k in rp["grads"]:      # (the encoder weights' gradient differs only in the columns whose inputs enc_cover zeroes)
        keep = slice(None) if not k.startswith("encoder.lins.") or not k.endswith(".weight") else (cover["x"][k.split(".")[2]] != 0).any(0)
        assert torch.equal(rp["grads"][k][..., keep], rc["grads"][k][..., keep]), k
    W = cover["params"]["encoder.lins.base.weight"]
    assert int((W != 0).any(0).sum()) > int((plain["params"]["encoder.lins.base.weight"] != 0).any(0).sum())
