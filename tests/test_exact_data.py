"""The rounding-free data of tests/test_exact_gpu.py, tests/test_exact_families_gpu.py and tests/test_input_grad_exact_gpu.py, checked on the host: for
every (model, batch size) the GPU files use, check_exact proves bf16 closure, fp32 closure and coverage (tests/exact_data.py), for the last file also
input-gradient closure and coverage; the families' cases have the live base nodes their names claim, with non-zero gradients on the base paths -- and the
comparison the GPU files rely on flags a single-ulp change, and a single wrong element of a base row or of a base-path gradient."""
import pytest
import torch

from tests import exact_data as xd
from tests import helpers
from tests import test_exact_families_gpu as fam
from tests import test_exact_gpu as gx
from tests import test_input_grad_exact_gpu as igx
from tests import ops_reference as opr
from tests import test_ops_exact_gpu as opx

CASES = sorted({("a1c2_L3", B) for B in gx.BATCHES + gx.TWO_CALL_BATCHES + [200]} | set(gx.WIDE_CASES) | {("a1c2_h200_L3", B) for B in gx.PADDED_BATCHES}
               | {("mck4_cls_L3", B) for B in gx.CLS_BATCHES}) + fam.CASES


@pytest.mark.parametrize("model,B", CASES)
def test_exact_case_is_rounding_free_and_covering(model, B):
    spec, case, ref, stats = gx._reference.__wrapped__(model, B)
    assert stats["nonzero_gout"] > 0 and stats["zero_decisions"] > 0
    assert stats["fwd_sum_bound"] <= 1.0 and stats["bwd_sum_bound"] <= 1.0
    if spec.regression:      # the loss reference is the mean of squares over the chosen targets
        assert float(((ref["out"] - case["y"]) ** 2).mean()) == ref["loss"]
    if model in fam.FAMILIES:
        _check_live_base(model, spec, ref)


def _base_path_tensors(spec):
    """base_transform.*, every tensor of a relation into a base node, and the relation weight of one out of a base node (the root weight and the bias of a
    relation act on its destination)."""
    return [k for k in spec.param_shapes() if k.startswith("base_transform.") or "___base>" in k or ("<base___" in k and k.endswith("lin_rel.weight"))]


def _check_live_base(model, spec, ref):
    """What the family is in the matrix for: the encoder computes base nodes (every family but MiniCheetah-K4 regression at 3 layers, whose base is dead
    as at every 3-layer GRF model), the base is a destination where the name says so, and every base-path tensor the oracle gives a gradient on random
    data has a non-zero one here.  Coverage (c) implies the last; it is stated per family so that a change of knobs cannot go back to a dead base."""
    live, need = spec.node_liveness()
    dest = model.replace("_h256", "") in fam.BASE_IS_A_DESTINATION
    assert bool(need[0]["base"]) == (model != "mck4_reg_L3"), (model, need[0]["base"])
    if dest:
        assert any(live[l]["base"] for l in range(spec.num_layers)), model
    else:
        assert not any(live[l]["base"] for l in range(spec.num_layers)), model
    live_random = xd._live_nonzero_in_random_case(spec)
    base_live = [k for k in _base_path_tensors(spec) if k in live_random]
    assert bool(base_live) == bool(need[0]["base"]), model
    if dest:
        assert any("___base>" in k for k in base_live) and (not spec.has_base_transform or "base_transform.0.weight" in base_live), model
    for k in base_live:
        assert float(ref["grads"][k].abs().max()) > 0, f"{model}: {k} is live on random data and zero here"


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


@pytest.mark.parametrize("model", fam.BASE_IS_A_DESTINATION)
def test_comparison_flags_one_element_of_the_base_destination_path(model):
    """The comparisons of the GPU files, given the oracle's own reference with one element negated as "got": one element of a base row of X_1 (what a layer
    with the base as a destination wrote), and one element of a gradient only that path feeds (base_transform.0.weight, on MI-HGNN a relation weight into
    base).  Both must be reported, and nothing else: the family cases look at the base path."""
    B = 17
    spec, case, ref, _ = gx._reference.__wrapped__(model, B)
    sl = helpers.node_slices(spec)
    live, _ = spec.node_liveness()
    assert live[0]["base"], model

    class Got:      # (an engine whose stash holds the perturbed hidden states)
        def __init__(self, hidden):
            self.hidden = hidden

        def hidden_state(self, B, l):
            return self.hidden[l]

    bad = []
    gx._compare_hidden(bad, "ref", Got(ref["hidden"]), spec, ref, B, range(spec.num_layers + 1))
    assert not bad
    node = sl["base"].start + live[0]["base"][0]
    row = ref["hidden"][1][:, node]
    w, f = (int(i) for i in (row != 0).nonzero()[0])
    hidden = [h.clone() for h in ref["hidden"]]
    hidden[1][w, node, f] = -hidden[1][w, node, f]
    gx._compare_hidden(bad, "negated", Got(hidden), spec, ref, B, range(spec.num_layers + 1))
    assert len(bad) == 1 and "X1[base]" in bad[0] and "1 of " in bad[0] and f"window {w} (tile {w // 16}), node {node}, feature {f} " in bad[0], bad

    key = "base_transform.0.weight" if spec.has_base_transform else next(k for k in ref["grads"] if "___base>" in k and k.endswith("lin_rel.weight")
                                                                         and float(ref["grads"][k].abs().max()) > 0)
    offs = spec.param_offsets()
    flat = torch.zeros(spec.flat_size(), dtype=torch.float32)
    for k, (off, n) in offs.items():
        flat[off:off + n] = ref["grads"][k].reshape(-1).float()
    bad = []
    gx._compare_grads(bad, "ref", spec, flat, ref)
    assert not bad
    i = int((ref["grads"][key].reshape(-1) != 0).nonzero()[0])
    flat[offs[key][0] + i] = -flat[offs[key][0] + i]
    gx._compare_grads(bad, "negated", spec, flat, ref)
    assert len(bad) == 1 and f"grad {key}:" in bad[0] and "1 of " in bad[0], bad


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


@pytest.mark.parametrize("model,B", opx.MODEL_CASES)
def test_operator_path_case_closes_in_the_operator_algebra(model, B):
    """check_exact proves fp32 closure for the FUSED algebra (root weights pre-summed per destination type).  The operator-by-operator path
    (models._forward_operators, tests/test_ops_exact_gpu.py) adds the same terms grouped per relation, so its sums of |terms| are larger: for exactly the
    (family, batch, seed) triples that file runs, every Linear / GraphConv call proves, for its forward product(s), its aggregation and each of its backward
    GEMMs and column sums, sum |terms| < 2^24 units of the terms' finest dyadic grid (ops_reference.operator_algebra raises otherwise) -- and the restated
    algebra gives the oracle's output and gradients bit for bit, so it is the right algebra."""
    spec, case, ref, _ = gx._reference.__wrapped__(model, B)
    out, grads, worst = opr.operator_algebra(spec, case["params"], case["x"], spec.topology.edge_index_dict(B), B, ref["gout"])
    assert torch.equal(out, ref["out"])
    for k, r in ref["grads"].items():
        g = grads[k] if grads[k] is not None else torch.zeros_like(r)
        assert torch.equal(g, r), k
    # (a call whose result cannot reach the output -- the last layer's relations into the other types -- has no backward and needs no proof: nothing compared
    #  depends on it; every layer has calls that do)
    assert "decoder" in worst and all(any(k.startswith(f"layer {l} ") for k in worst) for l in range(spec.num_layers)) and any(k.startswith("encoder.") for k in worst)
    top = max(max(w.values()) for w in worst.values())
    assert 0 < top < 1.0
    print(f"\n{model} B={B}: {len(worst)} operator calls, largest sum of |terms| {top:.2e} of the fp32 limit")
