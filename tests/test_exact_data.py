"""The rounding-free data of tests/test_exact_gpu.py, tests/test_exact_families_gpu.py and tests/test_input_grad_exact_gpu.py, checked on the host: for
every (model, batch size) the GPU files use, check_exact proves bf16 closure, fp32 closure and coverage (tests/exact_data.py), for the last file also
input-gradient closure and coverage; the families' cases have the live base nodes their names claim, with non-zero gradients on the base paths -- and the
comparison the GPU files rely on flags a single-ulp change, and a single wrong element of a base row or of a base-path gradient.
For tests/test_exact_generic_gpu.py (the generic-width engine) also: every aggregate the engine stages as one operand row is a bf16 value, the base node of
a many-limb model is a live destination of as many rows as its name says, the random topologies hold a repeated edge, an empty relation and a node without
in-edges -- and the comparison flags one dropped row of a long sum, a repeated edge counted once and a mean scaled by the wrong degree.
For tests/test_exact_ce_gpu.py (the fused cross-entropy steps): every (model, batch, seed, wrong share) closes with the softmax gradient the kernels' fp32 formula
gives, covers both labels per foot and every regime (tie, right, wrong) it declares -- and what a subtly wrong cross-entropy tail would compute changes a gradient."""
import pytest
import torch

from tests import exact_data as xd
from tests import helpers
from tests import test_exact_ce_gpu as cex
from tests import test_exact_families_gpu as fam
from tests import test_exact_generic_gpu as gen
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


# ---------------------------------------------------------------------------------------------------
# the generic-width engine's cases (tests/test_exact_generic_gpu.py)
# ---------------------------------------------------------------------------------------------------
def _edges_into(spec, t):
    return [(et, j, i) for et in spec.edge_types if et[2] == t for j, i in spec.topology.edges(et)]


@pytest.mark.parametrize("model,B", gen.CASES)
def test_generic_engine_case_is_rounding_free_and_covering(model, B):
    """(a)-(c) for every (model, batch, seed) of tests/test_exact_generic_gpu.py; and what check_exact does not ask of the LDS-resident kernels' cases: the
    generic engine stages a relation's aggregate (forward: the sum or mean of a destination's source rows; backward: of a source's destinations' dH rows)
    as one operand row in the plan's storage, so every such sum of a live destination must itself be a bf16 value."""
    spec, case, ref, stats = gx._reference.__wrapped__(model, B)
    assert stats["nonzero_gout"] > 0 and stats["zero_decisions"] > 0
    assert stats["fwd_sum_bound"] <= 1.0 and stats["bwd_sum_bound"] <= 1.0
    assert stats["aggregates_not_bf16"] == [], stats["aggregates_not_bf16"][:5]
    if spec.regression:
        assert float(((ref["out"] - case["y"]) ** 2).mean()) == ref["loss"]
    if model in gen.LIMBS:      # the base node is a live destination of as many rows as the name says, and the paths through it carry gradient
        live, need = spec.node_liveness()
        assert live[0]["base"] == [0] and need[0]["base"] == [0], model
        into = _edges_into(spec, "base")
        assert len(into) == gen.LIMBS[model] and len({j for _, j, _ in into}) == gen.LIMBS[model] and {et for et, _, _ in into} == {("joint", "connect", "base")}
        assert len([1 for et in spec.edge_types if et[0] == "base" for j, _ in spec.topology.edges(et)]) == gen.LIMBS[model]      # (the backward sum's rows)
        for k in ("convs.0.convs.<joint___connect___base>.lin_rel.weight", "convs.1.convs.<base___connect___joint>.lin_rel.weight", "encoder.lins.base.weight"):
            assert float(ref["grads"][k].abs().max()) > 0, f"{model}: {k} has a zero gradient"


def test_random_topology_cases_hold_what_no_robot_has():
    """Between them the random topologies of the GPU file have a repeated edge INTO A LIVE NODE (one the plan computes: a repeated edge elsewhere changes
    nothing that is compared), an empty relation, and a live node without in-edges."""
    seen = set()
    for model, B in gen.RANDOM_CASES:
        spec = gx._spec(model)
        live, _ = spec.node_liveness()
        for et in spec.edge_types:
            e = [tuple(p) for p in spec.topology.edges(et)]
            if not e:
                seen.add("an empty relation")
            if any(e.count(p) > 1 and any(p[1] in live[l][et[2]] for l in range(spec.num_layers)) for p in e):
                seen.add("a repeated edge into a live node")
        for t in spec.node_types:
            fed = {i for _, _, i in _edges_into(spec, t)}
            if any(set(live[l][t]) - fed for l in range(spec.num_layers)):
                seen.add("a live node without in-edges")
    assert seen == {"an empty relation", "a repeated edge into a live node", "a live node without in-edges"}, seen


class _Stash:      # (an engine whose stash holds given hidden states)
    def __init__(self, hidden):
        self.hidden = hidden

    def hidden_state(self, B, l):
        return self.hidden[l]


def _flagged(spec, ref, B, got):
    """What the GPU files' comparisons report when `got` (a reference of another model: out, hidden, grads) stands in for an engine's results."""
    bad_h, bad_g = [], []
    gx._compare_hidden(bad_h, "got", _Stash([h.double() for h in got["hidden"]]), spec, ref, B, range(spec.num_layers + 1))
    offs = spec.param_offsets()
    flat = torch.zeros(spec.flat_size(), dtype=torch.float64)
    for k, (off, n) in offs.items():
        flat[off:off + n] = got["grads"][k].reshape(-1)
    gx._compare_grads(bad_g, "got", spec, flat, ref)
    return bad_h, bad_g


def _without_edge(spec, et, pair):
    """`spec` with one occurrence of edge `pair` of relation `et` removed."""
    import copy
    import dataclasses
    topo = copy.deepcopy(spec.topology)
    rels = []
    for k, e in topo.relations:
        e = [list(p) for p in e]
        if k == tuple(et):
            e.remove(list(pair))
        rels.append((k, e))
    topo.relations = rels
    return dataclasses.replace(spec, topology=topo)


@pytest.mark.parametrize("model,B", sorted({("limbs8_h128_L5", 17)} | {(m, B) for m, B, _, _ in gen.MANY_ROW_CASES}))
def test_comparison_flags_one_dropped_row_of_the_sum_into_the_base(model, B):
    """The oracle evaluated with ONE of the in-edges into the base node removed -- what an aggregate that drops a row computes -- against the true
    reference, through the comparisons of the GPU files: a hidden state (X1[base], which that sum feeds) and at least one gradient differ in bits.
    (The reference compared with itself is clean.)"""
    spec, case, ref, _ = gx._reference.__wrapped__(model, B)
    assert _flagged(spec, ref, B, ref) == ([], [])
    et, j, i = _edges_into(spec, "base")[-1]
    got = xd.reference(_without_edge(spec, et, (j, i)), case, ref["gout"])
    bad_h, bad_g = _flagged(spec, ref, B, got)
    assert any("X1[base]" in b for b in bad_h) and bad_g, (bad_h[:3], bad_g[:3])


def test_comparison_flags_a_repeated_edge_counted_once():
    """The same for a repeated edge into a live node of a random topology, counted once (PyG sums it twice)."""
    done = 0
    for model, B in gen.RANDOM_CASES:
        spec, case, ref, _ = gx._reference.__wrapped__(model, B)
        live, _ = spec.node_liveness()
        for et in spec.edge_types:
            e = [tuple(p) for p in spec.topology.edges(et)]
            rep = [p for p in e if e.count(p) > 1 and p[1] in live[0][et[2]]]
            if not rep:
                continue
            got = xd.reference(_without_edge(spec, et, rep[0]), case, ref["gout"])
            bad_h, bad_g = _flagged(spec, ref, B, got)
            assert any(f"X1[{et[2]}]" in b for b in bad_h) and bad_g, (model, et, bad_h[:3], bad_g[:3])
            done += 1
    assert done > 0


def _algebra_reference(spec, case, gout):
    """out, hidden states and parameter gradients of the kernels' algebra (exact_data._kernel_algebra: the oracle's bits, check_exact (a)) in the layout
    of xd.reference."""
    B = case["B"]
    P = {k: v.clone().requires_grad_(True) for k, v in case["params"].items()}
    out, inter, _, _ = xd._kernel_algebra(spec, P, case["x"], B)
    out.backward(gout)
    X = {t: inter[f"X0.{t}"].detach() for t in spec.node_types}
    hidden = [torch.cat([X[t] for t in spec.node_types], dim=1)]
    for l in range(spec.num_layers):
        X = {t: (inter[f"X{l + 1}.{t}"].detach() if f"X{l + 1}.{t}" in inter else X[t]) for t in spec.node_types}
        hidden.append(torch.cat([X[t] for t in spec.node_types], dim=1))
    return {"out": out.detach(), "hidden": hidden, "grads": {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in P.items()}}


@pytest.mark.parametrize("model,B", gen.MEAN_CASES)
def test_comparison_flags_a_mean_scaled_by_the_wrong_degree(monkeypatch, model, B):
    """The 'mean' case has live destinations of in-degree 1, 2 and 4 (one edge repeated) on its mean relation -- and the kernels' algebra with the
    in-degree-4 node scaled by 1 / 2 instead of 1 / 4 differs from the reference in a hidden state (X1[base]) and in at least one gradient, where
    with the true scales it is the reference's bits."""
    spec, case, ref, _ = gx._reference.__wrapped__(model, B)
    et = ("base", "gt", "base")
    live, _ = spec.node_liveness()
    deg = {}
    for _, i in spec.topology.edges(et):
        deg[i] = deg.get(i, 0) + 1
    e = [tuple(p) for p in spec.topology.edges(et)]
    assert sorted(deg[i] for i in live[0]["base"]) == [1, 2, 2, 4] and any(e.count(p) > 1 for p in e)
    assert xd.mean_scales(spec, et) is not None and {xd.mean_scales(spec, k) is None for k in spec.edge_types if k != et} == {True}
    assert _flagged(spec, ref, B, _algebra_reference(spec, case, ref["gout"])) == ([], [])
    true = xd.mean_scales
    monkeypatch.setattr(xd, "mean_scales", lambda s, k: None if true(s, k) is None else [0.5 if v == 0.25 else v for v in true(s, k)])
    bad_h, bad_g = _flagged(spec, ref, B, _algebra_reference(spec, case, ref["gout"]))
    assert any("X1[base]" in b for b in bad_h) and bad_g, (bad_h[:3], bad_g[:3])


def test_mean_scale_leaves_the_in_degree_one_cases_alone():
    """Every 'mean' relation of the reference's robots has in-degree 1: no scale is applied (the emulation and the algebra are what they were)."""
    for name in ("a1c2_L3", "mck4_cls_L3"):
        spec = gx._spec(name)
        assert any(xd.relation_aggr(spec.kind, et) == "mean" for et in spec.edge_types)
        assert all(xd.mean_scales(spec, et) is None for et in spec.edge_types)


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


# ---------------------------------------------------------------------------------------------------
# the fused cross-entropy steps' cases (tests/test_exact_ce_gpu.py)
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,B", sorted(cex.CE_CASES))
def test_ce_case_is_rounding_free_and_covering(model, B):
    """(a)-(c) with the cross-entropy gradient and (i)-(iii) of exact_data.check_exact_ce for every (model, batch, seed, wrong share) of the GPU file; the
    gradient is the fp64 softmax's to 2^-149 per element; the generic engine's cases stage bf16 aggregates only."""
    c = cex.CE_CASES[(model, B)]
    spec, case, ref, stats = cex._reference.__wrapped__(model, B)
    assert stats["fwd_sum_bound"] <= 1.0 and stats["bwd_sum_bound"] <= 1.0 and stats["zero_decisions"] > 0
    assert case["ce_gout_err"] <= 2.0 ** -149 and bool(c["ties"]) == (stats["ties"] > 0)
    assert stats["ties"] + stats["right"] + stats["wrong"] == B * spec.num_nodes[spec.out_type] and stats["right"] > 0 and stats["wrong"] > 0
    assert ref["loss"] == case["loss_ce"] > 0 and (stats["loss_bound"] == 0.0) == (not c["ties"])
    if (model, B) in cex.GENERIC_CASES:
        assert stats["aggregates_not_bf16"] == [], stats["aggregates_not_bf16"][:5]
    print(f"\n{model} B={B}: seed {c['seed']}, wrong share {c['wrong_share']}, label seed {c['label_seed']}, flip_row {c.get('flip_row')}: ties / right / wrong = {stats['ties']} / {stats['right']} / "
          f"{stats['wrong']}, bwd_sum_bound {stats['bwd_sum_bound']:.3f}, |fp64 softmax gradient - gout| <= {case['ce_gout_err']:.1e}, loss {case['loss_ce']!r}")


def test_ce_matrix_has_the_cases_with_ties_it_must():
    assert all(cex.CE_CASES[(cex.LDS_MODEL, B)]["ties"] for B in (16, 1024))
    assert any(c["ties"] for (m, B), c in cex.CE_CASES.items() if "_h256_" in m or "_h384_" in m)
    assert not set(cex.CE_CASES) & set(cex.LEFT_OUT)
    assert {(cex.LDS_MODEL, B) for B in cex.LDS_BATCHES} | set(cex.FAMILY_CASES) | set(cex.GENERIC_CASES) == set(cex.CE_CASES)


@pytest.mark.parametrize("B", [16, 1024])
def test_comparison_flags_a_damaged_cross_entropy_tail(B):
    """What a wrong softmax tail would hand the backward pass (exact_data.ce_damaged_variants: one foot's labels from the next window on one tile, the two
    logits' gradients exchanged on one foot, the inv_n of a 64-window sub-step, one 16-window tile left out), run through the oracle, changes at least
    one gradient tensor the GPU file compares; the undamaged gradient changes none.  The output mask of channel dd taken for dd ^ 1 cannot show: the mask of
    every two-logit model is all ones (asserted)."""
    spec, case, ref, _ = cex._reference.__wrapped__(cex.LDS_MODEL, B)
    assert bool((spec.output_mask() == 1).all())
    assert _flagged(spec, ref, B, dict(hidden=ref["hidden"], grads=xd.reference(spec, case, case["gout_ce"])["grads"])) == ([], [])
    names = []
    for name, gout in xd.ce_damaged_variants(spec, case):
        assert not torch.equal(gout, case["gout_ce"]), name
        got = xd.reference(spec, case, gout)
        bad_h, bad_g = _flagged(spec, ref, B, got)
        assert bad_h == [] and bad_g, name
        names.append(name)
    assert len(names) == 4
