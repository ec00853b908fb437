"""Host proofs for tests/test_x3_exact_gpu.py (no GPU): for exactly the (model, family, batch, seed) that file runs,
  * x3_emulation.check_wide passes: the three-product emulation of the split kernels equals the fp64 oracle bit for bit, every packed and stored operand
    is hi + lo exactly, every result is an fp32 value, every product has a factor whose lo is zero, every accumulation fits 2^24 units of its grid, and the
    coverage conditions hold -- so the oracle IS the reference of the GPU file, plane by plane;
  * the families of a model widen, between them, every operand class the model has;
  * every damaged variant of the emulation (one cross term dropped in one product class, the planes of one stash exchanged) differs from the oracle in a
    quantity the GPU file compares, in at least one family of the model: none may go unseen;
  * without the split (quant=False), and on the narrow family, the emulation reproduces exact_data.reference;
  * each case the GPU file lists as left out is refused by the condition it names (with the table's seed; the search over seeds 1 .. 12 is not repeated
    here).
"""
import pytest
import torch

from tests import exact_data as xd
from tests import test_x3_exact_gpu as wx
from tests import x3_emulation as xe

FULL_MODELS = [m for m in wx.MODELS if m not in wx.ONLY]      # the models that run every family


def _checked(model, family, B):
    m = wx.MODELS[model]
    spec = wx._spec(model)
    case = xe.wide_case(spec, family, B, wx.seed_of(model, family, B), **m["knobs"])
    stats = {}
    ref, wide = xe.check_wide(spec, case, input_grads=m.get("input_grads", False), generic=m.get("generic", False), stats=stats)
    return spec, case, ref, wide, stats


def test_split_rounds_to_nearest_even_twice():
    u = 2.0 ** -17
    v = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -9), 3.0, 0.0, 1 + 515 * u, 1 + 517 * u], dtype=torch.float64)
    hi, lo = xe.split(v)
    # hi: ties to even (1 + 2^-8 -> 1, 1 + 3 2^-8 -> 1 + 2^-6); the last two lie above the tie 1 + 512 u and round up to 1 + 2^-7
    assert hi.tolist() == [1.0, 1 + 2.0 ** -6, -1.0, 3.0, 0.0, 1 + 2.0 ** -7, 1 + 2.0 ** -7]
    # lo rounds too: -509 u is a tie between -508 u and -510 u (even: -508 u; away from zero would give -510 u), -507 u one between -506 u and -508 u
    # (even: -508 u; truncation would give -506 u)
    assert lo.tolist() == [2.0 ** -8, -(2.0 ** -8), -(2.0 ** -9), 0.0, 0.0, -508 * u, -508 * u]


@pytest.mark.parametrize("model,B", [(m, B) for m in wx.MODELS for B in wx.BATCHES[m]])
def test_every_case_of_the_gpu_matrix_closes(model, B):
    for family, _ in [c for c in wx.cases(model) if c[1] == B]:
        _, _, _, wide, stats = _checked(model, family, B)
        assert wide, f"{model} {family} B={B}: no operand carries a lo half"
        print(f"{model} {family} B={B} seed {wx.seed_of(model, family, B)}: worst sum of |terms| {stats['sum_bound'][1]:.3g} of 2^24 ({stats['sum_bound'][0]}), wide {stats['wide']}")


def test_what_may_be_left_out():
    """none of wide_x, wide_gout, wide_enc, a wide_conv<l>, wide_dec is missing on A1-C2 L3 or the hidden-256 generic case; on the other models at most one
    family is missing, never both wide_x and wide_gout"""
    for model in FULL_MODELS:
        run = {f for f, _ in wx.cases(model)}
        fams = [f for f in wx.model_families(model) if not f.startswith("wide_conv") and f != "wide_bt"]
        missing = [f for f in fams if f not in run] + ([] if any(f.startswith("wide_conv") for f in run) else ["wide_conv*"])
        if model in ("a1c2_L3", "a1c2_h256_L3"):
            assert not missing, (model, missing)
        assert len(missing) <= 1 and not {"wide_x", "wide_gout"} <= set(missing), (model, missing)


@pytest.mark.parametrize("model,family,B", sorted(wx.LEFT_OUT))
def test_left_out_case_is_refused_by_the_condition_listed(model, family, B):
    with pytest.raises(AssertionError) as err:
        _checked(model, family, B)
    assert str(err.value).startswith(wx.LEFT_OUT[model, family, B]), str(err.value)[:200]


@pytest.mark.parametrize("model", FULL_MODELS)
def test_families_widen_every_operand_class_and_every_damaged_variant_is_seen(model):
    m = wx.MODELS[model]
    spec, generic = wx._spec(model), m.get("generic", False)
    B = 17 if 17 in wx.BATCHES[model] else min(wx.BATCHES[model])
    unseen = [v for v in xe.damaged_variants(spec, generic) if v not in xe.unseeable(spec)]
    if not m.get("input_grads"):
        unseen = [v for v in unseen if v.get("drop", ("", ""))[1] != "dx"]      # (the input gradient is compared on the input-gradient models)
    union = set()
    for family, _ in [c for c in wx.cases(model) if c[1] == B]:
        spec, case, ref, wide, _ = _checked(model, family, B)
        union |= wide
        unseen = [v for v in unseen if not xe.variant_is_seen(spec, case, ref, v, input_grads=False, generic=generic)]
    want = xe.all_classes(spec, generic) - ({"W_bt", "W_btT"} if len(xe.bt_layers(spec)) > 1 else set())      # (x3_emulation.unseeable says why)
    assert union >= want, f"{model}: no family widens {sorted(want - union)}"
    assert not unseen, f"{model}: damaged variants no family would see: {unseen}"


@pytest.mark.parametrize("model", [m for m in wx.MODELS if wx.MODELS[m].get("input_grads")])
def test_input_gradient_cross_terms_are_seen(model):
    m = wx.MODELS[model]
    spec, generic = wx._spec(model), m.get("generic", False)
    B = min(b for b in wx.BATCHES[model] if b > 1)
    unseen = [dict(drop=(term, "dx")) for term in ("lo_hi", "hi_lo")]
    for family, _ in [c for c in wx.cases(model) if c[1] == B]:
        spec, case, ref, wide, _ = _checked(model, family, B)
        for v in list(unseen):
            em = xe.emulate_step_x3(spec, case["params"], case["x"], B, ref["gout"], generic=generic, **v)
            if any(not torch.equal(em["xgrads"][t], ref["xgrads"][t]) for t in spec.node_types):
                unseen.remove(v)
    assert not unseen, f"{model}: {unseen}"


@pytest.mark.parametrize("family", ["narrow", "wide_x", "wide_conv1"])
def test_emulation_without_the_split_and_on_narrow_data_is_the_reference(family):
    model, B = "a1c2_L3", 17
    spec = wx._spec(model)
    case = xe.wide_case(spec, family, B, wx.MODELS[model]["seed"], **wx.MODELS[model]["knobs"])
    ref = xd.reference(spec, case, case["gout_mse"], input_grads=True)
    live = xe._live_nodes(spec)
    for quant in ((True, False) if family == "narrow" else (False,)):
        em = xe.emulate_step_x3(spec, case["params"], case["x"], B, case["gout_mse"], quant=quant)
        assert torch.equal(em["out"], ref["out"])
        assert all(torch.equal(em["hidden"][l][:, live[l]], ref["hidden"][l][:, live[l]]) for l in range(spec.num_layers + 1))
        assert all(torch.equal(em["grads"][k], g) for k, g in ref["grads"].items())
        assert all(torch.equal(em["xgrads"][t], g) for t, g in ref["xgrads"].items())
        if quant:
            assert all(not bool((p[1] != 0).any()) for p in em["hidden_pairs"] + em["dx_pairs"]), "narrow data carries a lo half"
