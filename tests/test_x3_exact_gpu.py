"""The split-bf16 plan's LO halves against the fp64 oracle BIT FOR BIT.

On tests/exact_data.py every operand is a bf16 value: in tests/test_exact_gpu.py, test_exact_families_gpu.py, test_exact_generic_gpu.py and
test_input_grad_exact_gpu.py both cross products, the lo planes of every stash, the lo rows handed through LDS, the lo images of the packed weights, the lo
halves of the weight-gradient launch, the generic engine's split arithmetic and the split form of mshgnn_input_grad run on zeros.  Here one operand class at
a time carries non-zero lo halves (tests/x3_emulation.py: the families wide_x, wide_gout, wide_enc, wide_conv<l>, wide_dec, wide_bt0 / wide_bt2) while every product
keeps a factor whose lo is zero, so the kernels must still give the oracle's bits.  tests/test_x3_emulation.py proves on the host, for exactly the cases
of this file, that the data closes ((a) .. (f) of x3_emulation.check_wide), that the families of a model widen every operand class it has, and that every
damaged variant (a dropped cross term in one product class, the planes of one stash exchanged) would be seen by what is compared here.

Compared, all for identical bits (the loss alone, summed by fp32 atomics, at test_exact_gpu.LOSS_RTOL): the output, every hidden state, every parameter
gradient, the input gradients -- and, new here, for the split plan the hi plane and the lo plane of every X_l and (after a backward) every dX_l, read straight
from the workspace rows [hi | lo] and compared with x3_emulation.split() of the reference on the live nodes: that pins the split's rounding (nearest even,
twice), which the hi + lo that Engine.hidden_state forms cannot.

Kernel sets of the wide families: the split plan over its compile-time program (MSHGNN_SPEC=1, asserted where the model has one), over the interpreter
(MSHGNN_SPEC=0), under type-level liveness (MSHGNN_PRUNE=0), and the fp32 plan.  The bf16 plan cannot hold this data and is not run.

Under MSHGNN_PRUNE=0 the plan also computes rows that reach no output; the host proof says nothing about those, so there the hidden states are compared on the
default plan's nodes only (through their planes), and the wide_bt families are not run (type-level liveness runs base_transform in several layers).

Matrix (BATCHES / ONLY below; the seed of a (model, family, batch) is the existing tables' seed unless SEEDS names the one a host search over 1 .. 12 found):
  * A1-C2 at 3 layers (X3_A1C2_L3), every family, B in {1, 15, 16, 17, 65, 200}: one-call step on every kernel set; at 17 and 200 also the two-call route,
    the two-phase step, the fp64-source step and a chunked step (MSHGNN_STEP_CHUNK=64: at 200 windows four sub-steps, a ragged last one).
  * A1-C2 at 5 layers (base_transform through mlp_mac3, base rows in the layers; also wide_bt0 / wide_bt2: its base_transform is live in layer 0 alone),
    Solo K4 centroidal momentum at 4 layers (out type first): one-call step on every kernel set, two-call route on the interpreter; MiniCheetah-K4 classification
    at 5 layers (the ALIAS kernels; wide_bt0 / wide_bt2 too): logits, every hidden state, backward(gout) on every kernel set.  B in {17, 33}.
  * The generic-width engine, split arithmetic: A1-C2 hidden 256 at B = 50 and 300 (every family), hidden 1024 at B = 70 (wide_x, wide_gout), padded hidden
    200 at B = 50 (wide_x, wide_conv1), A1-C2 at 5 layers (live base) forced through it at hidden 128, 17 windows; one-call step and two-call route.
  * Input gradients: A1-C2 at 4 layers with enc_cover, wide_gout / wide_dec (dY_enc wide, W_enc narrow) and wide_enc (W_enc wide, dY_enc narrow), B in
    {1, 17}, after backward(gout) (fp32 and fp64 outputs) and backward_mse, split and fp32 plans, with the planes of dY_enc; the generic engine at hidden 256.
Left out, and the condition of x3_emulation.check_wide that refuses it (tests/test_x3_emulation.py asserts each with the table's seed):
  * EVERY wide family at 1000 windows, on every model (LEFT_OUT): no seed of 1 .. 12 closes one; condition (e) -- see REFUSED_BATCH below for the figures.  200, 300
    and 33 windows stand in as the many-tile batches, over and above the issue's list.
  * wide_x / wide_gout at 8193 windows (the weight-gradient launch's window parts and second round of workgroups): the sums grow with the batch -- with the table's
    seed wide_gout is refused by (e) (decoder.weight: 10.9 times the limit) and wide_x by (c) already (a weight gradient is no fp32 value).  Those launch shapes keep the bf16-valued data of tests/test_exact_gpu.py (8191 .. 8208 windows) and the 1e-4 tolerance of tests/test_x3_gpu.py.
  * "wide_bt", both base_transform matrices at once: T1 is wide with W1 and meets the wide W2, conditions (a) and (d); wide_bt0 and wide_bt2 widen one each.
    Solo K4 COM runs base_transform in every layer, where the shared matrices compound over the layers and no widening of them closes: its W_bt images stay narrow,
    and the hi.lo term of its chain products cannot be seen on any data that closes (x3_emulation.unseeable).
  * A one-live-layer A1-C2 model for wide_bt at depth 4: A1-C2 runs base_transform in no layer at depths 3 and 4; depth 5 is its one-live-layer model and is run.
"""
from functools import lru_cache

import pytest
import torch

from morphsym_hgnn_amd import engine as eng
from tests import exact_data as xd
from tests import helpers
from tests import test_exact_gpu as gx
from tests import x3_emulation as xe

pytestmark = pytest.mark.gpu

_K1 = dict(rel_scales=(1.0,))
_CLS = dict(rel_scales=(1.0,), bias_range=(0, 1))
MODELS = {      # spec arguments, generator knobs, compile-time program, generic engine, input gradients, the seed of the existing tables
    "a1c2_L3": dict(spec=("c2", "a1-c2", "a1-c2", 128, 3, True), knobs=_K1, program="A1C2_L3", seed=3),
    "a1c2_L5": dict(spec=("c2", "a1-c2", "a1-c2", 128, 5, True), knobs=_K1, program=None, seed=5),
    "mck4_cls_L5": dict(spec=("k4", "mini_cheetah-k4", "mini_cheetah-k4", 128, 5, False), knobs=_CLS, program=None, seed=2),
    "solok4_com_L4": dict(spec=("k4_com", "solo-k4-com", "solo-k4", 128, 4, True, 1), knobs=_K1, program=None, seed=3),
    "a1c2_h256_L3": dict(spec=("c2", "a1-c2", "a1-c2", 256, 3, True), knobs=_K1, program=None, seed=3, generic=True),
    "a1c2_h1024_L3": dict(spec=("c2", "a1-c2", "a1-c2", 1024, 3, True), knobs=_K1, program=None, seed=3, generic=True),
    "a1c2_h200_L3": dict(spec=("c2", "a1-c2", "a1-c2", 200, 3, True), knobs=_K1, program=None, seed=3, generic=True),
    "a1c2_L5_generic": dict(spec=("c2", "a1-c2", "a1-c2", 128, 5, True), knobs=_K1, program=None, seed=5, generic=True, force=True),
    "a1c2_L4_ig": dict(spec=("c2", "a1-c2", "a1-c2", 128, 4, True), knobs=dict(_K1, enc_cover=True), program=None, seed=3, input_grads=True),
    "a1c2_h256_L4_ig": dict(spec=("c2", "a1-c2", "a1-c2", 256, 4, True), knobs=dict(_K1, enc_cover=True), program=None, seed=3, generic=True, input_grads=True),
}
IG_FAMILIES = ["wide_gout", "wide_dec", "wide_enc"]
# (model, family, batch) -> seed, where the existing tables' seed does not close the case (host search, seeds 1 .. 12; the condition that refused that seed)
SEEDS = {
    ("a1c2_L3", "wide_gout", 1): 4, ("a1c2_L4_ig", "wide_gout", 1): 9,      # (f): one window leaves a 32-feature slice of a dX_l without a non-zero lo
    ("a1c2_h256_L3", "wide_enc", 300): 2, ("a1c2_h256_L3", "wide_conv0", 300): 2, ("a1c2_h256_L3", "wide_conv1", 300): 2,      # (e): 1.01 of 2^24 units
    ("a1c2_h256_L3", "wide_conv2", 50): 8, ("a1c2_h256_L3", "wide_conv2", 300): 8,      # (f) at 50, (e) at 300
    ("a1c2_h1024_L3", "wide_gout", 70): 2,      # (f)
}
# The issue's batch of 1000 windows: no seed of 1 .. 12 closes ANY wide family there, on any model.  Condition (e) of x3_emulation.check_wide refuses them (the
# table's seed: asserted on the host; the refusals the search recorded for other seeds name (e) as well): a
# weight gradient is one sum over every window, and with an operand of 9 or more significant bits its sum of |terms| passes 2^24 units of the terms' grid
# between 300 and 450 windows at 3 layers and near 45 at 5 (decoder.weight first: A1-C2 L3 2.0 .. 4.0 times the limit at 1000 windows, A1-C2 L5 and
# MiniCheetah-K4 L5 9 .. 23 times).  The many-tile forms run at the largest batches that close instead: 200 windows at 3 layers (13 tiles, a ragged one; four
# sub-steps of 64 in the chunked step), 300 on the generic engine, 33 at 4 and 5 layers (two whole tiles and a window).
REFUSED_BATCH = 1000
LEFT_OUT_CONDITION = "(e)"
BATCHES = {"a1c2_L3": [1, 15, 16, 17, 65, 200, 1000], "a1c2_L5": [17, 33, 1000], "mck4_cls_L5": [17, 33, 1000], "solok4_com_L4": [17, 33, 1000],
           "a1c2_h256_L3": [50, 300], "a1c2_h1024_L3": [70], "a1c2_h200_L3": [50], "a1c2_L5_generic": [17], "a1c2_L4_ig": [1, 17, 1000], "a1c2_h256_L4_ig": [17]}
ONLY = {"a1c2_h1024_L3": ["wide_x", "wide_gout"], "a1c2_h200_L3": ["wide_x", "wide_conv1"], "a1c2_L4_ig": IG_FAMILIES, "a1c2_h256_L4_ig": IG_FAMILIES}
ROUTE_BATCHES = [17, 200]      # (the issue's 17 and 1000: see REFUSED_BATCH)

KERNEL_SETS = [      # (name, plan dtype, switches, compile-time program: True = the model's where it has one (asserted), False = none (asserted), None = printed)
    ("x3 MSHGNN_SPEC=1", "x3", {"MSHGNN_SPEC": "1"}, True),
    ("x3 MSHGNN_SPEC=0", "x3", {"MSHGNN_SPEC": "0"}, False),
    ("x3 MSHGNN_PRUNE=0", "x3", {"MSHGNN_PRUNE": "0"}, None),
    ("f32", "f32", {}, None),
]


def _spec(model):
    return helpers.make_spec(*MODELS[model]["spec"])


def model_families(model):
    return ONLY.get(model) or [f for f in xe.families(_spec(model)) if f != "narrow"]


LEFT_OUT = {(m, f, REFUSED_BATCH): LEFT_OUT_CONDITION for m in MODELS for f in model_families(m) if REFUSED_BATCH in BATCHES[m]}


def cases(model):
    """the (family, batch) this file runs for a model"""
    return [(f, B) for B in BATCHES[model] for f in model_families(model) if (model, f, B) not in LEFT_OUT]


def run_batches(model):
    return [B for B in BATCHES[model] if any(c[1] == B for c in cases(model))]


def seed_of(model, family, B):
    return SEEDS.get((model, family, B), MODELS[model]["seed"])


@lru_cache(maxsize=12)
def _reference(model, family, B):
    m = MODELS[model]
    spec = _spec(model)
    case = xe.wide_case(spec, family, B, seed_of(model, family, B), **m["knobs"])
    ref, wide = xe.check_wide(spec, case, input_grads=m.get("input_grads", False), generic=m.get("generic", False))
    assert wide, f"{model} {family} B={B}: no operand carries a lo half"
    ref["hidden"] = [h.float() for h in ref["hidden"]]      # (fp32 values: check_wide (c))
    return spec, case, ref


def _engine(monkeypatch, spec, model, name, dtype, env, program):
    """gx._engine over this file's table (the switches are read when the plan is created; the program is asserted where the model has one)"""
    m = MODELS[model]
    if m.get("force"):
        env = dict(env, MSHGNN_ENGINE="generic")
    for k in gx.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    e = eng.make_engine(spec, dtype)
    got = getattr(e, "specialised", "")
    if program is True and m["program"]:
        assert got == "X3_" + m["program"], (model, name, got)
    elif program is not None:
        assert got == "", (model, name, got)
    assert e.generic == bool(m.get("generic")), f"{model} {name}: the wrong engine"
    return e


def _planes(e, off, B, width):
    """the hi and the lo plane of an activation tensor of the split plan's workspace, [B, NN, width] each: rows of [hi h | lo h] bf16, node-major"""
    assert e.storage == "x3"
    ws, nn_ = e.workspace(B, True), e.info.total_nodes
    h = e.inner_spec.hidden if getattr(e, "padded", False) else e.spec.hidden
    halves = ws[off:off + 4 * B * nn_ * h].view(torch.bfloat16).view(nn_, B, 2, h)
    return tuple(halves[:, :, i].permute(1, 0, 2)[..., :width].double().cpu() for i in (0, 1))


def _compare_planes(bad, what, e, spec, ref, B, x_layers, dx_layers):
    """hi and lo plane of X_l (x_layers) and dX_l (dx_layers) on the live nodes against split() of the reference; the fp32 plan: the values themselves"""
    live = xe._live_nodes(spec)
    lay = e.layout(B, True)
    for kind, layers, offs, key in (("X", x_layers, lay.x, "hidden_pairs"), ("dX", dx_layers, lay.dx, "dx_pairs")):
        for l in layers:
            idx = live[l]
            if e.storage == "x3":
                got = dict(zip(("hi", "lo"), _planes(e, offs[l], B, spec.hidden)))
                want = dict(zip(("hi", "lo"), ref[key][l]))
            else:
                got = {"value": (e.hidden_state(B, l) if kind == "X" else e.grad_hidden(B, l)).double().cpu()}
                want = {"value": ref[key][l][0] + ref[key][l][1]}
            for plane in got:
                g, r = got[plane][:, idx], want[plane][:, idx]
                d = xd.first_difference(g, r)
                if d is not None:
                    w = (g != r).nonzero()[0].tolist()
                    bad.append(f"{what} {kind}{l} {plane} plane: {d}; " + xd.locate((w[0], int(idx[w[1]]), w[2]), "first"))


def _type_level(name):
    return "MSHGNN_PRUNE" in name


def _step(bad, name, e, spec, case, ref, B):
    """one-call step.  Under MSHGNN_PRUNE=0 the plan also computes rows that reach no output; check_wide proves nothing about those, so there the hidden
    states are compared on the default plan's nodes alone (plane by plane, which holds the values too)."""
    gx._step(bad, name, e, spec, case, ref, B, hidden=not _type_level(name))
    L = spec.num_layers
    _compare_planes(bad, f"{name} step_mse", e, spec, ref, B, range(L), range(L))      # (a one-call step stashes neither X_L nor dX_L: LDS holds them)


def _two_call(bad, name, e, spec, case, ref, B):
    """gx._two_call (training forward, every hidden state, evaluation forward, backward(gout)) and the planes of every X_l and dX_l"""
    L = spec.num_layers
    if not _type_level(name):
        gx._two_call(bad, name, e, spec, case, ref, B)
    else:      # (the same calls; the hidden states on the default plan's nodes alone, through their planes: see _step)
        flat = eng.flatten_params(spec, case["params"], e.device)
        xs = e.cast_inputs(case["x"])
        gx._compare(bad, f"{name} forward out", e.forward(xs, flat, B, training=True).clone(), ref["out"])
        gx._compare(bad, f"{name} evaluation forward out", e.forward(xs, flat, B, training=False), ref["out"])
        g = e.backward(xs, flat, ref["gout"].to(e.device, torch.float32).contiguous(), B)
        torch.cuda.synchronize()
        gx._compare_grads(bad, f"{name} backward", spec, g, ref)
    _compare_planes(bad, f"{name} forward + backward", e, spec, ref, B, range(L + 1), range(L + 1))


def _run(monkeypatch, model, B, sets, routes):
    """every family of (model, B) on every kernel set: one plan per kernel set, reused across the families"""
    spec = _spec(model)
    bad = []
    for name, dtype, env, program in sets:
        e = _engine(monkeypatch, spec, model, name, dtype, env, program)
        for family, _ in [c for c in cases(model) if c[1] == B]:
            if _type_level(name) and family.startswith("wide_bt"):
                continue      # (type-level liveness runs base_transform in more than one layer: the shared matrices compound, the rows leave hi + lo)
            _, case, ref = _reference(model, family, B)
            for route in routes:
                route(bad, f"{model} {family} B={B} {name}", e, spec, case, ref, B)
        del e
    assert not bad, "\n".join(bad[:30])


@pytest.mark.parametrize("B", run_batches("a1c2_L3"))
def test_a1c2_l3_one_call_step_on_wide_operands_is_the_oracle_bit_for_bit(monkeypatch, B):
    _run(monkeypatch, "a1c2_L3", B, KERNEL_SETS, [_step])


@pytest.mark.parametrize("B", ROUTE_BATCHES)
def test_a1c2_l3_routes_on_wide_operands_are_the_oracle_bit_for_bit(monkeypatch, B):
    """two-call route (training and evaluation forward, backward(gout)), two-phase step, fp64-source step: the split plan over its program"""
    _run(monkeypatch, "a1c2_L3", B, KERNEL_SETS[:1], [_two_call, gx._two_phase, gx._src_step])


@pytest.mark.parametrize("B", ROUTE_BATCHES)
def test_a1c2_l3_chunked_step_on_wide_operands_is_the_oracle_bit_for_bit(monkeypatch, B):
    """MSHGNN_STEP_CHUNK=64: sub-steps of 64 windows (a ragged last one at 200; at 17 one sub-step) accumulating into one gradient"""
    def chunked(bad, name, e, spec, case, ref, B):
        gx._step(bad, name, e, spec, case, ref, B, hidden=False)      # (the workspace holds the last sub-step only)
    _run(monkeypatch, "a1c2_L3", B, [("x3 MSHGNN_STEP_CHUNK=64", "x3", {"MSHGNN_STEP_CHUNK": "64"}, None)], [chunked])


@pytest.mark.parametrize("model,B", [(m, B) for m in ("a1c2_L5", "solok4_com_L4") for B in run_batches(m)])
def test_live_base_regression_models_on_wide_operands_are_the_oracle_bit_for_bit(monkeypatch, model, B):
    """A1-C2 at 5 layers (base_transform through mlp_mac3) and Solo K4 centroidal momentum at 4 layers (out type first): one-call step on every kernel
    set, the two-call route on the split plan's interpreter"""
    _run(monkeypatch, model, B, KERNEL_SETS, [_step])
    _run(monkeypatch, model, B, KERNEL_SETS[1:2], [_two_call])


@pytest.mark.parametrize("B", run_batches("mck4_cls_L5"))
def test_alias_kernels_on_wide_operands_are_the_oracle_bit_for_bit(monkeypatch, B):
    """MiniCheetah-K4 classification at 5 layers: the base_transform scratch aliases the last nodes' blocks.  Logits, every hidden state, backward(gout)."""
    _run(monkeypatch, "mck4_cls_L5", B, KERNEL_SETS, [_two_call])


@pytest.mark.parametrize("model,B", [(m, B) for m in ("a1c2_h256_L3", "a1c2_h1024_L3", "a1c2_h200_L3", "a1c2_L5_generic") for B in run_batches(m)])
def test_generic_engine_split_arithmetic_on_wide_operands_is_the_oracle_bit_for_bit(monkeypatch, model, B):
    """mshgnn_gen.hip, split arithmetic (its "x3" and its "f32" both run it): one-call step and two-call route.  A relation's aggregate is staged as ONE pair
    there: check_wide proves every staged aggregate of these cases hi + lo exactly, in both sweeps."""
    _run(monkeypatch, model, B, [("x3", "x3", {}, False)], [_step, _two_call])


def _input_grad_routes(bad, what, e, spec, case, ref, B):
    flat = eng.flatten_params(spec, case["params"], e.device)
    xs = e.cast_inputs(case["x"])
    gout = ref["gout"].to(e.device, torch.float32).contiguous()
    e.forward(xs, flat, B, training=True)
    e.backward(xs, flat, gout, B)
    for dt in (torch.float32, torch.float64):
        for t, g in e.input_grad(B, flat, dtype=dt).items():
            gx._compare(bad, f"{what} backward {str(dt)[6:]} dx[{t}]", g, ref["xgrads"][t])
    _compare_planes(bad, f"{what} backward", e, spec, ref, B, [], [0])      # (dY_enc: the stash mshgnn_input_grad reads)
    out = e.forward(xs, flat, B, training=True)
    e.backward_mse(xs, flat, out, case["y"].to(e.device, torch.float32).contiguous(), B)
    for t, g in e.input_grad(B, flat, dtype=torch.float32).items():
        gx._compare(bad, f"{what} backward_mse dx[{t}]", g, ref["xgrads"][t])


@pytest.mark.parametrize("model,B", [(m, B) for m in ("a1c2_L4_ig", "a1c2_h256_L4_ig") for B in run_batches(m)])
def test_input_grad_on_wide_operands_is_the_oracle_bit_for_bit(monkeypatch, model, B):
    """mshgnn_input_grad, split form and fp32: wide_gout / wide_dec widen dY_enc (hi.hi + lo.hi), wide_enc widens W_enc (hi.hi + hi.lo)"""
    sets = [("x3", "x3", {}, False)] if MODELS[model].get("generic") else [("x3", "x3", {}, False), ("f32", "f32", {}, None)]
    _run(monkeypatch, model, B, sets, [_input_grad_routes])
