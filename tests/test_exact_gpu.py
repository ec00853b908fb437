"""The bf16, split (x3) and fp32 plans against the fp64 oracle BIT FOR BIT, on rounding-free data (tests/exact_data.py: every bf16 store and every fp32
sum is exact, which check_exact proves on the host before the reference is used).  Any wrong element -- a dropped 16-window tile, a mis-indexed 32-feature
column slice, a wrong layer -- fails here, where the bf16 plan's tolerance tests (1.5e-2 L2 against its rounding emulation) cannot see it.

Asserted: the output, every hidden state the plan computes (live nodes) and every gradient are the oracle's bits (exact-zero gradients included); the loss,
summed by fp32 atomics, within 2e-7.  The relu decisions are the oracle's own (plain torch.relu): exact-zero pre-activations are common on this data, so
relu'(0) = 0 is pinned too.

Matrix of this file (3 layers: the base nodes are dead, need[0]["base"] == []):
  * A1-C2 at 3 layers (BASELINE configs[1]'s model at the paper's depth) at B in {1, 15, 16, 17, 50, 1000, 8191, 8192, 8193, 8208} (8208: the tile-staircase
    point of the batch sweep), through the one-call step on every kernel set: the bf16 plan's default slab kernels over the compile-time program, its
    interpreter (MSHGNN_SPEC=0), both stash store policies (MSHGNN_STASH_NT=0 / 1, read per plan), the 8-wave stack kernels (MSHGNN_SLAB=0) and the per-layer
    kernels (MSHGNN_FUSED=0); the split plan over its program and its interpreter; the fp32 plan; the bf16 and split plans under type-level liveness
    (MSHGNN_PRUNE=0, the plan of rounds 1-3: every node of every live type is computed and compared, base rows included).  At 17, 1000 and 8193 windows the
    two-call route (training and evaluation forward, backward), the two-phase step and the fp64-source step on the default kernels of both plans; a chunked
    step (MSHGNN_STEP_CHUNK=64).
  * The generic-width engine (mshgnn_gen.hip), bf16 and split arithmetic, at hidden 256 (50 and 300 windows: 64- and 128-window tiles, ragged ones) and 1024
    (70 windows; the width whose seed-6 random case test_generic_gpu.py had to swap out: a cancelling gradient needs no tolerance here).
  * The padded engine at hidden 200 (zero-padded to 256, which the generic engine serves: no two-phase step there), bf16 and split.
  * MiniCheetah-K4 contact classification at 3 layers: logits and backward(gout).  The fused cross-entropy steps (step_ce, backward_ce) are pinned by
    tests/test_exact_ce_gpu.py on cases whose every logit pair is a tie or saturated, where the fp32 softmax gradient itself is exact.
Matrix of tests/test_exact_families_gpu.py (this file's table, comparisons and routes; base nodes live), at 17 and 1000 windows unless said otherwise:
  * A1-C2 at 4 layers (base encoder and base -> joint relations; also 16 and 8193 windows, also MSHGNN_PRUNE=0) and at 5 layers (the base is a destination:
    relations into base, base_transform, base rows of a stack layer; also over the programs compiled on demand, jit.py).
  * MiniCheetah-C2 classification at 4 layers, MiniCheetah-K4 classification at 5 layers, MiniCheetah-K4 regression at 3 layers.
  * MI-HGNN at 5 layers (no symmetry group); Solo K4 (also 8193 windows), C2 (4 layers) and S4 (5 layers) centroidal momentum: decoder on the base nodes.
  * Every one of them at 17 windows through the generic engine forced at hidden 128; A1-C2 L4 and Solo K4 COM L4 at hidden 256.
Matrix of tests/test_exact_generic_gpu.py (this file's table, comparisons and routes): every kernel form of the generic-width engine -- see that file.
Not covered, and why:
  * 8-layer models (A1-C2 L=8, MiniCheetah-K4 L=8, Solo-12 K4 COM): with at most one signed entry per weight row, the residual and base_transform paths grow
    values past bf16's 8 significant bits within 8 layers for every generator setting tried (weight scales 1, 0.5, 0.25 per row or per matrix, row densities
    0.25-1, bias ranges -4..2, inputs in [-1, 1] and [-2, 2]): check_exact refuses them.  The 8-layer compile-time programs are held to these kernels
    indirectly: tests/test_spec_gpu.py pins a program to the interpreter bit for bit, and the interpreter is what these two files pin to the oracle.
  * MiniCheetah-C2 classification at 5 layers: none of seeds 1..12 closes it at 17 windows (X4.joint leaves bf16); it stops at 4 layers, where its base is a
    source only.  Its base-destination kernels are those MiniCheetah-K4 L5 and A1-C2 L5 run.
  * Of the cross-entropy steps, what tests/test_exact_ce_gpu.py cannot reach: batch sizes that are not powers of two (inv_n then has 24 significant bits and the
    first bf16 store of dX_L rounds it), the compile-time DecFacts tail with two output channels (only the 8-layer classification programs instantiate it,
    check_exact refuses 8 layers: pinned to the interpreter by tests/test_spec_gpu.py), the series step_ce routes (pinned to assemble + step_ce by torch.equal
    in tests/test_windows.py), and the (model, batch) of its LEFT_OUT.
  * The series step (step_mse_series): tests/test_windows.py already pins it to store.assemble(starts) + step_mse bit for bit, which this file pins to the
    oracle.
No (family, batch) of the two matrices is left out for want of a seed: tests/test_exact_data.py proves every one on the host.
"""
from functools import lru_cache

import pytest
import torch

from morphsym_hgnn_amd import engine as eng
from tests import exact_data as xd
from tests import helpers

pytestmark = pytest.mark.gpu

MODELS = {      # spec arguments (helpers.make_spec), generator knobs (exact_data.exact_case), the compile-time program of the LDS-resident plans
    "a1c2_L3": dict(spec=("c2", "a1-c2", "a1-c2", 128, 3, True), knobs=dict(rel_scales=(1.0,)), program="A1C2_L3"),
    "a1c2_h256_L3": dict(spec=("c2", "a1-c2", "a1-c2", 256, 3, True), knobs=dict(rel_scales=(1.0,)), program=None),
    "a1c2_h1024_L3": dict(spec=("c2", "a1-c2", "a1-c2", 1024, 3, True), knobs=dict(rel_scales=(1.0,)), program=None),
    "a1c2_h200_L3": dict(spec=("c2", "a1-c2", "a1-c2", 200, 3, True), knobs=dict(rel_scales=(1.0,)), program=None),
    "mck4_cls_L3": dict(spec=("k4", "mini_cheetah-k4", "mini_cheetah-k4", 128, 3, False), knobs=dict(rel_scales=(1.0,), bias_range=(0, 1)), program=None),
}
# (tests/test_exact_families_gpu.py adds its families -- deeper models, live base nodes, the other model kinds -- to this table, with a seed per batch size)
BATCHES = [1, 15, 16, 17, 50, 1000, 8191, 8192, 8193, 8208]
KERNEL_SETS = [      # (name, plan dtype, switches, compile-time program: True = the model's, False = none (asserted), None = not asserted)
    ("bf16", "bf16", {}, True),
    ("bf16 MSHGNN_SPEC=0", "bf16", {"MSHGNN_SPEC": "0"}, False),
    ("bf16 MSHGNN_STASH_NT=0", "bf16", {"MSHGNN_STASH_NT": "0"}, True),
    ("bf16 MSHGNN_STASH_NT=1", "bf16", {"MSHGNN_STASH_NT": "1"}, True),
    ("bf16 MSHGNN_SLAB=0", "bf16", {"MSHGNN_SLAB": "0"}, False),
    ("bf16 MSHGNN_FUSED=0", "bf16", {"MSHGNN_FUSED": "0"}, False),
    ("x3 MSHGNN_SPEC=1", "x3", {"MSHGNN_SPEC": "1"}, True),
    ("x3 MSHGNN_SPEC=0", "x3", {"MSHGNN_SPEC": "0"}, False),
    ("f32", "f32", {}, None),
    # type-level liveness (the plan of rounds 1-3: every node of every live type, base rows included; other tables, so the program it takes is printed, not asserted)
    ("bf16 MSHGNN_PRUNE=0", "bf16", {"MSHGNN_PRUNE": "0"}, None),
    ("x3 MSHGNN_PRUNE=0", "x3", {"MSHGNN_PRUNE": "0"}, None),
]
WIDE_CASES = [("a1c2_h256_L3", 50), ("a1c2_h256_L3", 300), ("a1c2_h1024_L3", 70)]
PADDED_BATCHES = [50]
CLS_BATCHES = [17, 1000]
TWO_CALL_BATCHES = [17, 1000, 8193]
SEED = 3
LOSS_RTOL = 2e-7
SWITCHES = ("MSHGNN_SPEC", "MSHGNN_STASH_NT", "MSHGNN_SLAB", "MSHGNN_FUSED", "MSHGNN_STEP_CHUNK", "MSHGNN_ENGINE", "MSHGNN_PRUNE")


def _spec(model):
    m = MODELS[model]      # ("build": a spec builder of tests/helpers.py with its arguments, for the models helpers.make_spec does not name)
    return m["build"][0](*m["build"][1:]) if "build" in m else helpers.make_spec(*m["spec"])


def _seed(model, B):
    """The seed of a (model, batch size): closure and coverage depend on the batch, so a family lists the seed the host search found for each of its own."""
    return MODELS[model].get("seeds", {}).get(B, SEED)


@lru_cache(maxsize=2)
def _reference(model, B, seed=None):
    spec = _spec(model)
    case = xd.exact_case(spec, B, _seed(model, B) if seed is None else seed, **MODELS[model]["knobs"])
    stats = {}
    ref = xd.check_exact(spec, case, stats=stats)
    ref["hidden"] = [h.float() for h in ref["hidden"]]      # (bf16 values, proven by check_exact: fp32 holds them exactly)
    return spec, case, ref, stats


def _engine(monkeypatch, spec, model, dtype, env, program):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    e = eng.make_engine(spec, dtype)          # (the switches are read when the plan is created)
    name = ("X3_" if dtype == "x3" else "") + (MODELS[model]["program"] or "")
    if program is True:
        assert e.specialised == name, (dtype, env, e.specialised)
    elif program is False:
        assert getattr(e, "specialised", "") == "", (dtype, env, e.specialised)
    elif "MSHGNN_PRUNE" in env:
        print(f"\n{model} {dtype} {env}: kernels of program {e.specialised!r}")
    return e


def _compare(bad, what, got, ref):
    d = xd.first_difference(got, ref)
    if d is not None:
        bad.append(f"{what}: {d}")


def _compare_hidden(bad, what, e, spec, ref, B, layers):
    sl = helpers.node_slices(spec)
    liv, need = spec.node_liveness()
    for l in layers:
        got = e.hidden_state(B, l)
        nodes = need[0] if l == 0 else liv[l - 1]
        for t in spec.node_types:
            if nodes[t]:
                idx = torch.tensor(nodes[t]) + sl[t].start
                g, r = got[:, idx].double().cpu(), ref["hidden"][l][:, idx].double()
                d = xd.first_difference(g, r)
                if d is not None:
                    w = (g != r).nonzero()[0].tolist()
                    bad.append(f"{what} X{l}[{t}]: {d}; " + xd.locate((w[0], int(idx[w[1]]), w[2]), "first"))


def _compare_grads(bad, what, spec, gflat, ref):
    grads = eng.unflatten(spec, gflat)
    for k, r in ref["grads"].items():
        _compare(bad, f"{what} grad {k}", grads[k], r)


def _compare_loss(bad, what, loss, ref):
    err = abs(float(loss) - ref["loss"]) / abs(ref["loss"])
    if not err <= LOSS_RTOL:
        bad.append(f"{what}: loss rel err {err:.3e}")


def _step(bad, name, e, spec, case, ref, B, hidden=True):
    flat = eng.flatten_params(spec, case["params"], e.device)
    out, loss, g = e.step_mse(e.cast_inputs(case["x"]), flat, case["y"].to(e.device, torch.float32).contiguous(), B)
    torch.cuda.synchronize()
    _compare(bad, f"{name} step_mse out", out, ref["out"])
    if hidden:      # (a one-call step does not stash X_L: the output and the decoder's gradients cover it)
        _compare_hidden(bad, f"{name} step_mse", e, spec, ref, B, range(spec.num_layers))
    _compare_grads(bad, f"{name} step_mse", spec, g, ref)
    _compare_loss(bad, f"{name} step_mse", loss, ref)


def _two_call(bad, name, e, spec, case, ref, B):
    """Training forward (output, every hidden state X_0..X_L), evaluation forward, backward of the reference's output gradient."""
    flat = eng.flatten_params(spec, case["params"], e.device)
    xs = e.cast_inputs(case["x"])
    out = e.forward(xs, flat, B, training=True).clone()
    torch.cuda.synchronize()
    _compare(bad, f"{name} forward out", out, ref["out"])
    _compare_hidden(bad, f"{name} forward", e, spec, ref, B, range(spec.num_layers + 1))
    _compare(bad, f"{name} evaluation forward out", e.forward(xs, flat, B, training=False), ref["out"])
    g = e.backward(xs, flat, ref["gout"].to(e.device, torch.float32).contiguous(), B)
    torch.cuda.synchronize()
    _compare_grads(bad, f"{name} backward", spec, g, ref)


def _two_phase(bad, name, e, spec, case, ref, B):
    assert e.info.grad_split >= 0, f"{name}: the plan has no two-phase step"
    flat = eng.flatten_params(spec, case["params"], e.device)
    xs = e.cast_inputs(case["x"])
    out = torch.empty(B * e.n_out, spec.out_channels, dtype=torch.float32, device=e.device)
    g = torch.empty(spec.flat_size(), dtype=torch.float32, device=e.device)
    loss = torch.empty(1, dtype=torch.float32, device=e.device)
    y = case["y"].to(e.device, torch.float32).contiguous()
    e.step_mse_phase(0, xs, flat, y, B, out, g, loss)
    e.step_mse_phase(1, xs, flat, y, B, out, g, loss)
    torch.cuda.synchronize()
    _compare(bad, f"{name} step_mse_phase out", out, ref["out"])
    _compare_grads(bad, f"{name} step_mse_phase", spec, g, ref)
    _compare_loss(bad, f"{name} step_mse_phase", loss, ref)


def _src_step(bad, name, e, spec, case, ref, B):
    """The fp64-source step: the encoder reads the caller's fp64 device tensors (mshgnn_step_mse_src)."""
    xs64 = e.cast_inputs({t: v.to(e.device) for t, v in case["x"].items()})
    assert isinstance(xs64, eng.WideInputs), "the fp64-source route"
    flat = eng.flatten_params(spec, case["params"], e.device)
    out, loss, g = e.step_mse(xs64, flat, case["y"].to(e.device, torch.float32).contiguous(), B)
    torch.cuda.synchronize()
    _compare(bad, f"{name} step_mse_src out", out, ref["out"])
    _compare_hidden(bad, f"{name} step_mse_src", e, spec, ref, B, range(spec.num_layers))
    _compare_grads(bad, f"{name} step_mse_src", spec, g, ref)
    _compare_loss(bad, f"{name} step_mse_src", loss, ref)


@pytest.mark.parametrize("B", BATCHES)
def test_one_call_step_is_the_oracle_bit_for_bit_on_every_kernel_set(monkeypatch, B):
    model = "a1c2_L3"
    spec, case, ref, stats = _reference(model, B)
    bad = []
    for name, dtype, env, program in KERNEL_SETS:
        e = _engine(monkeypatch, spec, model, dtype, env, program)
        _step(bad, f"{model} B={B} {name}", e, spec, case, ref, B)
        del e
    print(f"\n{model} B={B}: {stats['zero_decisions']} exact-zero relu pre-activations, {stats['nonzero_grads']} of {stats['grads']} gradient tensors non-zero, "
          f"sums of |terms| <= {stats['fwd_sum_bound']:.2e} (forward) / {stats['bwd_sum_bound']:.2e} (backward) of the fp32 limit")
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("B", TWO_CALL_BATCHES)
def test_two_call_two_phase_and_fp64_source_routes_are_the_oracle_bit_for_bit(monkeypatch, B):
    """forward (training, evaluation) + backward(gout) with the reference's dyadic gout, the two-phase step (mshgnn_step_mse_phase) and the fp64-source step
    (the encoder reads the caller's fp64 device tensors: mshgnn_step_mse_src) on the default kernels of the bf16 and split plans."""
    model = "a1c2_L3"
    spec, case, ref, _ = _reference(model, B)
    bad = []
    for name, dtype, env, program in (KERNEL_SETS[0], KERNEL_SETS[6]):
        e = _engine(monkeypatch, spec, model, dtype, env, program)
        _two_call(bad, name, e, spec, case, ref, B)
        _two_phase(bad, name, e, spec, case, ref, B)
        _src_step(bad, name, e, spec, case, ref, B)
        del e
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("dtype", ["bf16", "x3"])
def test_chunked_one_call_step_is_the_oracle_bit_for_bit(monkeypatch, dtype):
    """MSHGNN_STEP_CHUNK=64 at 200 windows: the one-call step as sub-steps of 64 (a ragged last one) accumulating into one gradient -- exact data makes
    the sub-step sums exact, so the result is the oracle's bits as for a whole-batch step."""
    model, B = "a1c2_L3", 200
    spec, case, ref, _ = _reference(model, B)
    e = _engine(monkeypatch, spec, model, dtype, {"MSHGNN_STEP_CHUNK": "64"}, None)
    bad = []
    _step(bad, f"{dtype} chunked", e, spec, case, ref, B, hidden=False)      # (the workspace holds the last sub-step only)
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("model,B", WIDE_CASES)
def test_generic_engine_is_the_oracle_bit_for_bit(monkeypatch, model, B):
    """The generic-width engine (mshgnn_gen.hip: hidden 256 and 1024) in bf16 and split arithmetic: one-call step and two-call route."""
    spec, case, ref, _ = _reference(model, B)
    bad = []
    for dtype in ("bf16", "x3"):
        e = _engine(monkeypatch, spec, model, dtype, {}, False)
        assert e.generic, f"{model} {dtype}: not the generic engine"
        _step(bad, f"{model} B={B} {dtype}", e, spec, case, ref, B)
        _two_call(bad, f"{model} B={B} {dtype}", e, spec, case, ref, B)
        del e
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("B", PADDED_BATCHES)
def test_padded_engine_is_the_oracle_bit_for_bit(monkeypatch, B):
    """A hidden width that is not a multiple of 128 (200, zero-padded to 256 by engine.PaddedEngine, on the generic engine): one-call step, two-call route."""
    model = "a1c2_h200_L3"
    spec, case, ref, _ = _reference(model, B)
    bad = []
    for dtype in ("bf16", "x3"):
        e = _engine(monkeypatch, spec, model, dtype, {}, None)
        assert isinstance(e, eng.PaddedEngine) and e.inner_spec.hidden == 256 and e.generic
        _step(bad, f"{model} B={B} {dtype}", e, spec, case, ref, B)
        _two_call(bad, f"{model} B={B} {dtype}", e, spec, case, ref, B)
        del e
    assert not bad, "\n".join(bad[:20])


CLS_KERNEL_SETS = [("bf16", "bf16", {}), ("bf16 MSHGNN_FUSED=0", "bf16", {"MSHGNN_FUSED": "0"}), ("x3", "x3", {})]


def _classification(monkeypatch, model, B, program=None):
    """Logits, every hidden state and backward(gout) with a dyadic gout, on the bf16 plan's default and per-layer kernels and the split plan."""
    spec, case, ref, _ = _reference(model, B)
    bad = []
    for name, dtype, env in CLS_KERNEL_SETS:
        e = _engine(monkeypatch, spec, model, dtype, env, program)
        assert not e.generic
        _two_call(bad, f"{model} B={B} {name}", e, spec, case, ref, B)
        del e
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("B", CLS_BATCHES)
def test_classification_forward_and_backward_are_the_oracle_bit_for_bit(monkeypatch, B):
    """MiniCheetah-K4 contact classification (mean aggregation over in-degree-1 relations, foot-input masks, 2 logits per foot): logits, every hidden state
    and backward(gout) with a dyadic gout, on the bf16 plan's default and per-layer kernels and the split plan."""
    _classification(monkeypatch, "mck4_cls_L3", B)
