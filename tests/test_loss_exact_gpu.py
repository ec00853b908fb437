"""The fused L1 / Huber steps against the fp64 oracle BIT FOR BIT on rounding-free data (tests/loss_reference.py robust_case: exact_data.exact_case with
targets whose fp32 loss gradient is a short dyadic number; exact_data.check_exact proves closure and coverage on the host before the reference is used).

Asserted, as tests/test_exact_gpu.py asserts them for the MSE step (its comparisons are reused): the output, every hidden state the plan computes and every
gradient are the oracle's bits; the loss within that file's LOSS_RTOL (2e-7).  Every copy of the loss tail is reached:
  * Huber on A1-C2 h = 128, L = 3, three channels (the 4-channel tail) at 17 and 33 windows (one / two whole 16-window tiles plus a one-window tail), plans
    bf16, x3 and f32, on every kernel-set switch that picks another tail copy: the default (bf16: a call at L1 / Huber runs the interpreting slab kernels -- the
    tails compiled for a program are MSE only, csrc/mshgnn_launch.hpp stack_query -- so the plan's program serves the forward of the two-call route below and
    the interpreter its backward_mse; x3: the program's kernels), MSHGNN_SPEC=0 (the same interpreting kernels, chosen by the plan),
    MSHGNN_STEP_KERNEL=0 (forward with the fused tail + backward launch), MSHGNN_SLAB=0 (8-wave stack kernels), MSHGNN_FUSED=0 (k_dec_bwd); and chunked,
    MSHGNN_STEP_CHUNK=16 at 48 windows: three sub-steps that scale by the whole batch and accumulate loss and gradient.
  * L1 on A1-C2 with grf_dimension = 1 (n = 4 B, a power of two) at 16 and 32 windows, same plans and switches.
  * Huber on Solo-K4 centroidal momentum, six channels (the 8-channel tail), 17 windows.
  * The generic engine (k_gdec_bwd): A1-C2 at hidden 256 on bf16 and x3, MSHGNN_ENGINE=generic at hidden 128, and a PaddedEngine (hidden 200).
  * backward_mse after forward, step_mse_phase (phases 0 and 1) and the fp64-source step: the oracle's bits, hence the one-call step's.
  * set("huber") then set("mse") gives the bits of a fresh engine's MSE step, and the getter follows.
Every test fails on a library without mshgnn_plan_set_regression_loss.
"""
from functools import lru_cache

import numpy as np
import pytest
import torch

from morphsym_hgnn_amd import engine as eng
from tests import exact_data as xd
from tests import helpers
from tests import loss_reference as lr
from tests import test_exact_gpu as gx

pytestmark = pytest.mark.gpu

_K1 = dict(rel_scales=(1.0,))
MODELS = {      # spec arguments (helpers.make_spec), loss kind, the seed the host search found per batch size (tests/test_loss_reference.py runs the first of each)
    "a1c2_L3": dict(spec=("c2", "a1-c2", "a1-c2", 128, 3, True, 3), kind="huber", seeds={17: 3, 33: 3, 48: 3}),
    "a1c2_g1_L3": dict(spec=("c2", "a1-c2", "a1-c2", 128, 3, True, 1), kind="l1", seeds={16: 4, 32: 8}),
    "solok4_com_L4": dict(spec=("k4_com", "solo-k4-com", "solo-k4", 128, 4, True, 1), kind="huber", seeds={17: 3}),
    "a1c2_h256_L3": dict(spec=("c2", "a1-c2", "a1-c2", 256, 3, True, 3), kind="huber", seeds={17: 6}),
    "a1c2_h200_L3": dict(spec=("c2", "a1-c2", "a1-c2", 200, 3, True, 3), kind="huber", seeds={17: 3}),
}
KERNEL_SETS = [      # (name, plan dtype, switches): every switch that picks another copy of the loss tail
    ("bf16", "bf16", {}),
    ("bf16 MSHGNN_SPEC=0", "bf16", {"MSHGNN_SPEC": "0"}),
    ("bf16 MSHGNN_STEP_KERNEL=0", "bf16", {"MSHGNN_STEP_KERNEL": "0"}),
    ("bf16 MSHGNN_SLAB=0", "bf16", {"MSHGNN_SLAB": "0"}),
    ("bf16 MSHGNN_FUSED=0", "bf16", {"MSHGNN_FUSED": "0"}),
    ("x3", "x3", {}),
    ("x3 MSHGNN_SPEC=0", "x3", {"MSHGNN_SPEC": "0"}),
    ("f32", "f32", {}),
]
SWITCHES = gx.SWITCHES + ("MSHGNN_STEP_KERNEL",)


@lru_cache(maxsize=3)
def _reference(model, B):
    m = MODELS[model]
    spec = helpers.make_spec(*m["spec"])
    case = lr.robust_case(spec, B, m["seeds"][B], m["kind"], **_K1)
    stats = {}
    ref = lr.check_robust(spec, case, stats=stats)
    ref["hidden"] = [h.float() for h in ref["hidden"]]
    return spec, case, ref, stats


def _engine(monkeypatch, spec, dtype, env, case):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    e = eng.make_engine(spec, dtype)          # (the switches are read when the plan is created)
    assert e.regression_loss == ("mse", 1.0), "a fresh plan is MSE"
    e.set_regression_loss(case["kind"], case["delta"])
    assert e.regression_loss == (case["kind"], float(torch.tensor(case["delta"], dtype=torch.float32)) if case["kind"] == "huber" else 1.0)
    return e


def _y(e, case):
    return case["y"].to(e.device, torch.float32).contiguous()


def _step(bad, name, e, spec, case, ref, B, hidden=True, xs=None):
    flat = eng.flatten_params(spec, case["params"], e.device)
    out, loss, g = e.step_mse(e.cast_inputs(case["x"]) if xs is None else xs, flat, _y(e, case), B)
    torch.cuda.synchronize()
    gx._compare(bad, f"{name} out", out, ref["out"])
    if hidden:
        gx._compare_hidden(bad, name, e, spec, ref, B, range(spec.num_layers))
    gx._compare_grads(bad, name, spec, g, ref)
    gx._compare_loss(bad, name, loss, ref)
    return out, loss, g


def _run_sets(monkeypatch, model, B, sets=KERNEL_SETS):
    spec, case, ref, stats = _reference(model, B)
    bad = []
    for name, dtype, env in sets:
        e = _engine(monkeypatch, spec, dtype, env, case)
        _step(bad, f"{model} {case['kind']} B={B} {name} step", e, spec, case, ref, B)
        del e
    print(f"\n{model} {case['kind']} B={B}: delta {case['delta']!r}, loss {ref['loss']!r}, {stats['nonzero_gout']} of {stats['gout']} output gradients non-zero, "
          f"{stats['zero_decisions']} exact-zero relu pre-activations")
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("B", [17, 33])
def test_huber_step_is_the_oracle_bit_for_bit_on_every_kernel_set(monkeypatch, B):
    _run_sets(monkeypatch, "a1c2_L3", B)


@pytest.mark.parametrize("B", [16, 32])
def test_l1_step_is_the_oracle_bit_for_bit_on_every_kernel_set(monkeypatch, B):
    _run_sets(monkeypatch, "a1c2_g1_L3", B)


@pytest.mark.parametrize("dtype", ["bf16", "x3"])
def test_chunked_huber_step_scales_by_the_whole_batch(monkeypatch, dtype):
    """MSHGNN_STEP_CHUNK=16 at 48 windows: three sub-steps.  inv_n and delta's branch are those of the whole batch; the sub-steps' loss and gradient add up."""
    model, B = "a1c2_L3", 48
    spec, case, ref, _ = _reference(model, B)
    e = _engine(monkeypatch, spec, dtype, {"MSHGNN_STEP_CHUNK": "16"}, case)
    bad = []
    _step(bad, f"{dtype} chunked huber", e, spec, case, ref, B, hidden=False)      # (the workspace holds the last sub-step only)
    assert not bad, "\n".join(bad[:20])


def test_huber_on_the_eight_channel_tail(monkeypatch):
    """Solo-K4 centroidal momentum: six output channels per base node."""
    _run_sets(monkeypatch, "solok4_com_L4", 17, [KERNEL_SETS[0], KERNEL_SETS[1], KERNEL_SETS[4], KERNEL_SETS[5]])


def test_huber_on_the_generic_engine(monkeypatch):
    """k_gdec_bwd: hidden 256 (bf16 and x3), the generic engine forced at hidden 128, and a padded width (200 -> 256)."""
    bad = []
    for model, dtype, env, padded in (("a1c2_h256_L3", "bf16", {}, False), ("a1c2_h256_L3", "x3", {}, False),
                                      ("a1c2_L3", "bf16", {"MSHGNN_ENGINE": "generic"}, False), ("a1c2_h200_L3", "bf16", {}, True)):
        spec, case, ref, _ = _reference(model, 17)
        e = _engine(monkeypatch, spec, dtype, env, case)
        assert e.generic and isinstance(e, eng.PaddedEngine) == padded, (model, dtype, env)
        out, _, _ = _step(bad, f"{model} {dtype} {env} generic huber", e, spec, case, ref, 17)
        gx._compare_loss(bad, f"{model} {dtype} reg_loss", e.reg_loss(out.reshape(-1), _y(e, case).reshape(-1), want_grad=False)[0], ref)
        del e
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("dtype,env", [("bf16", {}), ("x3", {}), ("f32", {})])
def test_two_call_two_phase_and_fp64_source_routes(monkeypatch, dtype, env):
    """forward + backward_mse, step_mse_phase (0 then 1) and the fp64-source step: the oracle's bits -- and so the one-call step's, compared directly too."""
    model, B = "a1c2_L3", 17
    spec, case, ref, _ = _reference(model, B)
    e = _engine(monkeypatch, spec, dtype, env, case)
    bad = []
    flat = eng.flatten_params(spec, case["params"], e.device)
    xs = e.cast_inputs(case["x"])
    y = _y(e, case)
    out1, loss1, g1 = _step(bad, f"{dtype} step", e, spec, case, ref, B)
    out1, loss1, g1 = out1.clone(), loss1.clone(), g1.clone()
    # backward_mse after forward
    out = e.forward(xs, flat, B, training=True).clone()
    loss, g = e.backward_mse(xs, flat, out, y, B)
    torch.cuda.synchronize()
    gx._compare(bad, f"{dtype} forward out", out, ref["out"])
    gx._compare_grads(bad, f"{dtype} backward_mse", spec, g, ref)
    gx._compare_loss(bad, f"{dtype} backward_mse", loss, ref)
    assert torch.equal(g, g1) and torch.equal(out, out1), "backward_mse after forward != the one-call step"
    # Engine.reg_loss, the loss of the two-call routes (mshgnn_regression_loss at the plan's kind): the mirror's gradient bits, the reference's loss
    lo, go = e.reg_loss(out.reshape(-1), y.reshape(-1))
    gm, _ = lr.mirror32(case["kind"], out.cpu().numpy(), y.cpu().numpy(), delta=case["delta"])
    assert np.array_equal(go.cpu().numpy().view(np.uint32), gm.view(np.uint32)), "reg_loss: the gradient is not the mirror's"
    gx._compare_loss(bad, f"{dtype} reg_loss", lo, ref)
    # the two-phase step
    if e.info.grad_split >= 0:
        o2 = torch.empty(B * e.n_out, spec.out_channels, dtype=torch.float32, device=e.device)
        g2 = torch.empty(spec.flat_size(), dtype=torch.float32, device=e.device)
        l2 = torch.empty(1, dtype=torch.float32, device=e.device)
        e.step_mse_phase(0, xs, flat, y, B, o2, g2, l2)
        e.step_mse_phase(1, xs, flat, y, B, o2, g2, l2)
        torch.cuda.synchronize()
        assert torch.equal(g2, g1) and torch.equal(o2.reshape(-1), out1.reshape(-1)) and torch.equal(l2, loss1), "step_mse_phase != the one-call step"
    else:
        assert dtype == "f32", "only the fp32 plan has no two-phase split here"
    # the fp64-source step (mshgnn_step_mse_src): equal to cast-then-step
    if dtype != "f32":
        xs64 = e.cast_inputs({t: v.to(e.device) for t, v in case["x"].items()})
        assert isinstance(xs64, eng.WideInputs), "the fp64-source route"
        o3, l3, g3 = _step(bad, f"{dtype} step_mse_src", e, spec, case, ref, B, xs=xs64)
        assert torch.equal(g3, g1) and torch.equal(o3, out1) and torch.equal(l3, loss1), "step_mse_src != cast-then-step"
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("dtype", ["bf16", "x3", "f32"])
def test_setter_round_trip_restores_the_mse_step(monkeypatch, dtype):
    """set("huber") then set("mse"): the bits of a fresh engine's MSE step (which the existing exact tests pin to the oracle; compared with it here as well)."""
    B = 17
    spec, case, ref, _ = gx._reference("a1c2_L3", B)      # the MSE case of tests/test_exact_gpu.py
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    fresh, e = eng.make_engine(spec, dtype), eng.make_engine(spec, dtype)
    flat = eng.flatten_params(spec, case["params"], e.device)
    y = case["y"].to(e.device, torch.float32).contiguous()
    want = [t.clone() for t in fresh.step_mse(fresh.cast_inputs(case["x"]), flat, y, B)]
    e.set_regression_loss("huber", 0.125)
    other = [t.clone() for t in e.step_mse(e.cast_inputs(case["x"]), flat, y, B)]
    assert e.regression_loss == ("huber", 0.125)
    e.set_regression_loss("mse")
    assert e.regression_loss == ("mse", 1.0)
    got = e.step_mse(e.cast_inputs(case["x"]), flat, y, B)
    torch.cuda.synchronize()
    for a, b, what in zip(got, want, ("out", "loss", "grad")):
        assert torch.equal(a, b), f"{dtype}: {what} after the round trip != a fresh engine's"
    assert torch.equal(other[0], want[0]) and not torch.equal(other[2], want[2]), "the Huber step in between: same forward, another gradient"
    bad = []
    gx._compare(bad, "out", got[0], ref["out"])
    gx._compare_grads(bad, "mse step", spec, got[2], ref)
    assert not bad, "\n".join(bad[:20])
    for kind, delta in (("nope", 1.0), ("huber", 0.0), ("huber", float("nan"))):
        with pytest.raises(ValueError):
            e.set_regression_loss(kind, delta)
    assert e.lib.mshgnn_plan_set_regression_loss(e._plan, 9, 1.0) == -1 and "mshgnn_plan_set_regression_loss" in e.lib.mshgnn_last_error().decode()
    assert e.lib.mshgnn_plan_set_regression_loss(e._plan, 2, float("inf")) == -1 and "delta" in e.lib.mshgnn_last_error().decode()
    assert e.regression_loss == ("mse", 1.0), "a refused setting changes nothing"
