"""The finalize ops that read no weight-gradient slab (zero fills of the dead slices, decoder sums, the fused loss) run in extra workgroups of the weight-gradient
launch on the bf16 and split plans, and k_finalize sums slabs from one record per workgroup (csrc/mshgnn_plan.hpp SIDE_INTS / FSLAB_INTS, gw_side_workgroup).
Nothing about the sums changed -- operands, grouping, order -- so every route still has to write every element of the caller's buffers:

  * the caller's gradient buffer and loss are pre-filled with NaN; afterwards every element is finite and every structurally dead slice (a parameter whose
    oracle gradient is exactly zero, an alignment gap of the flat buffer) is exactly +0.0;
  * one-call step == step_mse_phase 0 then 1, bit for bit, and after phase 0 alone grad_flat[grad_split:] and the loss are already final; two runs of a route
    are bit-equal; forward + backward_mse gives the step's output bits and its loss / gradients up to the summation order of the decoder partials
    (512 from k_dec_bwd against one per tile: the bounds of tests/test_engine_gpu.py::test_one_call_step_equals_forward_plus_backward);
  * the fp64 oracle (tests/helpers.run_engine_case / run_step_case, evaluated with the engine's relu decisions) at the plans' tolerances of
    tests/test_widths_gpu.py: 1e-4 on x3, 3e-2 on bf16;
  * a chunked step of two accumulating sub-steps (MSHGNN_STEP_CHUNK, read when the plan is created) against the whole step at the bounds of
    tests/test_step_chunks_gpu.py;
  * step_ce on the smallest MiniCheetah-K4 golden case.

Batches: 16 windows (one tile, one window part), 17 (ragged), 64, 1040 (several window parts)."""
import pytest
import torch

from tests import helpers

pytestmark = pytest.mark.gpu
RTOL = 1e-4          # x3
BF16_TOL = 3e-2      # bf16


def _tol(dtype):
    return (BF16_TOL, {"decision_tol": BF16_TOL}) if dtype == "bf16" else (RTOL, {})


def _assert_parity(errs, ref, tol, what):
    for k in sorted(errs):
        print(f"{what}: {k} {errs[k]:.3e}")
    bad = {k: v for k, v in errs.items() if not v <= tol}
    assert not bad, f"{what}: stages above {tol}: {bad}"
    assert errs["relu_decisions_outside_tolerance"] == 0.0, what


def _dead_mask(spec, ref_grads):
    """bool [flat_size]: True where nothing can reach the output -- parameters with an exact-zero oracle gradient and the gaps between parameters."""
    dead = torch.ones(spec.flat_size(), dtype=torch.bool)
    for k, (o, n) in spec.param_offsets().items():
        if float(ref_grads[k].abs().max()) != 0.0:
            dead[o:o + n] = False
    return dead


def _assert_written(g, loss, dead, what):
    g = g.detach().cpu()
    assert bool(torch.isfinite(g).all()), f"{what}: {int((~torch.isfinite(g)).sum())} gradient elements were not written"
    assert bool(torch.isfinite(loss.detach().cpu()).all()), f"{what}: the loss was not written"
    assert not bool(g[dead].view(torch.int32).any()), f"{what}: a dead slice is not exactly +0.0"


def _nan_buffers(e, spec, B):
    nan = float("nan")
    return (torch.full((B * e.n_out, spec.out_channels), nan, dtype=torch.float32, device=e.device),
            torch.full((spec.flat_size(),), nan, dtype=torch.float32, device=e.device), torch.full((1,), nan, dtype=torch.float32, device=e.device))


@pytest.mark.parametrize("dtype", ["bf16", "x3"])
@pytest.mark.parametrize("B", [16, 17, 64, 1040])
def test_every_route_writes_the_whole_gradient_and_agrees(dtype, B):
    from morphsym_hgnn_amd import engine as eng
    spec = helpers.make_spec("c2", "a1-c2", "a1-c2", 128, 3)
    x_dict, y, params = helpers.random_case(spec, B, 29)
    tol, kw = _tol(dtype)
    e = eng.Engine(spec, dtype)
    assert not e.generic
    # the fp64 oracle, forward + backward(gout) route
    errs, *_ = helpers.run_engine_case(spec, x_dict, y, params, spec.topology.edge_index_dict(B), B, dtype=dtype, engine=e, **kw)
    ref = helpers.run_engine_case.last_reference
    _assert_parity(errs, ref, tol, f"{dtype} B={B} forward + backward")
    dead = _dead_mask(spec, ref["grads"])
    assert bool(dead.any()) and not bool(dead.all())
    # ... and the one-call step
    errs, *_ = helpers.run_step_case(spec, x_dict, y, params, B, dtype=dtype, engine=e, **kw)
    _assert_parity(errs, helpers.run_step_case.last_reference, tol, f"{dtype} B={B} step_mse")

    xs = e.cast_inputs(x_dict)
    flat = eng.flatten_params(spec, params, e.device)
    yd = y.reshape(-1).to(e.device, torch.float32)
    # one-call step, twice
    out_a, g_a, loss_a = _nan_buffers(e, spec, B)
    e.step_mse(xs, flat, yd, B, out=out_a, grad_flat=g_a, loss=loss_a)
    out_r, g_r, loss_r = _nan_buffers(e, spec, B)
    e.step_mse(xs, flat, yd, B, out=out_r, grad_flat=g_r, loss=loss_r)
    torch.cuda.synchronize()
    _assert_written(g_a, loss_a, dead, "step_mse")
    assert torch.equal(out_a, out_r) and torch.equal(loss_a, loss_r) and torch.equal(g_a.view(torch.int32), g_r.view(torch.int32))
    # two-phase step: phase 0 leaves everything but the encoder's slice final, phase 1 the rest; bit for bit the one-call step
    split = int(e.info.grad_split)
    assert 0 < split < spec.flat_size()
    out_b, g_b, loss_b = _nan_buffers(e, spec, B)
    e.step_mse_phase(0, xs, flat, yd, B, out_b, g_b, loss_b)
    torch.cuda.synchronize()
    assert torch.equal(g_b[split:].view(torch.int32), g_a[split:].view(torch.int32)) and torch.equal(loss_b, loss_a) and torch.equal(out_b, out_a)
    assert bool(torch.isnan(g_b[:split]).all())           # the encoder's slice is untouched until phase 1
    e.step_mse_phase(1, xs, flat, yd, B, out_b, g_b, loss_b)
    torch.cuda.synchronize()
    assert torch.equal(g_b.view(torch.int32), g_a.view(torch.int32)) and torch.equal(loss_b, loss_a)
    # forward + backward_mse (decoder partials from k_dec_bwd), twice
    _, g_c, loss_c = _nan_buffers(e, spec, B)
    out_c = e.forward(xs, flat, B).clone()
    e.backward_mse(xs, flat, out_c, yd, B, grad_flat=g_c, loss=loss_c)
    _, g_d, loss_d = _nan_buffers(e, spec, B)
    out_d = e.forward(xs, flat, B)
    e.backward_mse(xs, flat, out_d, yd, B, grad_flat=g_d, loss=loss_d)
    torch.cuda.synchronize()
    _assert_written(g_c, loss_c, dead, "forward + backward_mse")
    assert torch.equal(out_c, out_a) and torch.equal(out_d, out_a)
    assert torch.equal(loss_c, loss_d) and torch.equal(g_c.view(torch.int32), g_d.view(torch.int32))
    assert abs(float(loss_c) - float(loss_a)) <= 1e-5 * abs(float(loss_a))
    assert float((g_c - g_a).abs().max() / g_a.abs().max()) < 2e-5


@pytest.mark.parametrize("dtype", ["bf16", "x3"])
def test_chunked_step_accumulates_into_a_prefilled_buffer(dtype, monkeypatch):
    """96 windows at MSHGNN_STEP_CHUNK=48: two sub-steps; the second one's launches add to what the first one wrote (no zero fills, decoder sums and loss accumulate)."""
    from morphsym_hgnn_amd import engine as eng
    spec = helpers.make_spec("c2", "a1-c2", "a1-c2", 128, 3)
    B = 96
    x_dict, y, params = helpers.random_case(spec, B, 31)
    res = {}
    for chunk in ("0", "48"):
        monkeypatch.setenv("MSHGNN_STEP_CHUNK", chunk)          # read when the plan is created
        e = eng.Engine(spec, dtype)
        assert not e.generic
        xs = e.cast_inputs(x_dict)
        flat = eng.flatten_params(spec, params, e.device)
        yd = y.reshape(-1).to(e.device, torch.float32)
        runs = []
        for _ in range(2):
            out, g, loss = _nan_buffers(e, spec, B)
            e.step_mse(xs, flat, yd, B, out=out, grad_flat=g, loss=loss)
            torch.cuda.synchronize()
            runs.append((out.cpu(), g.cpu(), loss.cpu()))
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(*runs))
        res[chunk] = runs[0]
    (out_w, g_w, loss_w), (out_c, g_c, loss_c) = res["0"], res["48"]
    gw, gc = eng.unflatten(spec, g_w), eng.unflatten(spec, g_c)
    dead = _dead_mask(spec, gw)
    _assert_written(g_w, loss_w, dead, "whole step")
    _assert_written(g_c, loss_c, dead, "chunked step")
    assert torch.equal(out_c, out_w)
    assert abs(float(loss_c) - float(loss_w)) <= 2e-6 * abs(float(loss_w))
    for k in gw:
        ref = float(gw[k].abs().max())
        if ref != 0.0:
            assert float((gc[k] - gw[k]).abs().max()) <= 4e-6 * ref, (k, float((gc[k] - gw[k]).abs().max()) / ref)
    assert not torch.equal(g_c, g_w)       # (it really ran in sub-steps: the summation order moved some bits)


@pytest.mark.parametrize("dtype", ["bf16", "x3"])
def test_cross_entropy_step_on_the_smallest_k4_case(dtype):
    from morphsym_hgnn_amd import engine as eng
    case, spec, fx, x_dict, y, params, ei = helpers.load_case("mck4_cls_h128_L2_B3")
    B = case["B"]
    tol, kw = _tol(dtype)
    e = eng.Engine(spec, dtype)
    errs, *_ = helpers.run_step_case(spec, x_dict, y, params, B, dtype=dtype, engine=e, **kw)
    ref = helpers.run_step_case.last_reference
    _assert_parity(errs, ref, tol, f"{dtype} step_ce")
    dead = _dead_mask(spec, ref["grads"])
    xs = e.cast_inputs(x_dict)
    flat = eng.flatten_params(spec, params, e.device)
    labels = y.reshape(B, spec.num_nodes[spec.out_type]).to(e.device, torch.int32).contiguous()
    runs = []
    for _ in range(2):
        _, g, loss = _nan_buffers(e, spec, B)
        out, loss, g = e.step_ce(xs, flat, labels, B, grad_flat=g, loss=loss)
        torch.cuda.synchronize()
        _assert_written(g, loss, dead, f"{dtype} step_ce")
        runs.append((out.cpu().clone(), g.cpu(), loss.cpu()))
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(*runs))
