"""GPU: the L1 / Huber tail of the fused MLP step (k_mlp_stack, csrc/mshgnn_mlp.hip) against the fp64 reference BIT FOR BIT, on the rounding-free data of
tests/mlp_reference.py / tests/mlp_x3_reference.py handed the loss gradient of tests/loss_reference.py (their check_exact / check_family prove closure and
coverage for that gradient on the host).

models.MLP's engine (engine.MLPEngine) on the bf16 and the split (x3) plan, hidden 128, a narrow input (24 = 8 columns x 3 steps), 3 layers:
  * Huber, 12 outputs, B in {31, 32, 33}: around the 32-row tile (31: a ragged only tile, 33: a whole tile and a one-row tail);
  * L1, 4 outputs, B in {32, 64}: sign(d) / n is a short dyadic number only where n = 4 B is a power of two, so the ragged batches 31 and 33 cannot be pinned
    bit for bit with L1 -- the tile edge of this tail is Huber's to hold (the same code: one call of reg_loss_terms per element).
    At B in {31, 33} L1 is held on the ragged tile a second way (test_l1_on_the_ragged_tile...): the step's gradients are, bit for bit, forward + backward of
    the fp32 mirror's L1 gradient -- the same kernels after the tail, so any wrong sign, a wrong 1 / n or a row of the ragged tile taken or dropped shows -- and
    the loss is exact quarters summed, within 1e-6.
Asserted: out, the input-layer stash and every dW / db are fp64's bits; the loss within 1e-6 (the bound of tests/test_mlp_exact_gpu.py); forward +
backward(the mirror's gradient) gives the step's bits; on the bf16 plan the series form equals the dense form bit for bit; set("mse") afterwards restores the
MSE step of a fresh engine.
"""
import functools

import numpy as np
import pytest
import torch

from tests import loss_reference as lr
from tests import mlp_reference as mr
from tests import mlp_x3_reference as xr

pytestmark = pytest.mark.gpu

SHAPE = dict(huber=(24, 3, 128, 3, 12), l1=(24, 3, 128, 3, 4))      # in_channels, history, hidden, layers, out_channels
CASES = [("huber", 31), ("huber", 32), ("huber", 33), ("l1", 32), ("l1", 64)]
TILE = 32


@functools.lru_cache(maxsize=None)
def _case(kind, B, dtype):
    in_channels, T, hidden, L, out_channels = SHAPE[kind]
    case = mr.exact_case(in_channels, T, hidden, L, out_channels, B) if dtype == "bf16" else xr.family_case(xr.FAMILIES[0], in_channels, T, hidden, L, out_channels, B)
    out = mr.reference(case["params"], case["x"])["out"].reshape(-1)
    y, cls, delta = lr.robust_targets(kind, out, out_channels, out_channels, tile=TILE, seed=1)
    g, _ = lr.mirror32(kind, out.numpy(), y.numpy(), delta=delta)
    case["y_reg"], case["gout_reg"] = y.view(B, out_channels), torch.from_numpy(g.astype(np.float64)).view(B, out_channels)
    case["delta"], case["loss_reg"] = delta, lr.ref64(kind, out, y, delta)[0]
    ref = mr.check_exact(case, "gout_reg") if dtype == "bf16" else xr.check_family(case, "gout_reg")[0]
    return case, ref


@pytest.mark.parametrize("dtype", ["bf16", "x3"])
@pytest.mark.parametrize("kind,B", CASES)
def test_fused_mlp_robust_step_reproduces_fp64_bit_for_bit(kind, B, dtype):
    from morphsym_hgnn_amd import engine, windows
    in_channels, T, hidden, L, out_channels = SHAPE[kind]
    dev = torch.device("cuda:0")
    case, ref = _case(kind, B, dtype)
    dims = (in_channels, hidden, out_channels, L)
    e = engine.MLPEngine(in_channels, hidden, out_channels, L, dtype, dev)
    fresh = engine.MLPEngine(in_channels, hidden, out_channels, L, dtype, dev)
    assert e.regression_loss == ("mse", 1.0)
    e.set_regression_loss(kind, case["delta"])
    assert e.regression_loss[0] == kind
    flat = mr.flatten(case["params"]).float().to(dev)
    x = e.cast_input(case["x"])
    y = case["y_reg"].float().to(dev).contiguous()

    o1, loss1, g1 = e.step_mse(x, flat, y)
    torch.cuda.synchronize()
    stash1 = e.stash(B, 1).clone()
    bad = mr.compare(ref, o1.view(B, out_channels), stash1, mr.unflatten(g1, mr.layer_dims(*dims)), f"{dtype} {kind} step: ")
    assert not bad, bad
    assert abs(float(loss1) - case["loss_reg"]) <= 1e-6 * abs(case["loss_reg"]), (float(loss1), case["loss_reg"])
    o1, g1, l1 = o1.clone(), g1.clone(), loss1.clone()

    # forward + backward of the mirror's gradient: the step's bits
    o2 = e.forward(x, flat, True)
    g2 = e.backward(x, flat, case["gout_reg"].float().to(dev).contiguous())
    assert torch.equal(o2.view(-1), o1.view(-1)) and torch.equal(g2, g1), "forward + backward(mirror gradient) differs from the step"

    # the series form on the same windows (the bf16 plan has one; an x3 engine assembles and runs the dense form)
    ncols = in_channels // T
    store = windows.SequenceStore({"s": case["series"].numpy()}, windows.mlp_recipe([("s", list(range(ncols)))], T), dtype="bf16", device=dev)
    _, o4, loss4, g4 = e.step_mse_series(store, case["starts"].to(dev), flat, targets=y)
    torch.cuda.synchronize()
    assert torch.equal(o4.view(-1), o1.view(-1)) and torch.equal(g4, g1) and torch.equal(loss4, l1), "the series form differs from the dense form"

    # a second run, then back to MSE: a fresh engine's bits
    o5, loss5, g5 = e.step_mse(x, flat, y)
    assert torch.equal(o5.view(-1), o1.view(-1)) and torch.equal(g5, g1) and torch.equal(loss5, l1)
    e.set_regression_loss("mse")
    got, want = e.step_mse(x, flat, y), fresh.step_mse(fresh.cast_input(case["x"]), flat, y)
    torch.cuda.synchronize()
    assert all(torch.equal(a.view(-1), b.view(-1)) for a, b in zip(got, want)), "set('mse') does not restore the MSE step"
    assert not torch.equal(got[2], g1)


@pytest.mark.parametrize("dtype", ["bf16", "x3"])
@pytest.mark.parametrize("B", [31, 33])
def test_l1_on_the_ragged_tile_is_forward_plus_backward_of_the_mirror_gradient(B, dtype):
    """n = 4 B is no power of two here, so sign(d) / n is not dyadic and fp64 cannot be matched bit for bit; what the tail hands the backward sweep can: the
    mirror's fp32 gradient.  Targets: y = out -+ quarters and y == out, every class in the one-row tail (B = 33) and in the ragged only tile (B = 31)."""
    from morphsym_hgnn_amd import engine
    in_channels, T, hidden, L, out_channels = SHAPE["l1"]
    dev = torch.device("cuda:0")
    case = mr.exact_case(in_channels, T, hidden, L, out_channels, B)
    out = mr.reference(case["params"], case["x"])["out"]
    k = torch.arange(B * out_channels).view(B, out_channels)
    cls = (k + k // out_channels) % 3
    u = 0.25 * (1 + k % 5).double()
    y = torch.where(cls == 1, out - u, torch.where(cls == 2, out + u, out))
    assert all(bool((cls[-1] == c).any()) for c in range(3)) and all(bool((cls[:, ch] == c).any()) for c in range(3) for ch in range(out_channels))
    gm, term = lr.mirror32("l1", out.numpy(), y.numpy())
    assert set(np.unique(gm).tolist()) == {float(-lr.inv_n32(gm.size)), 0.0, float(lr.inv_n32(gm.size))}
    e = engine.MLPEngine(in_channels, hidden, out_channels, L, dtype, dev)
    e.set_regression_loss("l1")
    flat = mr.flatten(case["params"]).float().to(dev)
    x = e.cast_input(case["x"])
    o1, loss1, g1 = [t.clone() for t in e.step_mse(x, flat, y.float().to(dev).contiguous())]
    assert torch.equal(o1.view(B, out_channels).double().cpu(), out)
    want = float(term.astype(np.float64).sum()) / gm.size
    assert abs(float(loss1) - want) <= 1e-6 * want, (float(loss1), want)
    o2 = e.forward(x, flat, True)
    g2 = e.backward(x, flat, torch.from_numpy(gm).view(B, out_channels).to(dev).contiguous())
    torch.cuda.synchronize()
    assert torch.equal(o2.view(-1), o1.view(-1)) and torch.equal(g2, g1) and bool(g1.any()), "the L1 step differs from forward + backward(mirror gradient)"
    damaged = e.backward(x, flat, torch.from_numpy(lr.mirror32("l1", out.numpy(), y.numpy(), n_total=4 * 32)[0]).view(B, out_channels).to(dev).contiguous())
    assert not torch.equal(damaged, g1), "a gradient scaled by another batch's 1 / n must not pass"
