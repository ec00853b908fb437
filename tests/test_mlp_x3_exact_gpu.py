"""GPU: the fused MLP on the split-bf16 parity plan (engine.MLPEngine(dtype="x3"), the k_mlp_*_x3 kernels) against the fp64 reference BIT FOR BIT on the
rounding-free families of tests/mlp_x3_reference.py (tests/test_mlp_x3_reference.py proves closure and coverage of every case on the host): operands with
non-zero lo halves whose every product has one factor with lo = 0, so the dropped lo lo term is zero.  Per family, row of mr.EXACT_MATRIX and batch: the
one-call step (MSE from y), forward + backward(gout) and the inference forward must give `out`, the input-layer stash (hi + lo) and every dW / db of fp64,
every bit; the loss may be 1e-6 relative off (a handful of fp32 roundings of an exact sum).  Sentinels sit behind `out`, the gradient buffer and the
workspace (filled with 0xFF), and a second run must reproduce every bit."""
import functools

import pytest
import torch

from tests import mlp_reference as mr
from tests import mlp_x3_reference as xr

pytestmark = pytest.mark.gpu

CASES = [(f, row[:5], B) for row in mr.EXACT_MATRIX for B in row[5] for f in xr.FAMILIES if not (f == "wide_w2" and row[3] < 3)]
PAD = 64


@functools.lru_cache(maxsize=None)
def _engine(in_channels, hidden, num_layers, out_channels):
    from morphsym_hgnn_amd import engine
    return engine.MLPEngine(in_channels, hidden, out_channels, num_layers, "x3", "cuda:0")


def _grads(flat, dims):
    return mr.unflatten(flat, mr.layer_dims(*dims))


def _guarded(n, dtype, dev, fill):
    t = torch.full((n + PAD,), fill, dtype=dtype, device=dev)
    return t, t[:n]


@pytest.mark.parametrize("family,shape,B", CASES, ids=[f"{f}_in{s[0]}_h{s[2]}_L{s[3]}_o{s[4]}_B{B}" for f, s, B in CASES])
def test_fused_x3_mlp_reproduces_fp64_bit_for_bit(family, shape, B):
    in_channels, T, hidden, L, out_channels = shape
    dev = torch.device("cuda:0")
    case = xr.family_case(family, in_channels, T, hidden, L, out_channels, B)
    ref_mse, _ = xr.check_family(case, "gout_mse")
    ref_g, _ = xr.check_family(case, "gout")
    dims = (in_channels, hidden, out_channels, L)
    e = _engine(in_channels, hidden, L, out_channels)
    flat = mr.flatten(case["params"]).float().to(dev)
    assert torch.equal(flat.double().cpu(), mr.flatten(case["params"]))
    x = e.cast_input(case["x"])
    assert x.dtype == torch.float32 and torch.equal(x[:, :in_channels].double().cpu(), case["x"])
    y = case["y"].float().to(dev).contiguous()
    n_out = B * out_channels

    ws_bytes = e.workspace_bytes(B, True)
    ws_full = torch.full((ws_bytes + 256,), 0xFF, dtype=torch.uint8, device=dev)
    ws_full[ws_bytes:] = 0xA5
    ws = ws_full[:ws_bytes]
    out_full, out = _guarded(n_out, torch.float32, dev, -7.5)
    g_full, grad = _guarded(e.n_flat, torch.float32, dev, -7.5)

    def check_guards():
        assert bool((ws_full[ws_bytes:] == 0xA5).all()), "the workspace sentinel was overwritten"
        assert bool((out_full[n_out:] == -7.5).all()) and bool((g_full[e.n_flat:] == -7.5).all()), "a sentinel behind out / grad was overwritten"

    # (1) the one-call step
    o1, loss1, g1 = e.step_mse(x, flat, y, out=out.view(B, out_channels), grad_flat=grad, workspace=ws)
    torch.cuda.synchronize()
    check_guards()
    stash1 = e.stash(B, 1, ws).clone()
    assert stash1.dtype == torch.float32
    bad = mr.compare(ref_mse, o1.view(B, out_channels), stash1, _grads(g1, dims), f"{family} step: ")
    assert not bad, bad
    want_loss = float(((ref_mse["out"] - case["y"]) ** 2).mean())
    assert abs(float(loss1) - want_loss) <= 1e-6 * max(abs(want_loss), 1e-30), (float(loss1), want_loss)
    o1, g1, l1 = o1.clone(), g1.clone(), loss1.clone()

    # (2) forward + backward(gout) with the same gradient: the step's bits; with another gradient: the reference's
    o2 = e.forward(x, flat, True, workspace=ws)
    g2 = e.backward(x, flat, case["gout_mse"].float().to(dev).contiguous(), workspace=ws)
    assert torch.equal(o2.view(-1), o1.view(-1)) and torch.equal(g2, g1) and torch.equal(e.stash(B, 1, ws), stash1), "forward + backward differs from the step"
    g3 = e.backward(x, flat, case["gout"].float().to(dev).contiguous(), workspace=ws)
    bad = mr.compare(ref_g, o2.view(B, out_channels), None, _grads(g3, dims), f"{family} forward + backward: ")
    assert not bad, bad

    # (3) the inference forward (no stashes), (4) a second run reproduces every bit
    o6 = e.forward(x, flat, False)
    assert torch.equal(o6.view(-1), o1.view(-1))
    ws_full[:ws_bytes] = 0xFF
    o7, loss7, g7 = e.step_mse(x, flat, y, workspace=ws)
    assert torch.equal(o7.view(-1), o1.view(-1)) and torch.equal(g7, g1) and torch.equal(loss7, l1)
    torch.cuda.synchronize()
    check_guards()
