"""GPU: the fused MLP (engine.MLPEngine, csrc/mshgnn_mlp.hip) against the fp64 reference BIT FOR BIT on rounding-free data (tests/mlp_reference.py;
tests/test_mlp_reference.py proves closure and coverage of every case on the host).  Per row of the matrix and per batch: the one-call step, forward +
backward(gout), the dense form and the series form on the same windows (history as listed, starts that include row 0 and the last valid row) must give
the same `out`, input-layer stash and gradients as fp64, every bit; the loss may be 1e-6 relative off (a handful of fp32 roundings of an exact sum).
Sentinels sit behind `out`, the gradient buffer and the workspace (which is poisoned: MSHGNN_POISON_WS), and a second run must reproduce every bit."""
import functools

import pytest
import torch

from tests import mlp_reference as mr

pytestmark = pytest.mark.gpu

CASES = [(row[:5], B) for row in mr.EXACT_MATRIX for B in row[5]]
PAD = 64


@functools.lru_cache(maxsize=None)
def _engine(in_channels, hidden, num_layers, out_channels):
    from morphsym_hgnn_amd import engine
    return engine.MLPEngine(in_channels, hidden, out_channels, num_layers, "bf16", "cuda:0")


def _grads(flat, dims):
    return mr.unflatten(flat, mr.layer_dims(*dims))


def _guarded(n, dtype, dev, fill):
    t = torch.full((n + PAD,), fill, dtype=dtype, device=dev)
    return t, t[:n]


@pytest.mark.parametrize("shape,B", CASES, ids=[f"in{s[0]}_T{s[1]}_h{s[2]}_L{s[3]}_o{s[4]}_B{B}" for s, B in CASES])
def test_fused_mlp_reproduces_fp64_bit_for_bit(shape, B):
    from morphsym_hgnn_amd import windows
    in_channels, T, hidden, L, out_channels = shape
    dev = torch.device("cuda:0")
    case = mr.exact_case(in_channels, T, hidden, L, out_channels, B)
    ref_mse, ref_g = mr.check_exact(case, "gout_mse"), mr.check_exact(case, "gout")
    dims = (in_channels, hidden, out_channels, L)
    e = _engine(in_channels, hidden, L, out_channels)
    flat = mr.flatten(case["params"]).float().to(dev)
    x = e.cast_input(case["x"])
    y = case["y"].float().to(dev).contiguous()
    n_out = B * out_channels

    # guarded buffers: sentinels behind out, the gradient and the (poisoned) workspace
    ws_bytes = e.workspace_bytes(B, True)
    ws_full = torch.full((ws_bytes + 256,), 0xFF, dtype=torch.uint8, device=dev)
    ws_full[ws_bytes:] = 0xA5
    ws = ws_full[:ws_bytes]
    out_full, out = _guarded(n_out, torch.float32, dev, -7.5)
    g_full, grad = _guarded(e.n_flat, torch.float32, dev, -7.5)

    def check_guards():
        assert bool((ws_full[ws_bytes:] == 0xA5).all()), "the workspace sentinel was overwritten"
        assert bool((out_full[n_out:] == -7.5).all()) and bool((g_full[e.n_flat:] == -7.5).all()), "a sentinel behind out / grad was overwritten"

    # (1) the one-call step on dense rows
    o1, loss1, g1 = e.step_mse(x, flat, y, out=out.view(B, out_channels), grad_flat=grad, workspace=ws)
    torch.cuda.synchronize()
    check_guards()
    stash1 = e.stash(B, 1, ws).clone()
    bad = mr.compare(ref_mse, o1.view(B, out_channels), stash1, _grads(g1, dims), "step: ")
    assert not bad, bad
    want_loss = float(((ref_mse["out"] - case["y"]) ** 2).mean())
    assert abs(float(loss1) - want_loss) <= 1e-6 * max(abs(want_loss), 1e-30), (float(loss1), want_loss)
    o1, g1, l1 = o1.clone(), g1.clone(), loss1.clone()

    # (2) forward + backward(gout) with the same gradient: the same bits as the step; with another gradient: the reference's
    o2 = e.forward(x, flat, True, workspace=ws)
    g2 = e.backward(x, flat, case["gout_mse"].float().to(dev).contiguous(), workspace=ws)
    assert torch.equal(o2.view(-1), o1.view(-1)) and torch.equal(g2, g1) and torch.equal(e.stash(B, 1, ws), stash1), "forward + backward differs from the step"
    g3 = e.backward(x, flat, case["gout"].float().to(dev).contiguous(), workspace=ws)
    bad = mr.compare(ref_g, o2.view(B, out_channels), None, _grads(g3, dims), "forward + backward: ")
    assert not bad, bad

    # (3) the series form on the same windows
    ncols = in_channels // T
    store = windows.SequenceStore({"s": case["series"].numpy()}, windows.mlp_recipe([("s", list(range(ncols)))], T), dtype="bf16", device=dev)
    starts = case["starts"].to(dev)
    ws_full[:ws_bytes] = 0xFF
    _, o4, loss4, g4 = e.step_mse_series(store, starts, flat, out=out.view(B, out_channels), grad_flat=grad, workspace=ws, targets=y)
    torch.cuda.synchronize()
    check_guards()
    assert torch.equal(o4.view(-1), o1.view(-1)) and torch.equal(g4, g1) and torch.equal(loss4, l1) and torch.equal(e.stash(B, 1, ws), stash1), \
        "the series form differs from the dense form"
    _, _, _, o5 = e.forward_series(store, starts, flat, labels=False, training=True, workspace=ws)
    g5 = e.backward_series(store, starts, flat, case["gout_mse"].float().to(dev).contiguous(), workspace=ws)
    assert torch.equal(o5.view(-1), o1.view(-1)) and torch.equal(g5, g1), "series forward + backward differs from the step"
    o6 = e.forward(x, flat, False)      # the inference forward (no stashes)
    assert torch.equal(o6.view(-1), o1.view(-1))

    # (4) a second run reproduces every bit
    o7, loss7, g7 = e.step_mse(x, flat, y, workspace=ws)
    assert torch.equal(o7.view(-1), o1.view(-1)) and torch.equal(g7, g1) and torch.equal(loss7, l1)
    check_guards()
