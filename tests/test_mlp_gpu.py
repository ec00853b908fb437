"""GPU: the fused MLP on random data against the rounding-point emulation and the fp64 reference (tests/mlp_reference.py), the operator route of models.MLP,
the series methods' fallback (standardised recipes, `transformed` / `orbit` stores: assemble, then the dense form -- bit for bit) and HIP-graph capture of
the series step.  Bounds: the project's for this arithmetic class (tests/test_bf16_emulation.py: output 4e-3 max-abs relative, gradients 1.5e-2 L2 relative per
tensor against the emulation; forward 2e-2 against fp64, the bound smoke() uses for the bf16 plan; the operator route 1e-4 against fp64)."""
import functools

import pytest
import torch
from torch import nn

from tests import mlp_reference as mr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B = 1000
OUT_TOL, GRAD_TOL, FWD64_TOL, OPS_TOL = 4e-3, 1.5e-2, 2e-2, 1e-4


@functools.lru_cache(maxsize=None)
def _case(in_channels, hidden, L, out_channels=8):
    """random data + the emulation's and the reference's results for both losses, computed once"""
    c = mr.random_case(in_channels, hidden, out_channels, L, B, seed=in_channels + L)
    c["em_mse"] = mr.emulate(c["params"], c["x"], loss="mse", target=c["y"])
    c["em_ce"] = mr.emulate(c["params"], c["x"], loss="ce", target=c["labels"])
    c["ref"] = mr.reference(c["params"], c["x"])
    return c


def _engine(in_channels, hidden, L, out_channels=8):
    from morphsym_hgnn_amd import engine
    return engine.MLPEngine(in_channels, hidden, out_channels, L, "bf16", DEV)


@pytest.mark.parametrize("loss", ["mse", "ce"])
@pytest.mark.parametrize("in_channels,hidden,L", [(450, 128, 3), (450, 128, 8), (8100, 128, 8)])
def test_step_against_the_emulation(in_channels, hidden, L, loss):
    c = _case(in_channels, hidden, L)
    e = _engine(in_channels, hidden, L)
    flat = mr.flatten(c["params"]).float().to(DEV)
    x = e.cast_input(c["x"])
    if loss == "mse":
        out, lv, g = e.step_mse(x, flat, c["y"].float().to(DEV).contiguous())
    else:
        out, lv, g = e.step_ce(x, flat, c["labels"].to(DEV).contiguous())
    em = c["em_" + loss]
    errs = {"out": mr.rel_max(out, em["out"]), "loss": abs(float(lv) - float(em["loss"])) / abs(float(em["loss"]))}
    for i, ((dW, db), (eW, eb)) in enumerate(zip(mr.unflatten(g, mr.layer_dims(in_channels, hidden, 8, L)), em["grads"])):
        errs[f"dW{i}"], errs[f"db{i}"] = mr.rel_l2(dW, eW), mr.rel_l2(db, eb)
    print(in_channels, hidden, L, loss, {k: f"{v:.2e}" for k, v in errs.items()})
    assert errs["out"] < OUT_TOL and errs["loss"] < OUT_TOL, errs
    assert all(v < GRAD_TOL for k, v in errs.items() if k[0] == "d"), errs


def test_forward_against_fp64():
    c = _case(450, 128, 3)
    e = _engine(450, 128, 3)
    out = e.forward(e.cast_input(c["x"]), mr.flatten(c["params"]).float().to(DEV), training=False)
    err = mr.rel_max(out, c["ref"]["out"])
    print("forward vs fp64 (450, 128, L 3):", f"{err:.2e}")
    assert err < FWD64_TOL, err


@pytest.mark.parametrize("activation", [None, nn.LeakyReLU(0.1)], ids=["relu-f32", "leaky"])
def test_operator_route_against_fp64(activation):
    from morphsym_hgnn_amd import models
    torch.manual_seed(5)
    m = models.MLP(450, 128, 8, 3, activation_fn=activation if activation is not None else nn.ReLU()).to(DEV).set_precision("f32")
    assert not m._fused()
    ref = mr.sequential(450, 128, 8, 3, activation).double()
    ref.load_state_dict({k: v.double().cpu() for k, v in m.state_dict().items()})
    g = torch.Generator().manual_seed(9)
    x, gout = torch.randn(257, 450, generator=g, dtype=torch.float64), torch.randn(257, 8, generator=g, dtype=torch.float64)
    out = m(x.float().to(DEV))
    (out * gout.float().to(DEV)).sum().backward()
    want = ref(x)
    (want * gout).sum().backward()
    assert mr.rel_max(out.detach(), want.detach()) < OPS_TOL
    for (k, p), q in zip(m.named_parameters(), ref.parameters()):
        assert mr.rel_l2(p.grad, q.grad) < OPS_TOL, k


def test_module_routes_to_the_fused_engine_with_autograd():
    """models.MLP at precision "bf16": forward + autograd backward are MLPEngine.forward(training) + mshgnn_mlp_backward -- the engine's own bits."""
    from morphsym_hgnn_amd import models
    torch.manual_seed(6)
    m = models.MLP(450, 128, 8, 3).to(DEV).set_precision("bf16")
    assert m._fused()
    g = torch.Generator().manual_seed(10)
    x, gout = mr.bf16(torch.randn(65, 450, generator=g, dtype=torch.float64)), torch.randn(65, 8, generator=g).to(DEV)
    out = m(x.to(DEV))
    (out * gout).sum().backward()
    e = _engine(450, 128, 3)
    flat = torch.cat([p.detach().reshape(-1) for p in m.parameters()]).contiguous()
    xs = e.cast_input(x)
    o2 = e.forward(xs, flat, training=True)
    g2 = e.backward(xs, flat, gout.contiguous())
    assert torch.equal(out.detach(), o2)
    assert torch.equal(torch.cat([p.grad.reshape(-1) for p in m.parameters()]), g2)


def _mc_store(history, normalize=False, dtype="bf16"):
    from morphsym_hgnn_amd import windows
    from tests import test_window_symmetry as ws
    recipe = windows.minicheetah_mlp_recipe(ws.JP, ws.FP, history, normalize)
    return windows.SequenceStore(ws.SEQ4, recipe, dtype=dtype, device=DEV), ws


@pytest.mark.parametrize("kind", ["plain", "standardised", "transformed", "orbit", "fp32-store"])
def test_series_methods_equal_assemble_then_dense(kind):
    """Where the library's series form applies ("plain") and where the engine falls back to assemble + dense (everything else): the same bits as
    `store.assemble` followed by the dense step / forward."""
    T = 20
    store, ws = _mc_store(T, normalize=(kind == "standardised"), dtype="f32" if kind == "fp32-store" else "bf16")
    elements = None
    if kind == "transformed":
        store = store.transformed("gs", ws.K4)
    if kind == "orbit":
        store = store.orbit(ws.K4)
    e = _engine(T * 54, 128, 3)
    assert e._series_ok(store) == (kind == "plain")
    torch.manual_seed(3)
    flat = mr.flatten([(m.weight.detach(), m.bias.detach()) for m in mr.sequential(T * 54, 128, 8, 3) if isinstance(m, nn.Linear)]).float().to(DEV)
    n = len(store)
    starts = torch.randint(0, n, (77,), generator=torch.Generator().manual_seed(2))
    starts[0], starts[-1] = 0, n - 1
    starts = starts.to(DEV)
    if kind == "orbit":
        starts = store.pack_starts(starts, (torch.arange(77) % store.n_elements).to(DEV))
    labels, out, loss, g = e.step_ce_series(store, starts, flat)
    out, loss, g, labels = out.clone(), loss.clone(), g.clone(), labels.clone()
    xs, y, _ = store.assemble(starts)
    x = xs[0] if xs[0].dtype == torch.bfloat16 else xs[0].to(torch.bfloat16)
    want_labels = (y != 0).to(torch.int32)
    o2, l2, g2 = e.step_ce(x, flat, want_labels.contiguous())
    assert torch.equal(labels, want_labels) and torch.equal(out, o2) and torch.equal(loss, l2) and torch.equal(g, g2)
    y3, _, li3, o3 = e.forward_series(store, starts, flat)
    assert torch.equal(o3, e.forward(x, flat, training=False)) and torch.equal(y3, y) and torch.equal(li3, want_labels)


def test_series_step_is_capturable_in_a_graph():
    """Three replays of a captured step_mse_series with fresh `starts` equal three eager steps bit for bit (no allocation, no host read inside the step)."""
    from morphsym_hgnn_amd import windows
    from tests import test_window_symmetry as ws
    T = 20
    recipe = windows.quadsdk_a1_mlp_recipe(ws.JP, ws.FP, T, 1)
    store = windows.SequenceStore(ws.SEQ, recipe, dtype="bf16", device=DEV)
    e = _engine(T * 42, 128, 3, 4)
    torch.manual_seed(4)
    flat = mr.flatten([(m.weight.detach(), m.bias.detach()) for m in mr.sequential(T * 42, 128, 4, 3) if isinstance(m, nn.Linear)]).float().to(DEV)
    n, Bs = len(store), 96
    batches = [torch.randint(0, n, (Bs,), generator=torch.Generator().manual_seed(s)).to(DEV) for s in range(4)]
    static = batches[0].clone()
    out, g, loss = torch.empty(Bs, 4, device=DEV), torch.empty(e.n_flat, device=DEV), torch.empty(1, device=DEV)
    e.step_mse_series(store, static, flat, out=out, grad_flat=g, loss=loss)      # warm-up: workspace, by-product buffers, run pointers resolved and vouched for
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        e.step_mse_series(store, static, flat, out=out, grad_flat=g, loss=loss)
    for st in batches[1:]:
        static.copy_(st)
        graph.replay()
        got = (out.clone(), g.clone(), loss.clone())
        _, o2, l2, g2 = e.step_mse_series(store, st, flat)
        assert torch.equal(got[0], o2) and torch.equal(got[1], g2) and torch.equal(got[2], l2)
