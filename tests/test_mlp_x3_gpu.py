"""GPU: the fused MLP on the split-bf16 parity plan (engine.MLPEngine(dtype="x3")) on random fp32-valued data against the fp64 reference under the
engine's own ReLU decisions (the project's method for the HGNN, tests/helpers.py: the decisions are read from the stashes, the reference runs under them,
and every decision that differs from the reference's own must sit on a pre-activation that is zero to the arithmetic's resolution), the module surface at
the default precision, the wrappers on resident data, HIP-graph capture of the dense step and the refusal of the series form.

Bounds.  Output rel-max, loss and the L2-relative error of every gradient tensor: 1e-4, the project's parity tolerance (OPS_TOL of tests/test_mlp_gpu.py).
The fp64 emulation of the split arithmetic alone (tests/mlp_x3_reference.emulate_x3: 16-bit operands, no lo lo term) gives 7.8e-6 .. 1.6e-5 on these
shapes; the remaining factor of about 6 is for the fp32 accumulation, which that emulation does not model.  Flipped decisions: |z_ref| <= 1e-5 of the layer's
max |z| (the emulation gives at most 7e-7) and at most 1e-4 of the decisions (the emulation: at most 3 of 512 000).
Measured on one MI355X: worst error 7.9e-6 .. 1.5e-5 (MSE), 8.3e-6 .. 4.6e-5 (cross entropy); at most 2 flips of 896 000 decisions, on |z| <= 1.2e-6 max |z|."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import mlp_reference as mr
from tests import mlp_x3_reference as xr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL, FLIP_Z, FLIP_FRACTION = 1e-4, 1e-5, 1e-4
SHAPES = [(450, 128, 3, 1000), (450, 128, 8, 1000), (450, 512, 3, 1000), (8100, 128, 8, 257)]
OUT = 8


@functools.lru_cache(maxsize=None)
def _case(in_channels, hidden, L, B):
    """mr.random_case weights, fp32-valued (not bf16-valued) inputs"""
    c = mr.random_case(in_channels, hidden, OUT, L, B, seed=in_channels + L)
    c["x"] = torch.randn(B, in_channels, generator=torch.Generator().manual_seed(in_channels + hidden + L), dtype=torch.float64).float().double()
    return c


@functools.lru_cache(maxsize=None)
def _engine(in_channels, hidden, L, out_channels=OUT):
    from morphsym_hgnn_amd import engine
    return engine.MLPEngine(in_channels, hidden, out_channels, L, "x3", DEV)


@pytest.mark.parametrize("loss", ["mse", "ce"])
@pytest.mark.parametrize("in_channels,hidden,L,B", SHAPES)
def test_step_against_fp64_under_the_engines_decisions(in_channels, hidden, L, B, loss):
    c = _case(in_channels, hidden, L, B)
    e = _engine(in_channels, hidden, L)
    flat = mr.flatten(c["params"]).float().to(DEV)
    x = e.cast_input(c["x"])
    assert x.dtype == torch.float32 and torch.equal(x[:, :in_channels].double().cpu(), c["x"])
    target = c["y"] if loss == "mse" else c["labels"]
    if loss == "mse":
        out, lv, g = e.step_mse(x, flat, c["y"].float().to(DEV).contiguous())
    else:
        out, lv, g = e.step_ce(x, flat, c["labels"].to(DEV).contiguous())
    masks = [(e.stash(B, l) > 0).cpu() for l in range(1, L)]
    ref = xr.reference_with_decisions(c["params"], c["x"], masks, loss=loss, target=target)
    # the decisions: a flip only where the reference's pre-activation is zero to the arithmetic's resolution, and only a few
    flips, total, worst_z = 0, 0, 0.0
    for l, m in enumerate(masks):
        z = ref["zs"][l]
        flipped = m != (z > 0)
        flips += int(flipped.sum()); total += m.numel()
        if bool(flipped.any()):
            worst_z = max(worst_z, float(z[flipped].abs().max() / z.abs().max()))
    errs = {"out": mr.rel_max(out, ref["out"]), "loss": abs(float(lv) - float(ref["loss"])) / abs(float(ref["loss"]))}
    for i, ((dW, db), (rW, rb)) in enumerate(zip(mr.unflatten(g, mr.layer_dims(in_channels, hidden, OUT, L)), ref["grads"])):
        errs[f"dW{i}"], errs[f"db{i}"] = mr.rel_l2(dW, rW), mr.rel_l2(db, rb)
    print(f"x3 mlp in {in_channels} h {hidden} L {L} B {B} {loss}: worst {max(errs.values()):.2e}", {k: f"{v:.2e}" for k, v in errs.items()},
          f"flips {flips} of {total}, worst |z| / max |z| {worst_z:.2e}")
    assert worst_z <= FLIP_Z, worst_z
    assert flips <= FLIP_FRACTION * total, (flips, total)
    assert all(v <= TOL for v in errs.values()), errs


def test_module_at_the_default_precision_is_the_fused_x3_engine():
    """models.MLP with nothing set (MSHGNN_DTYPE unset): forward + autograd backward are MLPEngine("x3").forward(training) + backward, bit for bit."""
    from morphsym_hgnn_amd import models
    torch.manual_seed(6)
    m = models.MLP(450, 128, 8, 3).to(DEV)
    assert m._precision == "x3" and m._fused()
    g = torch.Generator().manual_seed(10)
    x, gout = torch.randn(65, 450, generator=g), torch.randn(65, 8, generator=g).to(DEV)
    out = m(x.to(DEV))
    (out * gout).sum().backward()
    assert m._engine(torch.device(DEV)).dtype == "x3"
    e = _engine(450, 128, 3)
    flat = torch.cat([p.detach().reshape(-1) for p in m.parameters()]).contiguous()
    xs = e.cast_input(x)
    o2 = e.forward(xs, flat, training=True)
    g2 = e.backward(xs, flat, gout.contiguous())
    assert torch.equal(out.detach(), o2)
    assert torch.equal(torch.cat([p.grad.reshape(-1) for p in m.parameters()]), g2)
    m.set_precision("bf16")
    assert m._fused() and m._engine(torch.device(DEV)).dtype == "bf16"
    m.set_precision("f32")
    assert not m._fused()


T = 20


def _dataset(kind, dtype):
    from morphsym_hgnn_amd import windows
    from tests import test_window_symmetry as ws
    if kind == "mc":        # MiniCheetah contacts: classification, in = T x 54, out = 8
        recipe, seq = windows.minicheetah_mlp_recipe(ws.JP, ws.FP, T), ws.SEQ4
    else:                   # A1 GRFs (z): regression, in = T x 42, out = 4
        recipe, seq = windows.quadsdk_a1_mlp_recipe(ws.JP, ws.FP, T, 1), ws.SEQ
    half = len(next(iter(seq.values()))) // 2
    seqs = [{k: np.asarray(v)[:half] for k, v in seq.items()}, {k: np.asarray(v)[half:] for k, v in seq.items()}]
    return windows.ResidentDataset(seqs, recipe, dtype=dtype, device=DEV)


def _wrapper(kind, seed=1):
    from morphsym_hgnn_amd import wrappers
    torch.manual_seed(seed)
    w = wrappers.MLP_Lightning(T * 54, 128, 8, 3, 64, regression=False) if kind == "mc" else wrappers.MLP_Lightning(T * 42, 128, 4, 3, 64, regression=True)
    return w.to(DEV)      # (the default precision)


def _dense_rows(e, ds, starts):
    xs, y, _ = ds.assemble(starts)
    x = xs[0]
    return e.cast_input(x if x.dtype == torch.float32 and x.shape[1] % 8 == 0 else x[:, :e.in_channels].float()), y


@pytest.mark.parametrize("store_dtype", ["f32", "bf16"])
@pytest.mark.parametrize("kind", ["mc", "a1"])
def test_wrapper_training_step_equals_assemble_plus_the_dense_step(kind, store_dtype):
    ds = _dataset(kind, store_dtype)
    view = ds.view()
    idx = torch.randint(0, len(view), (200,), generator=torch.Generator().manual_seed(3))
    w = _wrapper(kind)
    loss = w.training_step(view.batch(idx, {}), 0)
    loss.backward()
    got = torch.cat([p.grad.detach().reshape(-1) for p in w.parameters()]).clone()
    loss = loss.detach().clone()
    e = w.model._engine(torch.device(DEV))
    assert e.dtype == "x3" and not e._series_ok(ds)
    flat = w.model._flat_params(torch.device(DEV)).detach().clone()
    x, y = _dense_rows(e, ds, view.starts(idx.to(DEV)))
    if kind == "mc":
        _, l2, g2 = e.step_ce(x, flat, (y != 0).to(torch.int32).contiguous())
    else:
        _, l2, g2 = e.step_mse(x, flat, y.contiguous())
    assert torch.equal(loss.reshape(-1), l2.reshape(-1)) and torch.equal(got, g2)


def test_evaluate_sequence_equals_batch_by_batch_forward():
    from morphsym_hgnn_amd import wrappers
    ds = _dataset("a1", "bf16")
    w = _wrapper("a1")
    pred = wrappers.evaluate_sequence(w, ds, {}, batch_size=96)
    assert pred.shape[0] == len(ds)
    e, flat = w.model._engine(torch.device(DEV)), w.model._flat_params(torch.device(DEV))
    assert e.dtype == "x3"
    view = ds.view()
    for lo in (0, 96, (len(ds) - 1) // 96 * 96):
        idx = torch.arange(lo, min(lo + 96, len(ds)))
        x, _ = _dense_rows(e, ds, view.starts(idx.to(DEV)))
        assert torch.equal(pred[lo:lo + idx.numel()].reshape(idx.numel(), -1), e.forward(x, flat, training=False))


def test_dense_step_is_capturable_in_a_graph():
    """Three replays of a captured step_mse on fresh rows equal three eager steps bit for bit (no allocation, no host read inside the step)."""
    in_channels, Bs = 450, 96
    e = _engine(in_channels, 128, 3, 4)
    torch.manual_seed(4)
    flat = mr.flatten([(m.weight.detach(), m.bias.detach()) for m in mr.sequential(in_channels, 128, 4, 3) if isinstance(m, torch.nn.Linear)]).float().to(DEV)
    gen = torch.Generator().manual_seed(7)
    batches = [(e.cast_input(torch.randn(Bs, in_channels, generator=gen)), torch.randn(Bs, 4, generator=gen).to(DEV)) for _ in range(4)]
    sx, sy = batches[0][0].clone(), batches[0][1].clone()
    out, g, loss = torch.empty(Bs, 4, device=DEV), torch.empty(e.n_flat, device=DEV), torch.empty(1, device=DEV)
    e.step_mse(sx, flat, sy, out=out, grad_flat=g, loss=loss)      # warm-up: the workspace exists
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        e.step_mse(sx, flat, sy, out=out, grad_flat=g, loss=loss)
    for x, y in batches[1:]:
        sx.copy_(x); sy.copy_(y)
        graph.replay()
        got = (out.clone(), g.clone(), loss.clone())
        o2, l2, g2 = e.step_mse(x, flat, y)
        assert torch.equal(got[0], o2) and torch.equal(got[1], g2) and torch.equal(got[2], l2)


def test_series_form_is_refused_on_the_split_plan_and_launches_nothing():
    from morphsym_hgnn_amd import engine
    e = _engine(450, 128, 3, 4)
    B = 40
    flat = torch.zeros(e.n_flat, device=DEV)
    out, grad, loss = torch.full((B, 4), -7.5, device=DEV), torch.full((e.n_flat,), -7.5, device=DEV), torch.full((1,), -7.5, device=DEV)
    y = torch.zeros(B, 4, device=DEV)
    ws = torch.full((e.workspace_bytes(B, True),), 0xA5, dtype=torch.uint8, device=DEV)
    inp = engine.MshgnnMlpInput()      # x == NULL: the series form
    rc = e.lib.mshgnn_mlp_step(e._plan, C.byref(inp), 0, C.c_void_p(y.data_ptr()), C.c_void_p(flat.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(loss.data_ptr()),
                               C.c_void_p(grad.data_ptr()), C.c_void_p(ws.data_ptr()), B, None)
    assert rc == -2 and b"assemble" in e.lib.mshgnn_last_error()      # MSHGNN_EUNSUPPORTED
    rc = e.lib.mshgnn_mlp_forward(e._plan, C.byref(inp), C.c_void_p(flat.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()), B, 1, None)
    assert rc == -2
    torch.cuda.synchronize()
    assert bool((out == -7.5).all()) and bool((grad == -7.5).all()) and bool((loss == -7.5).all()) and bool((ws == 0xA5).all())
