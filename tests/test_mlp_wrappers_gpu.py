"""GPU: the MLP wrappers (wrappers.MLP_Lightning, wrappers.COM_MLP_Lightning) on resident data: the one-call training step against the two-call route through
torch's loss and autograd (within the emulation bounds of tests/test_mlp_gpu.py: both run the same bf16 arithmetic, the loss sums differ), graphed against
eager training bit for bit, evaluation straight from the series, the evaluators' table over an orbit view, and the reference's (x, y) tuple batches."""
import numpy as np
import pytest
import torch

from tests import mlp_reference as mr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = 20
OUT_TOL, GRAD_TOL = 4e-3, 1.5e-2


def _dataset(kind, orbit=False):
    from morphsym_hgnn_amd import windows
    from tests import test_window_symmetry as ws
    if kind == "mc":        # MiniCheetah contacts: classification, in = T x 54, out = 8
        recipe, seq, group = windows.minicheetah_mlp_recipe(ws.JP, ws.FP, T), ws.SEQ4, ws.K4
    elif kind == "a1":      # A1 GRFs (z): regression, in = T x 42, out = 4
        recipe, seq, group = windows.quadsdk_a1_mlp_recipe(ws.JP, ws.FP, T, 1), ws.SEQ, ws.A1
    else:                   # Solo centroidal momentum: in = 24, out = 6
        g = np.random.default_rng(5)
        X, Y = g.standard_normal((300, 24)).astype(np.float32), g.standard_normal((300, 6)).astype(np.float32)
        recipe, seq, group = windows.solo_com_mlp_recipe(list(range(12)), 1), windows.solo_com_arrays(X, Y), None
    half = len(next(iter(seq.values()))) // 2
    seqs = [{k: np.asarray(v)[:half] for k, v in seq.items()}, {k: np.asarray(v)[half:] for k, v in seq.items()}]
    ds = windows.ResidentDataset(seqs, recipe, dtype="bf16", device=DEV)
    return (ds.orbit(group) if orbit else ds), recipe


def _wrapper(kind, seed=1, lr=1e-3):
    from morphsym_hgnn_amd import wrappers
    torch.manual_seed(seed)
    if kind == "mc":
        w = wrappers.MLP_Lightning(T * 54, 128, 8, 3, 64, lr=lr, regression=False)
    elif kind == "a1":
        w = wrappers.MLP_Lightning(T * 42, 128, 4, 3, 64, lr=lr, regression=True)
    else:
        w = wrappers.COM_MLP_Lightning(24, 128, 6, 3, 64, lr=lr, stats=(np.zeros(6), np.ones(6)))
    w = w.to(DEV)
    w.model.set_precision("bf16")
    return w


@pytest.mark.parametrize("kind", ["mc", "a1", "com"])
def test_training_step_equals_helper_plus_torch_loss_and_autograd(kind):
    ds, _ = _dataset(kind)
    view = ds.view()
    idx = torch.randint(0, len(view), (200,), generator=torch.Generator().manual_seed(3))
    w = _wrapper(kind)
    loss = w.training_step(view.batch(idx, {}), 0)
    loss.backward()
    got = [p.grad.detach().clone() for p in w.parameters()]
    w2 = _wrapper(kind)
    w2.fused_training_step = False
    y, y_pred = w2.step_helper_function(view.batch(idx, {}))
    if kind == "mc":
        want_loss = torch.nn.functional.cross_entropy(y_pred.reshape(-1, 2), (y.reshape(-1) != 0).long())
    else:
        want_loss = torch.nn.functional.mse_loss(y_pred, y.view_as(y_pred))
    want_loss.backward()
    assert abs(float(loss) - float(want_loss)) <= OUT_TOL * abs(float(want_loss)), (float(loss), float(want_loss))
    for (k, p), g in zip(w2.named_parameters(), got):
        assert mr.rel_l2(g, p.grad.detach().cpu()) < GRAD_TOL, k


@pytest.mark.parametrize("kind", ["mc", "a1"])
def test_graphed_training_equals_its_eager_twin_and_lowers_the_loss(kind):
    from morphsym_hgnn_amd import wrappers
    ds, _ = _dataset(kind)
    view = ds.view()
    batches = [torch.randint(0, len(view), (64,), generator=torch.Generator().manual_seed(100 + s)) for s in range(20)]
    losses = {}
    for mode in ("graph", "eager"):
        w = _wrapper(kind, lr=3e-3)
        w.graph_safe_optimizer = True
        opt = w.configure_optimizers()
        if mode == "graph":
            step = wrappers.GraphedTrainingStep(w, opt, view.batch(batches[0], {}), index_source=view)
            run = [step(b).clone() for b in batches]
        else:
            run = []
            for b in batches:
                opt.zero_grad(set_to_none=True)
                lv = w.training_step(view.batch(b.to(DEV), {}), 0)
                lv.backward()
                opt.step()
                run.append(lv.detach().clone())
        losses[mode] = (torch.stack([v.reshape(()) for v in run]).cpu(), torch.cat([p.detach().reshape(-1) for p in w.parameters()]).cpu())
    assert torch.equal(losses["graph"][0], losses["eager"][0]), (losses["graph"][0], losses["eager"][0])
    assert torch.equal(losses["graph"][1], losses["eager"][1])
    ls = losses["eager"][0]
    assert float(ls[-5:].mean()) < float(ls[:5].mean()), ls


@pytest.mark.parametrize("kind", ["mc", "a1", "com"])
def test_evaluate_sequence_equals_batch_by_batch_forward(kind):
    from morphsym_hgnn_amd import wrappers
    ds, _ = _dataset(kind)
    w = _wrapper(kind)
    pred = wrappers.evaluate_sequence(w, ds, {}, batch_size=96)
    assert pred.shape[0] == len(ds)
    e, flat = w.model._engine(torch.device(DEV)), w.model._flat_params(torch.device(DEV))
    view = ds.view()
    for lo in (0, 96, (len(ds) - 1) // 96 * 96):
        idx = torch.arange(lo, min(lo + 96, len(ds)))
        xs, _, _ = ds.assemble(view.starts(idx.to(DEV)))
        assert torch.equal(pred[lo:lo + idx.numel()].reshape(idx.numel(), -1), e.forward(xs[0], flat, training=False))


def test_evaluate_table_over_an_orbit_view_is_full():
    from morphsym_hgnn_amd import wrappers
    ds, _ = _dataset("mc", orbit=True)
    w = _wrapper("mc")
    tab = wrappers.evaluate_table(w, ds.view(), {}, batch_size=128)
    K, S = ds.view().segment_shape
    assert (K, S) == (4, 2) and tab.predictions.shape[0] == len(ds.view())
    for name, t in tab.table.items():
        assert tuple(t.shape) == (K, S) and bool(torch.isfinite(t).all()), name


def test_tuple_batches_work_as_in_the_reference():
    w = _wrapper("a1")
    g = torch.Generator().manual_seed(8)
    x, y = torch.randn(33, T * 42, generator=g, dtype=torch.float64).to(DEV), torch.randn(33, 4, generator=g, dtype=torch.float64).to(DEV)
    yy, y_pred = w.step_helper_function((x, y))
    assert yy is y and tuple(y_pred.shape) == (33, 4)
    loss = w.training_step((x, y), 0)
    loss.backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in w.parameters())
    want = torch.nn.functional.mse_loss(y_pred.double(), y)
    assert abs(float(loss) - float(want)) <= OUT_TOL * float(want)
    with torch.no_grad():
        assert float(w.validation_step((x, y), 0)) > 0
