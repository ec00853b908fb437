"""The L1 / Huber training loss on the routes above the engine's exact tests (tests/test_loss_exact_gpu.py):

  * random data on the parity plans x3 and f32, A1-C2 L = 3 at 64 windows: the one-call step against the fp64 oracle evaluated with the engine's relu
    decisions (helpers.run_step_case's method, the loss swapped) at the project's parity bound 1e-4.  L1 is discontinuous at d = 0, so its targets are built
    from the oracle's output, y = out_ref + s u with u in [0.25, 1] and s either sign, and the test asserts 0.25 >= 100 * 1e-4 * max|out_ref|: no element is
    near the kink and none is left out.  Huber is C1 and needs no exclusion; delta is the median |d|, and both branches are asserted to be populated.
  * wrappers: training_step returns the chosen loss on the fused and on the two-call route.  On rounding-free data the gradients of both routes are the same
    bits; the two losses are sums of the same fp32 terms in two orders (the tile sums of the fused tail, the grid-stride sums of mshgnn_regression_loss), so
    they are the same bits where the terms add exactly (L1 on the dyadic case) and within the exact tests' 2e-7 otherwise (Huber).  `mse_loss` / `l1_loss`
    stay the metric kernel's values, validation_step returns the MSE, the GRF wrapper logs "train_loss" only at a kind other than MSE.
  * series routes: training_step on a view batch of a small synthetic dataset (tests/test_dataset_gpu.py's: three A1-C2 sequences of 150 / 151 / 407 rows) --
    mshgnn_step_mse_series, standardised: mshgnn_step_mse_series_std, nothing assembled -- equals assemble-then-step bit for bit at Huber, loss and the whole
    flat gradient.
  * the kind is kept on the model alone: set there directly, the wrapper's next step follows; MLP_Lightning and COM_MLP_Lightning (the training / validation
    steps the GRF wrappers do not share) return Engine.reg_loss of the prediction, keep `mse_loss` the metric value and validate on the MSE.
  * Symmetrised at Huber equals the hand composition orbit average -> Engine.reg_loss -> transpose -> engine backward, loss and flat gradient, bit for bit.
  * GraphedTrainingStep: replay equals the eager step bit for bit at 32 windows, Huber; a graph captured at Huber keeps it when the plan is set back.
  * a model at "f64": the wrapper's loss within 1e-9 of torch's fp64 loss of its own prediction (the bound of tests/test_f64_models_gpu.py).
  * a checkpoint round trip keeps kind and delta, and a default model's hyper-parameters are unchanged.
"""
import types

import numpy as np
import pytest
import torch

from morphsym_hgnn_amd import engine as eng
from tests import helpers
from tests import loss_reference as lr

pytestmark = pytest.mark.gpu

PARITY = 1e-4
A1C2 = ("c2", "a1-c2", "a1-c2", 128, 3, True)


def _oracle(spec, e, x_dict, params, B, loss_fn=None):
    """The fp64 oracle under the relu decisions of the engine's last training forward (helpers.run_step_case): (out, loss, grads, decisions outside 1e-4)."""
    from oracle import ms_hgnn_oracle as orc
    decisions = helpers.engine_relu_decisions(e, spec, B)
    outside = [0]

    def relu_fn(key, h):
        if key not in decisions:
            return torch.relu(h)
        rows = helpers.row_live_mask(spec, key, B).view(-1, 1)
        exact = h.detach() > 0
        m = torch.where(rows, decisions[key], exact)
        diff = m != exact
        if bool(diff.any()):
            outside[0] += int((h.detach().abs()[diff] > 1e-4 * float(h.detach().abs().max())).sum())
        return h * m.to(h.dtype)

    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in params.items()}
    out = orc.forward(helpers.oracle_config(spec), leaves, {k: v.clone() for k, v in x_dict.items()}, spec.topology.edge_index_dict(B), relu_fn=relu_fn)
    out = out[0] if isinstance(out, tuple) else out
    if loss_fn is None:
        return out.detach().reshape(-1), None, None, outside[0]
    loss = loss_fn(out.reshape(-1))
    loss.backward()
    return out.detach().reshape(-1), float(loss.detach()), {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()}, outside[0]


@pytest.mark.parametrize("dtype", ["x3", "f32"])
@pytest.mark.parametrize("kind", ["l1", "huber"])
def test_random_data_step_matches_the_fp64_oracle_at_the_parity_bound(kind, dtype):
    spec, B = helpers.make_spec(*A1C2), 64
    x, y0, params = helpers.random_case(spec, B, seed=5)
    e = eng.Engine(spec, dtype)
    flat = eng.flatten_params(spec, params, e.device)
    xs = e.cast_inputs(x)
    e.forward(xs, flat, B, training=True)
    torch.cuda.synchronize()
    out_ref, _, _, _ = _oracle(spec, e, x, params, B)
    g = torch.Generator().manual_seed(11)
    if kind == "l1":
        u = 0.25 + 0.75 * torch.rand(out_ref.shape, generator=g, dtype=torch.float64)
        s = torch.randint(0, 2, out_ref.shape, generator=g).double() * 2 - 1
        y = (out_ref + s * u).float().double()
        assert 0.25 >= 100 * PARITY * float(out_ref.abs().max()), "an element could cross the kink within the parity bound"
        delta = 1.0
        loss_fn = lambda o: torch.nn.functional.l1_loss(o, y)
    else:
        y = y0.reshape(-1).float().double()
        delta = float(np.float32(float((out_ref - y).abs().median())))
        quad = (out_ref - y).abs() <= delta
        assert 0.3 < float(quad.double().mean()) < 0.7, "both branches of Huber are populated"
        loss_fn = lambda o: torch.nn.functional.huber_loss(o, y, delta=delta)
    e.set_regression_loss(kind, delta)
    out, loss, gflat = e.step_mse(xs, flat, y.to(e.device, torch.float32), B)
    torch.cuda.synchronize()
    o_out, o_loss, o_grads, outside = _oracle(spec, e, x, params, B, loss_fn)
    assert outside == 0

    def rel(a, b):
        a, b = a.detach().double().cpu().reshape(-1), b.detach().double().cpu().reshape(-1)
        return float((a - b).abs().max() / max(float(b.abs().max()), 1e-300))

    errs = {"out": rel(out, o_out), "loss": abs(float(loss) - o_loss) / abs(o_loss)}
    for k, v in eng.unflatten(spec, gflat).items():
        errs["grad:" + k] = float(v.abs().max()) if float(o_grads[k].abs().max()) == 0.0 else rel(v, o_grads[k])
    worst = max(errs, key=errs.get)
    print(f"\n{kind} {dtype}: worst {worst} {errs[worst]:.2e}, loss {errs['loss']:.2e}, delta {delta!r}")
    assert errs[worst] < PARITY, {k: v for k, v in errs.items() if v >= PARITY}


# ---- wrappers -----------------------------------------------------------------------------------------------------------------------------------------
def _batch(x_dict, ei, y, B, dev):
    return types.SimpleNamespace(x_dict={k: v.to(dev) for k, v in x_dict.items()}, edge_index_dict={k: v.to(dev) for k, v in ei.items()},
                                 y=y.to(dev).flatten(), batch_size=B)


def _wrapper(spec, batch, grf, dev, params):
    from morphsym_hgnn_amd import wrappers
    _, cfg = helpers.load_group("a1-c2")
    w = wrappers.HGNN_C2_Lightning_Reg(128, 3, spec.topology.metadata(), batch, lr=1e-3, grf_dimension=grf, symmetry_mode="MorphSym", group_operator_path=cfg).to(dev)
    w.model.load_state_dict(params)
    return w


def _grads(w):
    return {k: (p.grad.detach().clone() if p.grad is not None else torch.zeros_like(p)) for k, p in w.model.named_parameters()}


@pytest.mark.parametrize("kind,grf,B,seed", [("l1", 1, 16, 4), ("huber", 3, 17, 3)])
@pytest.mark.parametrize("plan", ["x3", "bf16"])
def test_training_step_returns_the_chosen_loss_on_both_routes(kind, grf, B, seed, plan, monkeypatch):
    monkeypatch.setenv("MSHGNN_DTYPE", plan)
    torch.set_default_dtype(torch.float64)
    dev = torch.device("cuda")
    spec = helpers.make_spec("c2", "a1-c2", "a1-c2", 128, 3, True, grf)
    case = lr.robust_case(spec, B, seed, kind, rel_scales=(1.0,))
    ref = lr.check_robust(spec, case)
    batch = _batch(case["x"], spec.topology.edge_index_dict(B), case["y"], B, dev)
    got = {}
    for fused in (True, False):
        w = _wrapper(spec, batch, grf, dev, case["params"])
        assert w.set_regression_loss(kind, case["delta"]) is w
        w.fused_training_step = fused
        loss = w.training_step(batch, 0)
        assert w.model._gpend_id == (1 if fused else 0)
        assert loss.requires_grad and loss is w.loss and loss is w.logged["train_loss"]
        metric = (float(w.mse_loss), float(w.l1_loss), float(w.rmse_loss))
        d = ref["out"] - case["y"]
        assert abs(metric[0] - float((d * d).mean())) <= 1e-6 * metric[0] and abs(metric[1] - float(d.abs().mean())) <= 1e-6 * metric[1]
        assert torch.equal(w.logged["train_MSE_loss"], w.mse_loss) and not w.mse_loss.requires_grad
        w.model.zero_grad()
        loss.backward()
        got[fused] = (loss.detach().float().cpu(), _grads(w))
        assert abs(float(loss.detach()) - ref["loss"]) <= 2e-7 * ref["loss"]
        for k, r in ref["grads"].items():
            assert torch.equal(got[fused][1][k].double().cpu(), r), f"{kind} fused={fused}: gradient {k} is not the oracle's"
        with torch.no_grad():
            v = w.validation_step(batch, 0)
        assert v is w.mse_loss and abs(float(v) - metric[0]) <= 1e-6 * metric[0] and not v.requires_grad
    for k in got[True][1]:
        assert torch.equal(got[True][1][k], got[False][1][k])
    if kind == "l1":      # the terms |d| are quarters: every summation order gives the same bits
        assert torch.equal(got[True][0], got[False][0]), (got[True][0], got[False][0])
    else:
        # Huber: the same fp32 terms, all positive, added in two fixed orders.  Neither order is longer than 16 dependent additions here (fused: <= 4 per lane, a
        # 6-step wave butterfly, the wave and tile sums; operator: <= 4 per lane, the butterfly, 4 waves, <= 1 partial), and the mean is one product: each loss is
        # within 17 u of the exact sum of the terms (u = 2^-24), the two within 34 u of each other -- directly, not through the reference
        a, b = float(got[True][0]), float(got[False][0])
        print(f"\nhuber {plan}: fused {a!r}, two-call {b!r}, apart by {abs(a - b) / b / 2.0 ** -24:.2f} u")
        assert abs(a - b) <= 34 * 2.0 ** -24 * b, (a, b)
    # back to MSE: the keys and the returned value are the MSE step's
    w.set_regression_loss("mse")
    w.logged.clear()
    loss = w.training_step(batch, 1)
    assert loss is w.mse_loss and "train_loss" not in w.logged and set(w.logged) == {"train_MSE_loss", "train_RMSE_loss", "train_L1_loss"}


@pytest.mark.parametrize("plan", ["bf16", "x3"])
@pytest.mark.parametrize("normalize", [False, True], ids=["plain", "std"])
def test_series_steps_equal_assemble_then_step_at_huber(normalize, plan, monkeypatch):
    from tests import test_dataset_gpu as dg
    ds = dg._dataset("a1c2", normalize, plan)
    w, spec, dev = dg._wrapper("a1c2", plan, ds)
    w.set_regression_loss("huber", 0.5)
    view, B = ds.view(), 17
    ix = dg._mixed_indices(view, B)
    ei = spec.topology.edge_index_dict(B, device=dev)
    xs, y, _ = ds.assemble(dg._mirror(view, ix).tolist())
    plain = types.SimpleNamespace(x_dict={t: x.clone() for t, x in zip(ds.recipe.node_types, xs)}, edge_index_dict=ei, y=y.clone(), batch_size=B)

    def run(batch):
        w.model.zero_grad()
        loss = w.training_step(batch, 0)
        assert loss is w.loss and w.model._gpend_id > 0      # the one-call route
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach().clone(), w.model._gflat.clone(), w.mse_loss.detach().clone()

    loss_a, flat_a, mse_a = run(plain)
    assert bool(flat_a.any()) and bool(torch.isfinite(flat_a).all())
    wb = view.batch(ix.cuda(), ei)
    with monkeypatch.context() as m:
        m.setattr(ds, "assemble", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the fused route assembles nothing")))
        loss_b, flat_b, mse_b = run(wb)
    assert torch.equal(loss_b, loss_a) and torch.equal(flat_b, flat_a) and torch.equal(mse_b, mse_a)
    # and it IS the Huber loss of the prediction, not the MSE
    with torch.no_grad():
        pred = w.model(x_dict=plain.x_dict, edge_index_dict=ei).reshape(-1).double().cpu()
    want = lr.ref64("huber", pred, y.reshape(-1).cpu(), 0.5)[0]
    assert abs(float(loss_a) - want) <= 1e-5 * want and abs(float(loss_a) - float(mse_a)) > 1e-3 * want
    view.check()


def test_the_kind_lives_on_the_model_whoever_sets_it(monkeypatch):
    """model.set_regression_loss directly (not through the wrapper): the wrapper's next fused step returns and logs the Huber loss as `loss` / "train_loss", and
    `mse_loss` stays the metric value -- the engine's Huber loss is never published as MSE."""
    monkeypatch.setenv("MSHGNN_DTYPE", "x3")
    torch.set_default_dtype(torch.float64)
    dev = torch.device("cuda")
    spec, B = helpers.make_spec(*A1C2), 5
    x, y, params = helpers.random_case(spec, B, seed=3)
    batch = _batch(x, spec.topology.edge_index_dict(B), y, B, dev)
    w = _wrapper(spec, batch, 3, dev, params)
    mse = w.training_step(batch, 0)
    assert mse is w.mse_loss and "train_loss" not in w.logged
    w.model.set_regression_loss("huber", 0.5)
    loss = w.training_step(batch, 1)
    assert w.model._gpend_id == 2 and loss is w.loss and loss is w.logged["train_loss"] and loss is not w.mse_loss
    assert abs(float(w.mse_loss) - float(mse.detach())) <= 1e-6 * float(mse.detach()) and torch.equal(w.logged["train_MSE_loss"], w.mse_loss)
    with torch.no_grad():
        pred = w.model(x_dict=batch.x_dict, edge_index_dict=batch.edge_index_dict).reshape(-1).double().cpu()
    want = lr.ref64("huber", pred, y.reshape(-1), 0.5)[0]
    assert abs(float(loss) - want) <= 1e-5 * want and abs(want - float(mse)) > 1e-2 * want


@pytest.mark.parametrize("which", ["mlp", "com_mlp"])
@pytest.mark.parametrize("fused", [True, False])
def test_the_other_wrappers_training_and_validation_steps(which, fused, monkeypatch):
    """MLP_Lightning (its own training_step over Base_Lightning) and COM_MLP_Lightning (its own over COM_Base_Lightning's validation_step and `loss`) at Huber:
    the returned loss is Engine.reg_loss of the prediction, `mse_loss` the metric value, validation returns the MSE; back at "mse" the returned value is `mse_loss`."""
    from morphsym_hgnn_amd import wrappers
    monkeypatch.setenv("MSHGNN_DTYPE", "bf16")
    torch.set_default_dtype(torch.float32)
    torch.manual_seed(5)
    dev = torch.device("cuda")
    B, n_in, n_out = 33, 24, 12 if which == "mlp" else 6
    if which == "mlp":
        w = wrappers.MLP_Lightning(n_in, 128, n_out, 3, batch_size=B).to(dev)
    else:
        w = wrappers.COM_MLP_Lightning(n_in, 128, n_out, 3, batch_size=B, stats=(np.zeros(6), np.ones(6))).to(dev)
    g = torch.Generator().manual_seed(9)
    batch = (torch.randn(B, n_in, generator=g).to(dev), (2.0 * torch.randn(B, n_out, generator=g)).to(dev))
    w.fused_training_step = fused
    w.set_regression_loss("huber", 0.75)
    loss = w.training_step(batch, 0)
    assert (w.model._gpend_id == 1) == fused and loss.requires_grad and loss is w.loss
    with torch.no_grad():
        pred = w.model(batch[0]).float().contiguous()
    e = next(iter(w.model._engines.values()))
    assert e.regression_loss == ("huber", 0.75)
    want, _ = e.reg_loss(pred.reshape(-1), batch[1].reshape(-1).contiguous(), want_grad=False)
    # (the fused tail and the operator add the same terms in two orders: the 34 u of the test above)
    assert abs(float(loss) - float(want)) <= 34 * 2.0 ** -24 * float(want), (float(loss), float(want))
    mse = float(((pred.double() - batch[1].double()) ** 2).mean())
    assert abs(float(w.mse_loss) - mse) <= 1e-5 * mse and abs(float(loss) - mse) > 1e-2 * mse
    w.model.zero_grad()
    loss.backward()
    assert any(p.grad is not None and bool(p.grad.any()) for p in w.model.parameters())
    w.on_validation_epoch_start()
    with torch.no_grad():
        v = w.validation_step(batch, 0)
    assert v is w.mse_loss and abs(float(v) - mse) <= 1e-5 * mse
    w.on_validation_epoch_end()
    w.set_regression_loss("mse")
    again = w.training_step(batch, 1)
    assert again is w.mse_loss and abs(float(again) - mse) <= 1e-5 * mse


@pytest.mark.parametrize("kind,plan", [("mi", "x3"), ("mlp", "bf16")])
def test_symmetrised_step_equals_orbit_average_plus_reg_loss(kind, plan, monkeypatch):
    """Symmetrised(w) at Huber on an orbit-complete batch (the fixtures of tests/test_symmetrised_gpu.py: MI-HGNN on the A1 sequence under {e, gs}, MLP_Lightning):
    the view's training_step loss and the WHOLE flat gradient equal, by torch.equal, the hand composition engine forward -> the mirror's orbit average ->
    Engine.reg_loss -> the mirror's transpose -> engine backward.  The kind is set on the wrapper BEFORE the view is made for one case and through the view for
    the other; either way wrapper, view and model agree."""
    from morphsym_hgnn_amd import symmetrise as sym
    from tests import orbit_reference as orb
    from tests import test_symmetrised_gpu as sg
    w, orbit, act, spec, B = sg._wrapper(kind, plan, monkeypatch)
    K, dev = act.n_elements, torch.device("cuda")
    ei = spec.topology.edge_index_dict(K * B, device=dev) if spec is not None else None
    if kind == "mi":
        w.set_regression_loss("huber", 0.5)
        s = sym.Symmetrised(w, act)
    else:
        s = sym.Symmetrised(w, act)
        s.set_regression_loss("huber", 0.5)
    assert w.model.regression_loss == ("huber", 0.5)
    wb = orbit.orbit_batch(sg._starts(len(orbit), B), ei)
    w.model.zero_grad()
    loss = s.training_step(wb, 0)
    assert w.model._gpend_id == 0 and loss is s.loss and loss is s.logged["train_loss"] and loss is not s.mse_loss and w.mse_loss is None
    loss.backward()
    torch.cuda.synchronize()
    got_loss, got_flat = loss.detach().clone(), w.model._gflat.clone()
    assert bool(got_flat.any()) and bool(torch.isfinite(got_flat).all())
    m = w.model
    pdev = next(m.parameters()).device
    e, flat = m._engine(pdev), m._flat_params(pdev)
    assert e.regression_loss == ("huber", 0.5)
    if kind == "mlp":
        x = e.cast_input(wb.x_dict["mlp"][:, :m.in_channels].detach())
        out = e.forward(x, flat, training=True)
    else:
        x = e.cast_inputs(wb.x_dict)
        out = e.forward(x, flat, K * B, training=True)
    avg = torch.from_numpy(orb.average(out.reshape(K * B, act.row).cpu().numpy(), act.perm, act.sign, act.width, B)).to(dev)
    y = wb.y[:B].detach().to(dev, torch.float32).reshape(-1).contiguous()
    want_loss, g = e.reg_loss(avg.float().reshape(-1).contiguous(), y)
    go = torch.from_numpy(orb.average_backward(g.reshape(B, act.row).cpu().numpy(), act.perm, act.sign, act.width, B)).to(dev).reshape(out.shape).contiguous()
    want_flat = e.backward(x, flat, go) if kind == "mlp" else e.backward(x, flat, go, K * B)
    torch.cuda.synchronize()
    assert torch.equal(got_loss.reshape(()), want_loss.reshape(())) and torch.equal(got_flat, want_flat)
    # it is the Huber loss of the averaged prediction, and the metric values are still the metric kernel's
    want64 = lr.ref64("huber", avg.double().cpu().reshape(-1), y.double().cpu(), 0.5)[0]
    mse64 = float(((avg.double().cpu().reshape(-1) - y.double().cpu()) ** 2).mean())
    assert abs(float(got_loss) - want64) <= 1e-5 * want64 and abs(float(s.mse_loss) - mse64) <= 1e-5 * mse64 and abs(want64 - mse64) > 1e-3 * want64


def test_graphed_training_step_replays_the_huber_step_bit_for_bit():
    from morphsym_hgnn_amd import wrappers
    torch.set_default_dtype(torch.float64)
    dev = torch.device("cuda")
    spec, B = helpers.make_spec(*A1C2), 32
    ei = spec.topology.edge_index_dict(B)
    batches = []
    for s in range(4):
        x, y, params = helpers.random_case(spec, B, seed=200 + s)
        batches.append(_batch(x, ei, y, B, dev))
    _, _, params = helpers.random_case(spec, B, seed=1)
    twins = []
    for _ in range(2):
        w = _wrapper(spec, batches[0], 3, dev, params)
        w.set_regression_loss("huber", 0.75)
        w.graph_safe_optimizer = True
        twins.append((w, w.configure_optimizers()))
    (a, oa), (b, ob) = twins
    gs = wrappers.GraphedTrainingStep(a, oa, batches[0])
    a.set_regression_loss("mse")      # the captured step keeps the kind it was captured with: the setting travels by value in the kernel arguments
    la, lb = [], []
    for bt in batches[1:]:
        la.append(float(gs(bt)))
        ob.zero_grad(set_to_none=True)
        l = b.training_step(bt, 0); l.backward(); ob.step()
        lb.append(float(l))
    torch.cuda.synchronize()
    assert la == lb, (la, lb)
    for p, q in zip(a.model.parameters(), b.model.parameters()):
        assert torch.equal(p.detach(), q.detach())


@pytest.mark.parametrize("kind,delta", [("l1", 1.0), ("huber", 0.6)])
def test_f64_model_trains_on_the_fp64_loss(kind, delta):
    torch.set_default_dtype(torch.float64)
    dev = torch.device("cuda")
    spec, B = helpers.make_spec(*A1C2), 5
    x, y, params = helpers.random_case(spec, B, seed=3)
    batch = _batch(x, spec.topology.edge_index_dict(B), y, B, dev)
    w = _wrapper(spec, batch, 3, dev, params)
    w.model.set_precision("f64")
    w.set_regression_loss(kind, delta)
    assert w.model.regression_loss == (kind, delta if kind == "huber" else 1.0)
    loss = w.training_step(batch, 0)
    assert loss.dtype == torch.float64 and loss.requires_grad and loss is w.loss
    pred = w.model(x_dict=batch.x_dict, edge_index_dict=batch.edge_index_dict).detach().reshape(-1).cpu()
    want, gref = lr.ref64(kind, pred, y.reshape(-1), delta)
    assert abs(float(loss) - want) <= 1e-9 * want
    w.model.zero_grad()
    loss.backward()
    leaf = w.model(x_dict=batch.x_dict, edge_index_dict=batch.edge_index_dict)
    w.model.zero_grad()
    leaf.backward(gref.to(dev).reshape(leaf.shape))      # the fp64 reference gradient through the same fp64 operators
    g2 = _grads(w)
    w.model.zero_grad()
    w.training_step(batch, 1).backward()
    for k, g in _grads(w).items():
        assert float((g - g2[k]).abs().max()) <= 1e-9 * max(float(g2[k].abs().max()), 1e-300), k
    assert abs(float(w.mse_loss) - float(((pred - y.reshape(-1)) ** 2).mean())) <= 1e-5 * float(w.mse_loss)


def test_checkpoint_round_trip_keeps_kind_and_delta():
    from morphsym_hgnn_amd import checkpoint, models
    m = models.MLP(24, 128, 12, 3)
    assert "regression_loss" not in checkpoint.mlp_to_lightning_checkpoint(m)["hyper_parameters"]
    m.set_regression_loss("huber", 0.375)
    ck = checkpoint.mlp_to_lightning_checkpoint(m)
    assert ck["hyper_parameters"]["regression_loss"] == "huber" and ck["hyper_parameters"]["huber_delta"] == 0.375
    assert checkpoint.mlp_from_checkpoint(ck).regression_loss == ("huber", 0.375)
    m.set_regression_loss("l1")
    ck = checkpoint.mlp_to_lightning_checkpoint(m)
    assert "huber_delta" not in ck["hyper_parameters"] and checkpoint.mlp_from_checkpoint(ck).regression_loss == ("l1", 1.0)
    spec = helpers.make_spec(*A1C2)
    _, cfg = helpers.load_group("a1-c2")
    g = models.GRF_HGNN_C2(128, 3, spec.topology.metadata(), symmetry_mode="MorphSym", group_operator_path=cfg, grf_dimension=3)
    dev = torch.device("cuda")
    x, y, params = helpers.random_case(spec, 2, seed=1)
    g = g.to(dev)
    g(x_dict={k: v.to(dev) for k, v in x.items()}, edge_index_dict={k: v.to(dev) for k, v in spec.topology.edge_index_dict(2).items()})
    g.set_regression_loss("huber", 2.0)
    assert all(e.regression_loss == ("huber", 2.0) for e in g._engines.values()) and g._engines
    hp = dict(hidden_channels=128, num_layers=3, data_metadata=spec.topology.metadata(), symmetry_mode="MorphSym", group_operator_path=cfg, grf_dimension=3)
    ck = checkpoint.to_lightning_checkpoint(g, hp)
    back = checkpoint.model_from_checkpoint(ck, "heterogeneous_gnn_c2" if "heterogeneous_gnn_c2" in checkpoint.MODEL_CLASSES else
                                            next(k for k, v in checkpoint.MODEL_CLASSES.items() if v is models.GRF_HGNN_C2))
    assert back.regression_loss == ("huber", 2.0)
