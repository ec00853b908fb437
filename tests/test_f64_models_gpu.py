"""Precision "f64" on the module surface: `set_precision("f64")` (and MSHGNN_DTYPE=f64) on the MS-HGNN models, models.MLP and the wrappers -- fp64
parameters, every Linear / GraphConv on the fp64 MFMA operators (csrc/mshgnn_ops.hip), autograd for the gradients, an fp64 loss.

Tolerance 1e-9 against the fp64 oracle, DERIVED, not measured: the longest reduction of these cases is under 1e3 terms (n u ~ 1e-13), the worst
cancellation this project has seen on a gradient (the decoder-bias case noted in tests/test_generic_gpu.py) costs about two orders, which leaves two more.
The fp32 operator route measures up to 1.4e-6 on the same checker and fails this file by three orders.  Measured worst values per case: DESIGN.md 8.
"""
import types

import pytest
import torch

from tests import helpers
from tests.test_models import _build

pytestmark = pytest.mark.gpu
RTOL = 1e-9
DEV = "cuda"
FIXTURE_CASES = ["a1c2_h128_L3_d3_B3", "a1c2_h128_L2_d3_B37", "mck4_cls_h128_L2_B3", "mi_h128_L2_d3_B2", "solok4com_h128_L3_B5", "solos4com_h128_L2_B3",
                 "a1c2_h256_L2_d3_B3"]


def _f64_model(case, spec, x_dict, ei, params):
    """The model of a golden case at "f64" on the device, lazily initialised and loaded with the case's fp64 parameters."""
    m = _build(case, spec).set_precision("f64").to(DEV)
    xd = {k: v.to(DEV) for k, v in x_dict.items()}
    eid = {k: v.to(DEV) for k, v in ei.items()}
    with torch.no_grad():
        m(x_dict={k: v.clone() for k, v in xd.items()}, edge_index_dict=eid)
    m.load_state_dict(params)
    assert all(p.dtype == torch.float64 for p in m.parameters()) and not m._engines, "an f64 model compiles no engine and holds fp64 parameters"
    return m, xd, eid


def _loss(case, m, out, y, B):
    w = m.num_bases * m.num_dimensions_per_base if case["kind"].endswith("_com") else m.out_channels_per_foot * 4
    y_pred = torch.reshape(out.squeeze(), (B, w))
    if case["regression"]:
        return ((y_pred.flatten() - y.to(out.device).reshape(B, w).flatten()) ** 2).mean()
    return torch.nn.functional.cross_entropy(y_pred.reshape(B * 4, 2), y.to(out.device).reshape(B, 4).long().flatten())


@pytest.mark.parametrize("name", FIXTURE_CASES)
def test_f64_model_matches_the_golden_fixture_at_1e_9(name):
    """Output, loss and every parameter gradient through helpers.check_against_fixture at rtol = 1e-9 (the fixtures hold the fp64 oracle's values)."""
    assert torch.cuda.is_available()
    torch.set_default_dtype(torch.float64)
    case, spec, fx, x_dict, y, params, ei = helpers.load_case(name)
    B = case["B"]
    m, xd, eid = _f64_model(case, spec, x_dict, ei, params)
    out = m(x_dict=xd, edge_index_dict=eid)
    assert out.dtype == torch.float64 and out.is_cuda
    loss = _loss(case, m, out, y, B)
    assert loss.dtype == torch.float64
    loss.backward()
    grads = {k: (p.grad.detach().cpu() if p.grad is not None else torch.zeros_like(p).cpu()) for k, p in m.named_parameters()}
    assert all(g.dtype == torch.float64 for g in grads.values())
    err, worst = helpers.check_against_fixture(fx, out.detach().cpu(), loss.detach().cpu(), grads, rtol=RTOL, what=name + " f64")
    print(f"f64 {name}: output rel err {err:.3e}, worst gradient measure {worst[0]:.3e} ({worst[1]})")
    # inputs of another dtype are widened: the fp32 image of the inputs gives the output of those fp32 values, in fp64
    x32 = {k: v.float() for k, v in xd.items()}
    with torch.no_grad():
        o32 = m(x_dict=x32, edge_index_dict=eid)
        o64 = m(x_dict={k: v.double() for k, v in x32.items()}, edge_index_dict=eid)
    assert o32.dtype == torch.float64 and torch.equal(o32, o64)
    # the one-call and series routes step aside
    assert m.fused_training_step(xd, eid, y) is None


def _rel(a, b):
    a, b = a.detach().double().cpu().reshape(-1), b.detach().double().cpu().reshape(-1)
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-300))


def test_f64_a1c2_l3_at_257_windows_matches_the_oracle_step():
    """A1-C2, 3 layers, 257 windows (past one 64-row tile for every node type, weight gradients over 257 n_t rows up to 3084: split-K), random data:
    output, loss, every parameter gradient and the input gradients (autograd on the operator route) within 1e-9 of oracle.step's, relative to each
    tensor's largest entry; gradients the oracle has as exact zeros are exact zeros or None."""
    from oracle import ms_hgnn_oracle as orc
    torch.set_default_dtype(torch.float64)
    spec = helpers.make_spec("c2", "a1-c2", "a1-c2", 128, 3)
    B = 257
    x_dict, y, params = helpers.random_case(spec, B, seed=257)
    ei = spec.topology.edge_index_dict(B)
    case = dict(kind="c2", cfg="a1-c2", hidden=128, layers=3, regression=True, grf=3)
    m, xd, eid = _f64_model(case, spec, x_dict, ei, params)
    xd = {k: v.requires_grad_(True) for k, v in xd.items()}
    out = m(x_dict=xd, edge_index_dict=eid)
    loss = _loss(case, m, out, y, B)
    loss.backward()
    xr = {k: v.clone().requires_grad_(True) for k, v in x_dict.items()}
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in params.items()}      # (oracle.step, with the inputs as leaves too)
    cfg = helpers.oracle_config(spec)
    o_out = orc.forward(cfg, leaves, {k: v.clone() for k, v in xr.items()}, ei)
    yy, yp = orc.wrapper_outputs(cfg, o_out, y, B)
    o_loss = orc.mse_loss(yy, yp)
    o_loss.backward()
    s_out, s_loss, s_grads = orc.step(cfg, params, x_dict, ei, y, B)
    assert torch.equal(s_out, o_out.detach()) and torch.equal(s_loss, o_loss.detach())
    errs = {"out": _rel(out, o_out), "loss": _rel(loss, o_loss)}
    for k, p in m.named_parameters():
        ref = s_grads[k]
        if float(ref.abs().max()) == 0.0:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
        else:
            errs["grad:" + k] = _rel(p.grad, ref)
    for k in xd:
        if xr[k].grad is not None and float(xr[k].grad.abs().max()) > 0.0:
            errs["dx:" + k] = _rel(xd[k].grad, xr[k].grad)
    worst = max(errs, key=errs.get)
    print(f"f64 A1-C2 L3 B257: worst {worst} {errs[worst]:.3e}; out {errs['out']:.3e} loss {errs['loss']:.3e}")
    assert errs[worst] <= RTOL, {k: v for k, v in errs.items() if v > RTOL}
    assert any(k.startswith("dx:") for k in errs)


def test_precision_round_trip_keeps_the_x3_bits_and_a_state_dict_keeps_every_bit():
    """x3 forward, set_precision("f64") and a forward, x3 again and a forward: fp32 -> fp64 -> fp32 of the parameters is the identity, so the two x3 outputs
    are bit-equal (and the f64 one is another, closer to the oracle).  A reference-style state dict (fp64 tensors that are NOT fp32 values) loaded into the
    f64 model leaves every parameter bit-equal to its source; f64 -> x3 then rounds them to fp32 once."""
    torch.set_default_dtype(torch.float64)
    case, spec, fx, x_dict, y, params, ei = helpers.load_case("a1c2_h128_L3_d3_B3")
    m = _build(case, spec).to(DEV)
    xd, eid = {k: v.to(DEV) for k, v in x_dict.items()}, {k: v.to(DEV) for k, v in ei.items()}
    with torch.no_grad():
        m(x_dict=xd, edge_index_dict=eid)
        m.load_state_dict(params)
        a = m(x_dict=xd, edge_index_dict=eid).clone()
        p32 = {k: v.detach().clone() for k, v in m.named_parameters()}
        assert all(v.dtype == torch.float32 for v in p32.values()) and m._flat_ok
        m.set_precision("f64")
        assert all(p.dtype == torch.float64 and torch.equal(p, p32[k].double()) for k, p in m.named_parameters()) and not m._flat_ok
        mid = m(x_dict=xd, edge_index_dict=eid).clone()
        m.set_precision("x3")
        assert all(p.dtype == torch.float32 for p in m.parameters())
        b = m(x_dict=xd, edge_index_dict=eid).clone()
        assert m._flat_ok and all(torch.equal(p, p32[k]) for k, p in m.named_parameters())
    assert torch.equal(a, b), "x3 -> f64 -> x3 changed the x3 output"
    ref = torch.from_numpy(fx["out"]).reshape(-1)
    assert mid.dtype == torch.float64 and not torch.equal(mid, a)
    # a reference checkpoint: fp64 tensors with bits below fp32's
    m.set_precision("f64")
    src = {k: v.double() * (1.0 + 2.0 ** -40) for k, v in params.items()}
    assert not any(torch.equal(v.float().double(), v) for v in src.values())
    m.load_state_dict(src)
    assert all(torch.equal(p.detach().cpu(), src[k]) for k, p in m.named_parameters()), "load_state_dict into an f64 model narrowed a parameter"
    with torch.no_grad():
        exact = m(x_dict=xd, edge_index_dict=eid)
    m.set_precision("x3")
    assert all(torch.equal(p.detach().cpu(), src[k].float()) for k, p in m.named_parameters())      # rounded to fp32, once
    assert _rel(mid, ref) < 1e-6 and exact.dtype == torch.float64
    with pytest.raises(ValueError):
        m.set_precision("f16")


# ---- wrappers -----------------------------------------------------------------------------------------------------------------------------------------
def _batch(x_dict, ei, y, B):
    return types.SimpleNamespace(x_dict={k: v.to(DEV) for k, v in x_dict.items()}, edge_index_dict={k: v.to(DEV) for k, v in ei.items()},
                                 y=y.to(DEV).flatten(), batch_size=B)


@pytest.mark.parametrize("name,by_env", [("a1c2_h128_L3_d3_B3", False), ("mck4_cls_h128_L2_B3", True)])
def test_wrapper_at_f64_trains_like_its_cpu_twin(name, by_env, monkeypatch):
    """HGNN_C2_Lightning_Reg (set_precision after construction) and HGNN_K4_Lightning (MSHGNN_DTYPE=f64 at construction: the lazy-initialising call runs
    with host parameters): training_step returns an fp64 loss within 1e-9 of the oracle's that never passed the fp32 loss kernel, configure_optimizers
    hands out torch's Adam, and three steps follow a CPU fp64 twin that steps the same Adam on the oracle's gradients; validation_step's loss is fp64 as
    well; GraphedTrainingStep refuses the model with a reason."""
    from morphsym_hgnn_amd import metrics, wrappers
    from oracle import ms_hgnn_oracle as orc
    from tests.test_wrappers import _wrapper
    torch.set_default_dtype(torch.float64)
    if by_env:
        monkeypatch.setenv("MSHGNN_DTYPE", "f64")
    case, spec, fx, x_dict, y, params, ei = helpers.load_case(name)
    B = case["B"]
    batch = _batch(x_dict, ei, y, B)
    w = _wrapper(case, spec, batch)
    if not by_env:
        w.model.set_precision("f64")
    w = w.to(DEV)
    assert w.model._precision == "f64"
    w.model.load_state_dict(params)
    opt = w.configure_optimizers()
    assert type(opt) is torch.optim.Adam, "the flat optimizers are fp32 by construction: an f64 model gets torch's own"
    with pytest.raises(ValueError, match="f64"):
        wrappers.GraphedTrainingStep(w, opt, batch)
    calls = []
    real = metrics._StepLoss.forward
    monkeypatch.setattr(metrics._StepLoss, "forward", staticmethod(lambda *a, **k: calls.append(1) or real(*a, **k)))
    cfg = helpers.oracle_config(spec)
    twin = {k: v.detach().clone().double().requires_grad_(True) for k, v in params.items()}
    topt = torch.optim.Adam(list(twin.values()), lr=w.lr)
    for step in range(3):
        loss = w.training_step(batch, step)
        assert loss.dtype == torch.float64 and loss.requires_grad and loss is (w.mse_loss if case["regression"] else w.ce_loss)
        o_out, o_loss, o_grads = orc.step(cfg, {k: v.detach() for k, v in twin.items()}, x_dict, ei, y, B)
        assert abs(float(loss.detach()) - float(o_loss)) <= RTOL * abs(float(o_loss)), (step, float(loss.detach()), float(o_loss))
        opt.zero_grad()
        loss.backward()
        assert all(p.grad is None or p.grad.dtype == torch.float64 for p in w.model.parameters())
        opt.step()
        topt.zero_grad()
        for k, v in twin.items():
            v.grad = o_grads[k].clone()
        topt.step()
    assert not calls, "the training loss of an f64 model passed through the fp32 loss kernel"
    worst = max((_rel(p, twin[k]), k) for k, p in w.model.named_parameters())
    print(f"f64 wrapper {name}: after three Adam steps the worst parameter is {worst[0]:.3e} off its twin ({worst[1]})")
    assert worst[0] <= RTOL, worst
    moved = max(_rel(p, params[k]) for k, p in w.model.named_parameters())
    assert moved > 1e-6      # (the steps did move the parameters)
    key = "train_MSE_loss" if case["regression"] else "train_CE_loss"
    assert w.logged[key].dtype == torch.float64
    w.on_validation_epoch_start()
    with torch.no_grad():
        v = w.validation_step(batch, 0)
    assert v.dtype == torch.float64 and not v.requires_grad
    w.on_validation_epoch_end()
    ep = w.logged["val_MSE_loss" if case["regression"] else "val_CE_loss"]      # (the epoch value: the fp32 metric kernels' sums, as documented)
    assert abs(float(ep) - float(v)) <= 1e-5 * abs(float(v))


def test_evaluate_sequence_at_f64_is_the_forward_on_the_assembled_windows():
    """A model at "f64" takes none of the series routes: evaluate_sequence over a resident sequence assembles every batch and calls forward() -- its
    predictions are, bit for bit, the model's forward on `store.assemble`'s windows (fp32 rows at the engine pitch, widened)."""
    from morphsym_hgnn_amd import wrappers
    from tests import test_series_eval_gpu as se
    w, store, spec, n, dev = se._wrapper("a1c2_regression", "x3", False)
    w.model.set_precision("f64")
    ei1 = spec.topology.edge_index_dict(1, device=dev)
    stride, bs = 3, 32
    pred = wrappers.evaluate_sequence(w, store, ei1, bs, stride=stride)
    assert not w.model._engines or all(k[0] != "f64" for k in w.model._engines)
    starts = torch.arange(0, len(store), stride, device=dev)
    assert pred.dtype == torch.float64 and pred.shape[0] == starts.numel() and starts.numel() % bs != 0
    want = []
    with torch.no_grad():
        for lo in range(0, starts.numel(), bs):
            st = starts[lo:lo + bs]
            xs = store.assemble(st)[0]
            xd = {t: x.clone() for t, x in zip(store.recipe.node_types, xs)}
            want.append(w.model(x_dict=xd, edge_index_dict=spec.topology.edge_index_dict(int(st.numel()), device=dev)).reshape(-1, 12))
    assert torch.equal(pred, torch.cat(want))
    assert any(k.startswith("test_") for k in w.logged)


# ---- models.MLP -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss_kind", ["mse", "ce"])
def test_mlp_at_f64_matches_the_fp64_reference(loss_kind):
    """models.MLP at "f64" (operator route on the fp64 kernels, no casts) against tests/mlp_reference.reference -- torch's fp64 nn.Sequential -- at 1e-9:
    output, loss and every gradient, on one regression (MSE) and one classification (CE) shape, 300 rows (dW over 300 rows; three 64-row tiles and a tail)."""
    from morphsym_hgnn_amd import models
    from tests import mlp_reference as mr
    torch.set_default_dtype(torch.float32)
    in_c, hid, out_c, L, B = (450, 128, 12, 4, 300) if loss_kind == "mse" else (234, 256, 8, 3, 300)
    case = mr.random_case(in_c, hid, out_c, L, B, seed=5)
    m = models.MLP(in_c, hid, out_c, L, regression=loss_kind == "mse").set_precision("f64").to(DEV)
    src = {f"{2 * i}.{n}": t for i, (W, b) in enumerate(case["params"]) for n, t in (("weight", W), ("bias", b))}
    m.load_state_dict(src)
    assert all(p.dtype == torch.float64 and torch.equal(p.detach().cpu(), src[k]) for k, p in m.named_parameters())
    target = case["y"] if loss_kind == "mse" else case["labels"]
    ref = mr.reference(case["params"], case["x"], loss=loss_kind, target=target)
    out = m(case["x"].to(DEV))
    assert out.dtype == torch.float64 and not m._engines
    if loss_kind == "mse":
        loss = ((out - target.to(DEV)) ** 2).mean()
    else:
        loss = torch.nn.functional.cross_entropy(out.reshape(-1, 2), target.to(DEV).reshape(-1).long())
    loss.backward()
    errs = {"out": _rel(out, ref["out"]), "loss": _rel(loss, ref["loss"])}
    for i, (lin, (dW, db)) in enumerate(zip(m.linears(), ref["grads"])):
        errs[f"dW{i}"], errs[f"db{i}"] = _rel(lin.weight.grad, dW), _rel(lin.bias.grad, db)
    worst = max(errs, key=errs.get)
    print(f"f64 MLP {loss_kind}: worst {worst} {errs[worst]:.3e}")
    assert errs[worst] <= RTOL, errs
    assert m.fused_training_step(case["x"].to(DEV), target.to(DEV)) is None
