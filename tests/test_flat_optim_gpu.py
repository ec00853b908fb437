"""optim.FlatSGD / FlatAdam(weight_decay) / FlatAdamW, optim.clip_grad_norm_ and wrappers.GraphedTrainingStep with them, on the smallest golden case
(a1c2_h128_L3_d3_B3, three windows, 996 227 parameters).

Per-step arithmetic is held to the per-element checkers of tests/optim_reference.py (tests/test_optim_reference.py shows what they reject): the test writes
the gradients into the flat gradient buffer itself, so no forward amplifies a rounding, and runs the same three steps through torch's own optimizer on a
twin -- which must pass the same checkers: the control that the bounds are about rounding and nothing else.  Every optimizer is built with fp32-valued
hyperparameters (what the C ABI receives), so that torch's double scalars are the same numbers.  The captured steps are compared with eager twins bit for bit."""
import copy
import types

import pytest
import torch

from tests import helpers
from tests import optim_reference as orf

pytestmark = pytest.mark.gpu
CASE = "a1c2_h128_L3_d3_B3"
F = orf.f32


def _batch(x_dict, ei, y, B, dev):
    return types.SimpleNamespace(x_dict={k: v.to(dev) for k, v in x_dict.items()}, edge_index_dict={k: v.to(dev) for k, v in ei.items()},
                                 y=y.to(dev).flatten(), batch_size=B)


def _setup(n_batches=1, seed=300):
    torch.set_default_dtype(torch.float64)
    case, spec, fx, x_dict, y, params, ei = helpers.load_case(CASE)
    dev = torch.device("cuda")
    batches = [_batch(x_dict, ei, y, case["B"], dev)]
    for s in range(1, n_batches):
        g = torch.Generator().manual_seed(seed + s)
        xb = {k: torch.randn(v.shape, generator=g, dtype=torch.float64) * (0.0 if k == "foot" else 1.0) + (1.0 if k == "foot" else 0.0) for k, v in x_dict.items()}
        batches.append(_batch(xb, ei, torch.randn(y.shape, generator=g, dtype=torch.float64), case["B"], dev))
    return case, spec, params, batches, dev


def _new_wrapper(case, spec, params, batch, dev, optimizer="sgd", lr=1e-2, **attrs):
    from morphsym_hgnn_amd import wrappers
    _, cfg = helpers.load_group(case["cfg"])
    w = wrappers.HGNN_C2_Lightning_Reg(case["hidden"], case["layers"], spec.topology.metadata(), batch, optimizer=optimizer, lr=F(lr),
                                       grf_dimension=case["grf"], symmetry_mode="MorphSym" if cfg else None, group_operator_path=cfg).to(dev)
    w.model.load_state_dict(params)
    for k, v in attrs.items():
        setattr(w, k, v)
    return w


def _first_backward(w, batch):
    """One training_step + backward: the parameters become views of the flat buffer and their .grad views of the flat gradient buffer."""
    loss = w.training_step(batch, 0)
    loss.backward()
    assert all(p.grad is v for p, v in zip(w.model._param_list, w.model._gviews))
    return loss


def _real(model):
    """Positions of the flat buffers that belong to a parameter (every tensor starts at a multiple of 16 elements: the gaps belong to nobody)."""
    return torch.cat([torch.arange(o, o + n) for o, n in model._spec.param_offsets().values()])


def _gradients(model, steps=3):
    """Flat gradients in the style of the tables: exact zeros on three elements of four (whole parameter tensors of this project have them) and in the
    gaps between the tensors, magnitudes over eight decades on the rest, values of size 1 on the first and last two parameters."""
    n, real = model._flat.numel(), _real(model)
    out = []
    for s in range(steps):
        gen = torch.Generator().manual_seed(4243 + s)
        g = 10.0 ** (torch.rand(n, generator=gen, dtype=torch.float64) * 8.0 - 6.0) * (torch.randint(0, 2, (n,), generator=gen).double() * 2 - 1)
        g[torch.arange(n) % 4 != s] = 0.0
        g[real[:2]], g[real[-2:]] = torch.tensor([0.75, -1.5]), torch.tensor([1.25, -0.5])
        keep = torch.zeros(n, dtype=torch.bool)
        keep[real] = True
        g[~keep] = 0.0
        out.append(g.float())
    return out


def test_configure_optimizers_returns_the_flat_sgd_and_maximize_takes_torchs_route():
    from morphsym_hgnn_amd.optim import FlatSGD
    case, spec, params, batches, dev = _setup()
    w = _new_wrapper(case, spec, params, batches[0], dev, graph_safe_optimizer=True, device_lr_optimizer=True)
    opt = w.configure_optimizers()
    assert isinstance(opt, FlatSGD) and isinstance(opt, torch.optim.SGD) and opt._graph_safe and opt._device_lr and opt.defaults["lr"] == F(1e-2)
    assert type(w).device_lr_optimizer is False and type(w).graph_safe_optimizer is False
    _first_backward(w, batches[0])
    opt.step()
    assert opt._owner is w.model._flat and int(opt._t_dev.item()) == 1 and float(opt._lr_dev.item()) == F(1e-2)
    # maximize: torch's own step on the views, in the other direction
    w2 = _new_wrapper(case, spec, params, batches[0], dev)
    o2 = FlatSGD(w2.model, lr=F(1e-2), maximize=True)
    _first_backward(w2, batches[0])
    p0, g0 = w2.model._flat.clone(), w2.model._gflat.clone()
    o2.step()
    assert o2._owner is None and o2._flat_route() is None
    want = p0.double() + F(1e-2) * g0.double()
    assert bool(((w2.model._flat.double() - want).abs() <= 2.0 ** -22 * want.abs()).all()) and bool(g0.any())
    with pytest.raises(ValueError, match="[Nn]esterov"):
        FlatSGD(w2.model, lr=1e-2, nesterov=True)


OPTIMIZERS = {
    "sgd_nesterov_decay": ("sgd", dict(lr=1e-2, momentum=0.9, weight_decay=1e-3, nesterov=True)),
    "sgd_dampening": ("sgd", dict(lr=3e-3, momentum=0.5, dampening=0.25)),
    "sgd_plain": ("sgd", dict(lr=1e-2)),
    "adam_coupled_decay": ("adam", dict(lr=1e-3, weight_decay=1e-2)),
    "adamw": ("adamw", dict(lr=1e-3, weight_decay=1e-2)),
}


def _make(kind, kw, model, flat):
    from morphsym_hgnn_amd import optim
    kw = {k: (F(v) if isinstance(v, float) else v) for k, v in kw.items()}
    if kind == "adam":
        kw["betas"] = (F(0.9), F(0.999))
        return (optim.FlatAdam(model, **kw) if flat else torch.optim.Adam(model.parameters(), **kw)), kw
    if kind == "adamw":
        kw["betas"] = (F(0.9), F(0.999))
        return (optim.FlatAdamW(model, **kw) if flat else torch.optim.AdamW(model.parameters(), **kw)), kw
    return (optim.FlatSGD(model, **kw) if flat else torch.optim.SGD(model.parameters(), **kw)), kw


def _flat_state(opt, model, key):
    """The per-parameter state entries `key` of any optimizer laid out as the flat buffer, on the host (None when no parameter has one)."""
    parts = [opt.state.get(p, {}).get(key) for p in model._param_list]
    if all(x is None for x in parts):
        return None
    assert all(x is not None for x in parts)
    out = torch.zeros(model._flat.numel(), dtype=torch.float32)
    for (o, n), x in zip(model._spec.param_offsets().values(), parts):
        out[o:o + n] = x.detach().reshape(-1).float().cpu()
    return out


def _check_step(kind, kw, before, g, after, t):
    if kind == "sgd":
        hp = (kw["lr"], kw.get("momentum", 0.0), kw.get("dampening", 0.0), kw.get("weight_decay", 0.0), kw.get("nesterov", False), 1.0)
        case = dict(p=before["p"], g=g, buf=before["buf"], first=t == 1, t=t, n=g.numel(), hp=hp, exact=False)
        return orf.sgd_check(case, after["p"], after["buf"])
    hp = (kw["betas"][0], kw["betas"][1], F(1e-8), 1.0, kw["lr"], kw["weight_decay"], int(kind == "adamw"))
    case = dict(p=before["p"], g=g, m=before["m"], v=before["v"], t=t, n=g.numel(), hp=hp, exact=False)
    return orf.adamw_check(case, after["p"], after["m"], after["v"])


def _state(kind, opt, model):
    opt.state_dict()      # (publishes the flat optimizers' state; torch's: a no-op)
    n = model._flat.numel()
    s = dict(p=model._flat.detach().float().cpu().clone())
    if kind == "sgd":
        s["buf"] = _flat_state(opt, model, "momentum_buffer")
    else:
        m, v = _flat_state(opt, model, "exp_avg"), _flat_state(opt, model, "exp_avg_sq")
        s["m"], s["v"] = (torch.zeros(n) if m is None else m), (torch.zeros(n) if v is None else v)
    return s


@pytest.mark.parametrize("name", list(OPTIMIZERS))
def test_three_steps_and_the_state_round_trip_stay_within_the_per_element_bounds(name):
    """The flat optimizer and torch's own on a twin, three steps on gradients the test wrote, every step of both checked element by element from the state it
    started from; then the two state_dicts are exchanged (torch's layout both ways) and one more step on each side is checked the same way."""
    kind, kw0 = OPTIMIZERS[name]
    case, spec, params, batches, dev = _setup()
    a, b = (_new_wrapper(case, spec, params, batches[0], dev) for _ in range(2))
    oa, kw = _make(kind, kw0, a.model, True)
    for w in (a, b):
        _first_backward(w, batches[0])
    ob, _ = _make(kind, kw0, b.model, False)      # (after the first forward: its parameters are the flat views by now)
    assert isinstance(oa, type(ob)) and oa._flat_route() is not None
    if kind == "sgd" and kw.get("momentum", 0):
        assert oa.state_dict()["state"] == {} or all(s.get("momentum_buffer") is None for s in oa.state_dict()["state"].values())
    grads = _gradients(a.model, 4)
    for t in (1, 2, 3):
        for w, o, who in ((a, oa, "flat"), (b, ob, "torch")):
            before = _state(kind, o, w.model)
            if before.get("buf") is None and kind == "sgd":
                before["buf"] = torch.zeros_like(before["p"])
            w.model._gflat.copy_(grads[t - 1])
            o.step()
            d = _check_step(kind, kw, before, grads[t - 1], _state(kind, o, w.model), t)
            assert d is None, f"{name}, step {t}, {who}: {d}"
    assert oa._owner is a.model._flat and oa._t == 3
    # state round trip in torch's layout, both directions, then a fourth step on each side from the exchanged state
    sd_a, sd_b = copy.deepcopy(oa.state_dict()), copy.deepcopy(ob.state_dict())
    assert set(sd_a["state"]) == set(sd_b["state"]) and all(set(sd_a["state"][k]) == set(sd_b["state"][k]) for k in sd_a["state"])
    ob.load_state_dict(sd_a); oa.load_state_dict(sd_b)
    with torch.no_grad():      # (the parameters travel with the state)
        pa = a.model._flat.clone()
        a.model._flat.copy_(b.model._flat); b.model._flat.copy_(pa)
    for w, o, who in ((a, oa, "flat, torch's state"), (b, ob, "torch, the flat state")):
        before = _state(kind, o, w.model)
        w.model._gflat.copy_(grads[3])
        o.step()
        d = _check_step(kind, kw, before, grads[3], _state(kind, o, w.model), 4)
        assert d is None, f"{name}, step 4, {who}: {d}"
    assert oa._owner is a.model._flat


def test_flat_sgd_refuses_a_state_with_some_momentum_buffers_missing():
    from morphsym_hgnn_amd.optim import FlatSGD
    case, spec, params, batches, dev = _setup()
    w = _new_wrapper(case, spec, params, batches[0], dev)
    opt = FlatSGD(w.model, lr=1e-2, momentum=0.9)
    _first_backward(w, batches[0])
    opt.step()
    sd = copy.deepcopy(opt.state_dict())
    assert all(s["momentum_buffer"] is not None for s in sd["state"].values())
    sd["state"][0]["momentum_buffer"] = None
    opt.load_state_dict(sd)
    with pytest.raises(RuntimeError, match="momentum buffer"):
        opt.step()


def test_clip_grad_norm_matches_torch_and_falls_back_off_the_flat_route():
    from morphsym_hgnn_amd import optim
    case, spec, params, batches, dev = _setup()
    a, b = (_new_wrapper(case, spec, params, batches[0], dev) for _ in range(2))
    for w in (a, b):
        _first_backward(w, batches[0])
    g = _gradients(a.model, 1)[0]
    ref_norm = orf.norm_reference(g)
    for max_norm in (F(ref_norm / 3), F(ref_norm * 3)):
        for w in (a, b):
            w.model._gflat.copy_(g)
        got = optim.clip_grad_norm_(a.model, max_norm)
        assert got.dtype == torch.float64 and got.is_cuda
        assert orf.norm_check(dict(n=g.numel(), norm=ref_norm, exact=False), float(got)) is None
        case_c = dict(g=g, norm=float(got), max_norm=max_norm)
        d = orf.clip_check(case_c, a.model._gflat)
        assert d is None, d
        t = torch.nn.utils.clip_grad_norm_(b.model.parameters(), max_norm)      # fp32 norm: the control is loose there, the clipped values are compared
        assert abs(float(t) - ref_norm) <= 1e-5 * ref_norm
        assert bool(((b.model._gflat - a.model._gflat).abs() <= 4e-6 * a.model._gflat.abs()).all())
    again = optim.clip_grad_norm_(a.model, 1.0)
    assert again.data_ptr() == got.data_ptr(), "the norm is one static tensor per model"
    a.zero_grad(set_to_none=True)      # no flat views any more: torch's own function, on no gradients
    assert float(optim.clip_grad_norm_(a.model, 1.0)) == 0.0


# ---------------------------------------------------------------------------------------------------
# wrappers.GraphedTrainingStep
# ---------------------------------------------------------------------------------------------------
def _eager(w, opt, batch, max_grad_norm=None):
    from morphsym_hgnn_amd import optim
    opt.zero_grad(set_to_none=True)
    loss = w.training_step(batch, 0)
    loss.backward()
    norm = None if max_grad_norm is None else float(optim.clip_grad_norm_(w.model, max_grad_norm))
    opt.step()
    return float(loss.detach()), norm


def _same_parameters(a, b):
    for p, q in zip(a.model.parameters(), b.model.parameters()):
        assert torch.equal(p.detach(), q.detach())


@pytest.mark.parametrize("which", ["sgd_momentum", "adamw"])
def test_graphed_training_step_replays_flat_sgd_and_flat_adamw_bit_for_bit(which):
    from morphsym_hgnn_amd import optim, wrappers
    case, spec, params, batches, dev = _setup(4)
    a, b = (_new_wrapper(case, spec, params, batches[0], dev) for _ in range(2))

    def make(w, graph_safe):
        if which == "adamw":
            return optim.FlatAdamW(w.model, lr=F(1e-3), graph_safe=graph_safe)
        return optim.FlatSGD(w.model, lr=F(1e-2), momentum=F(0.9), graph_safe=graph_safe)
    oa, ob = make(a, True), make(b, False)
    before = [p.detach().clone() for p in a.parameters()]
    gs = wrappers.GraphedTrainingStep(a, oa, batches[0])
    for p, q in zip(a.parameters(), before):
        assert torch.equal(p.detach().float(), q.float()), "building the graph must not train"
    assert int(oa._t_dev.item()) == 0 and not bool(oa._bufs[0].any())
    la = [float(gs(bt)) for bt in batches[1:]]
    lb = [_eager(b, ob, bt)[0] for bt in batches[1:]]
    torch.cuda.synchronize()
    assert la == lb, (la, lb)
    _same_parameters(a, b)
    assert int(oa._t_dev.item()) == 3 and ob._t == 3
    sa, sb = oa.state_dict()["state"], ob.state_dict()["state"]
    for k in sa:
        for name in sa[k]:
            assert torch.equal(torch.as_tensor(sa[k][name]).cpu().double(), torch.as_tensor(sb[k][name]).cpu().double()), (k, name)
    with pytest.raises(ValueError, match="graph_safe"):
        wrappers.GraphedTrainingStep(b, ob, batches[0])


def test_graphed_training_step_follows_a_scheduler_through_the_device_lr():
    """device_lr + StepLR(step_size=1, gamma=0.5): three replays == three eager steps under the same schedule (an eager twin WITHOUT device_lr: the learning
    rate as a launch argument gives the same bits), and nothing raises; without device_lr the changed lr still raises."""
    from morphsym_hgnn_amd import optim, wrappers
    case, spec, params, batches, dev = _setup(4)
    a = _new_wrapper(case, spec, params, batches[0], dev, graph_safe_optimizer=True, device_lr_optimizer=True)
    b = _new_wrapper(case, spec, params, batches[0], dev)
    oa, ob = a.configure_optimizers(), optim.FlatSGD(b.model, lr=F(1e-2))
    assert isinstance(oa, optim.FlatSGD) and oa._device_lr and oa._graph_safe
    gs = wrappers.GraphedTrainingStep(a, oa, batches[0])
    scha, schb = (torch.optim.lr_scheduler.StepLR(o, step_size=1, gamma=0.5) for o in (oa, ob))
    for k, bt in enumerate(batches[1:]):
        la = float(gs(bt))
        lb, _ = _eager(b, ob, bt)
        assert la == lb, (k, la, lb)
        assert float(oa._lr_dev.item()) == F(oa.param_groups[0]["lr"]) == F(F(1e-2) * 0.5 ** k)
        scha.step(); schb.step()
    torch.cuda.synchronize()
    _same_parameters(a, b)
    assert oa.param_groups[0]["lr"] == ob.param_groups[0]["lr"] == F(1e-2) * 0.125
    c = _new_wrapper(case, spec, params, batches[0], dev, graph_safe_optimizer=True)
    oc = c.configure_optimizers()
    gc = wrappers.GraphedTrainingStep(c, oc, batches[0])
    gc(batches[1])
    oc.param_groups[0]["lr"] *= 0.5
    with pytest.raises(RuntimeError, match="lr"):
        gc(batches[2])


def test_graphed_training_step_clips_inside_the_graph():
    from morphsym_hgnn_amd import optim, wrappers
    case, spec, params, batches, dev = _setup(4)
    a, b = (_new_wrapper(case, spec, params, batches[0], dev) for _ in range(2))
    oa, ob = optim.FlatSGD(a.model, lr=F(1e-2), momentum=F(0.9), graph_safe=True), optim.FlatSGD(b.model, lr=F(1e-2), momentum=F(0.9))
    _, n0 = _eager(b, optim.FlatSGD(b.model, lr=0.0), batches[0], max_grad_norm=1e30)      # (a step that moves nothing: the size of this model's gradient norm)
    max_norm = F(n0 / 4)
    gs = wrappers.GraphedTrainingStep(a, oa, batches[0], max_grad_norm=max_norm)
    assert gs.grad_norm is not None and gs.grad_norm.dtype == torch.float64 and gs.grad_norm.is_cuda
    for bt in batches[1:]:
        la = float(gs(bt))
        na = float(gs.grad_norm)
        lb, nb = _eager(b, ob, bt, max_grad_norm=max_norm)
        assert la == lb and na == nb and na > max_norm, (la, lb, na, nb, max_norm)
    torch.cuda.synchronize()
    _same_parameters(a, b)


def test_load_state_dict_after_capture_fills_the_buffers_the_graph_addresses():
    """As the FlatAdam test of tests/test_wrappers.py, for FlatSGD with momentum: two replays, snapshot, two more (A); parameters and state put back, the
    same two batches again -> A's bits; the momentum buffer and the step count at the same addresses."""
    from morphsym_hgnn_amd import optim, wrappers
    case, spec, params, batches, dev = _setup(4)
    w = _new_wrapper(case, spec, params, batches[0], dev)
    opt = optim.FlatSGD(w.model, lr=F(1e-2), momentum=F(0.9), weight_decay=F(1e-3), graph_safe=True)
    gs = wrappers.GraphedTrainingStep(w, opt, batches[0])
    for bt in batches[:2]:
        gs(bt)
    torch.cuda.synchronize()
    snap_p = [p.detach().clone() for p in w.model.parameters()]
    snap_o = copy.deepcopy(opt.state_dict())
    assert all(s["momentum_buffer"] is not None for s in snap_o["state"].values())
    addr = (opt._bufs[0].data_ptr(), opt._t_dev.data_ptr())
    la = [float(gs(bt)) for bt in batches[2:]]
    a = [p.detach().clone() for p in w.model.parameters()]
    buf_a = opt._bufs[0].clone()
    with torch.no_grad():
        for p, q in zip(w.model.parameters(), snap_p):
            p.copy_(q)
    opt.load_state_dict(snap_o)
    assert (opt._bufs[0].data_ptr(), opt._t_dev.data_ptr()) == addr, "load_state_dict re-allocated the flat state a captured step addresses"
    assert int(opt._t_dev.item()) >= 1
    lb = [float(gs(bt)) for bt in batches[2:]]
    torch.cuda.synchronize()
    assert la == lb
    for p, q in zip(w.model.parameters(), a):
        assert torch.equal(p.detach(), q), "the replays after load_state_dict did not continue from the loaded state"
    assert torch.equal(opt._bufs[0], buf_a)
