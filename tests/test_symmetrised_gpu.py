"""Symmetrisation at model level (morphsym_hgnn_amd/symmetrise.py): the equivariance defect of our own kernels against the fp64 oracle's, the orbit-averaged
prediction, a `Symmetrised` wrapper's training step against the manual composition, `evaluate_sequence_symmetrised`, and the refusals.

Fixtures: the sequences of tests/test_windows.py (tw.SEQ / tw.SEQ4, their T), hidden 128, 2 layers.  A1 with the C2 orbit {e, gs} (K = 2, 17 base windows),
MiniCheetah-K4 contact classification with the whole group (K = 4, 5 base windows).

Tolerances -- no new number: `tol` is the project's contract of a plan against the fp64 oracle, relative to the output's largest magnitude: 1e-4 for the f32
and x3 plans, the bf16 plan's forward bound of tests/test_full_size_gpu.py (BF16_VS_EXACT).  Every output value is within tol max|o_0| of the oracle's, so a
difference of two of them -- and with it the rms and the maximum of the differences -- is within the MARGIN 2 tol max|o_0| of the oracle's own.

Measured on an MI355X (rms of the defect over max|o_0|; the architecture promises 0): see DESIGN.md section 8."""
import functools
import types

import numpy as np
import pytest
import torch

from tests import helpers
from tests import orbit_reference as orb
from tests import test_full_size_gpu as fs
from tests import test_window_symmetry as ws
from tests import test_windows as tw

pytestmark = pytest.mark.gpu
T = tw.T
TOL = {"f32": 1e-4, "x3": 1e-4, "bf16": fs.BF16_VS_EXACT}
PLANS = ("f32", "x3", "bf16")
MI_SEED = 7      # parameters for which the fp64 oracle's MI-HGNN defect under gs is 0.527 max|o_0| (checked on the CPU for seeds 1 .. 12: 0.19 .. 0.53; the test asserts >= 10 margins)


def _kind(kind):
    """(recipe, spec, sequence, group, operators, base windows, parameter seed)"""
    from morphsym_hgnn_amd.windows import quadsdk_a1_c2_recipe, minicheetah_k4_recipe
    if kind == "a1c2":
        return quadsdk_a1_c2_recipe(tw.JP, tw.FP, T, 3), helpers.make_spec("c2", "a1-c2", "a1-c2", 128, 2), tw.SEQ, ws.A1, ("gs",), 17, 8
    if kind == "mck4":
        return (minicheetah_k4_recipe(tw.JP, tw.FP, T), helpers.make_spec("k4", "mini_cheetah-k4", "mini_cheetah-k4", 128, 2, regression=False), tw.SEQ4, ws.K4,
                ("gs", "gt", "gr"), 5, 8)
    if kind == "mcc2":      # the C2 model on MiniCheetah contact classification (two base nodes), the C2 orbit {e, gs}
        from morphsym_hgnn_amd.windows import GroupAction
        return (minicheetah_k4_recipe(tw.JP, tw.FP, T, n_base=2), helpers.make_spec("c2", "mini_cheetah-c2", "mini_cheetah-c2", 128, 2, regression=False), tw.SEQ4,
                GroupAction.load("mini_cheetah-c2"), ("gs",), 5, 8)
    return quadsdk_a1_c2_recipe(tw.JP, tw.FP, T, 3, n_base=1), helpers.make_spec("mi", "quadruped-mi", "", 128, 2, grf=3), tw.SEQ, ws.A1, ("gs",), 17, MI_SEED


def _starts(n, B):
    st = torch.randint(0, n, (B,), generator=torch.Generator().manual_seed(B))
    st[0], st[-1] = 0, n - 1
    return st


def _orbit(kind, plan):
    from morphsym_hgnn_amd.symmetrise import OutputAction
    from morphsym_hgnn_amd.windows import SequenceStore
    recipe, spec, seq, group, ops, B, seed = _kind(kind)
    orbit = SequenceStore(seq, recipe, dtype=plan).orbit(group, ops)
    return orbit, OutputAction.from_store(orbit, spec.regression)


def _mapped(o, act, B, e):
    """rho(g_e)^-1 of element e's block, fp64 numpy [B, row]"""
    pinv = orb.inverse(act.perm[e])
    sg = np.asarray(act.sign[e], dtype=np.float64)[pinv]
    return (o[e * B:(e + 1) * B].reshape(B, act.n_units, act.width)[:, pinv, :] * sg[None, :, None]).reshape(B, -1)


@functools.lru_cache(maxsize=None)
def _oracle(kind):
    """The fp64 oracle on the K assembled element windows (the fp32 store's windows: the raw series' fp32 values), once per kind: (o [K B, row], per
    operator (rms, max) of its own defect, the fp64 average, max|o_0|)."""
    from morphsym_hgnn_amd import synth
    from oracle import ms_hgnn_oracle as orc
    recipe, spec, seq, group, ops, B, seed = _kind(kind)
    orbit, act = _orbit(kind, "f32")
    K = act.n_elements
    wb = orbit.orbit_batch(_starts(len(orbit), B), None)
    xs, _, _ = orbit.assemble(wb.starts)
    x = {t: xs[i][:, :recipe.width(t)].double().cpu() for i, t in enumerate(recipe.node_types)}
    params = synth.make_params(seed, spec.param_shapes())
    with torch.no_grad():
        o = orc.forward(helpers.oracle_config(spec), params, x, spec.topology.edge_index_dict(K * B)).reshape(K * B, act.row).numpy()
    back = [_mapped(o, act, B, e) for e in range(K)]
    defect = [(float(np.sqrt(((t - back[0]) ** 2).mean())), float(np.abs(t - back[0]).max())) for t in back[1:]]
    return o, defect, sum(back) / K, float(np.abs(o[:B]).max())


def _engine_outputs(kind, plan, starts=None):
    """our kernels on the same orbit-complete batch: (out [K B, row] on the device, the action, B)"""
    from morphsym_hgnn_amd import engine as eng, synth
    recipe, spec, seq, group, ops, B, seed = _kind(kind)
    orbit, act = _orbit(kind, plan)
    e = eng.Engine(spec, plan)
    flat = eng.flatten_params(spec, synth.make_params(seed, spec.param_shapes()), e.device)
    st = orbit.orbit_batch(_starts(len(orbit), B), None).starts if starts is None else starts(orbit, B)
    xs, _, _ = orbit.assemble(st)
    n = int(st.numel())
    return e.forward(xs, flat, n, training=False).reshape(n, act.row).clone(), act, B


def _check_report(rep, act, want, margin, B, what):
    for op, (rms, mx) in zip(act.operators[1:], want):
        r = rep[str(op)]
        print(f"{what} {op}: rms {r['rms']:.3e} (oracle {rms:.3e}), max {r['max_abs']:.3e} (oracle {mx:.3e}), relative rms {r['relative_rms']:.3e}, margin {margin:.3e}")
        assert r["n"] == B * act.row
        assert abs(r["rms"] - rms) <= margin and abs(r["max_abs"] - mx) <= margin, (what, op, r, rms, mx, margin)


@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("kind", ["a1c2", "mck4"])
def test_the_defect_of_the_equivariant_models_is_the_oracles_within_the_plans_contract(kind, plan):
    """MS-HGNN is equivariant by architecture: the oracle's own defect is at rounding level, and the report of our kernels (neighbour sums in permuted order,
    bf16 roundings) agrees with it within the margin.  The averaged prediction is the fp64 average of the oracle's blocks within tol."""
    from morphsym_hgnn_amd import symmetrise as sym
    o_ref, d_ref, avg_ref, scale = _oracle(kind)
    assert all(rms <= 1e-12 * scale and mx <= 1e-12 * scale for rms, mx in d_ref), d_ref      # the reference value: rounding level in fp64
    out, act, B = _engine_outputs(kind, plan)
    assert act.n_elements == (2 if kind == "a1c2" else 4) and B == (17 if kind == "a1c2" else 5)
    margin = 2 * TOL[plan] * scale
    d = sym.EquivarianceDefect(act)
    d.update(out, B)
    _check_report(d.report(), act, d_ref, margin, B, f"{kind}/{plan}")
    err = float(np.abs(out.double().cpu().numpy() - o_ref).max())
    avg = sym.orbit_average(out, act, B).double().cpu().numpy()
    print(f"{kind}/{plan}: output error {err / scale:.3e}, average error {np.abs(avg - avg_ref).max() / scale:.3e} of max|o_0| = {scale:.3e}")
    assert err <= TOL[plan] * scale                                         # (the contract itself, on this batch)
    assert np.abs(avg - avg_ref).max() <= TOL[plan] * scale
    if kind == "mck4":
        assert not np.array_equal(o_ref[B:2 * B], o_ref[:B])                # the blocks differ: the average is not vacuous


@pytest.mark.parametrize("plan", PLANS)
def test_the_defect_of_mi_hgnn_is_the_oracles_and_the_symmetrised_model_has_none(plan):
    """MI-HGNN is not equivariant: with the seed picked on the CPU the oracle's defect under gs is at least 10 margins, our report agrees within one margin,
    and the symmetrised model -- fed the orbit of x and the orbit of gs x -- has a defect within the margin of zero."""
    from morphsym_hgnn_amd import symmetrise as sym
    o_ref, d_ref, avg_ref, scale = _oracle("mi")
    margin = 2 * TOL[plan] * scale
    assert d_ref[0][0] >= 10 * margin, (d_ref, margin)
    out, act, B = _engine_outputs("mi", plan)
    d = sym.EquivarianceDefect(act)
    d.update(out, B)
    _check_report(d.report(), act, d_ref, margin, B, f"mi/{plan}")
    avg = sym.orbit_average(out, act, B)
    assert np.abs(avg.double().cpu().numpy() - avg_ref).max() <= TOL[plan] * scale

    def both_orbits(orbit, B):      # the orbit of x = {x, gs x}, then the orbit of gs x = {gs x, gs gs x = x}
        st = _starts(len(orbit), B).cuda()
        el = torch.tensor([0] * B + [1] * B + [1] * B + [0] * B, dtype=torch.int64).cuda()
        return orbit.pack_starts(st.repeat(4), el)
    out2, _, _ = _engine_outputs("mi", plan, both_orbits)
    sym_x, sym_gx = sym.orbit_average(out2[:2 * B], act, B), sym.orbit_average(out2[2 * B:], act, B)
    d.reset()
    d.update(torch.cat([sym_x, sym_gx]), B)
    rep = d.report()["gs"]
    print(f"mi/{plan} symmetrised: rms {rep['rms']:.3e}, max {rep['max_abs']:.3e}, margin {margin:.3e}")
    assert rep["rms"] <= margin and rep["max_abs"] <= margin and rep["n"] == B * act.row


# ---- the wrappers ----------------------------------------------------------------------------------------------------------------------------------------

def _wrapper(kind, plan, monkeypatch):
    """(wrapper, orbit store, action, spec or None, B) on the fixture of `kind`; "mlp": MLP_Lightning on the A1 sequence"""
    from morphsym_hgnn_amd import wrappers
    from morphsym_hgnn_amd.symmetrise import OutputAction
    from morphsym_hgnn_amd.windows import SequenceStore, quadsdk_a1_mlp_recipe
    dev = torch.device("cuda")
    torch.set_default_dtype(torch.float32)
    monkeypatch.setenv("MSHGNN_DTYPE", plan)
    torch.manual_seed(3)
    if kind == "mlp":
        recipe = quadsdk_a1_mlp_recipe(tw.JP, tw.FP, T, 3)
        orbit = SequenceStore(tw.SEQ, recipe, dtype=plan).orbit(ws.A1, ("gs",))
        w = wrappers.MLP_Lightning(recipe.width("mlp"), 128, 12, 2, batch_size=17).to(dev)
        return w, orbit, OutputAction.from_store(orbit, True), None, 17
    recipe, spec, seq, group, ops, B, seed = _kind(kind)
    orbit, act = _orbit(kind, plan)
    xs, _, _ = orbit.assemble([0, 1])
    dummy = types.SimpleNamespace(edge_index_dict=spec.topology.edge_index_dict(2, device=dev),
                                  x_dict={t: x[:, :recipe.width(t)].float().contiguous() for t, x in zip(recipe.node_types, xs)})
    meta = spec.topology.metadata()
    if kind == "a1c2":
        _, cfg = helpers.load_group("a1-c2")
        w = wrappers.HGNN_C2_Lightning_Reg(128, 2, meta, dummy, symmetry_mode="MorphSym", group_operator_path=cfg)
    elif kind == "mck4":
        _, cfg = helpers.load_group("mini_cheetah-k4")
        w = wrappers.HGNN_K4_Lightning(128, 2, meta, dummy, regression=False, symmetry_mode="MorphSym", group_operator_path=cfg)
    elif kind == "mcc2":
        _, cfg = helpers.load_group("mini_cheetah-c2")
        w = wrappers.HGNN_C2_Lightning_Cls(128, 2, meta, dummy, regression=False, symmetry_mode="MorphSym", group_operator_path=cfg)
    else:
        w = wrappers.Heterogeneous_GNN_Lightning(128, 2, meta, dummy, grf_dimension=3)
    return w.to(dev), orbit, act, spec, B


@pytest.mark.parametrize("kind,plan,on_instance", [("mi", "x3", False), ("mi", "bf16", True), ("a1c2", "f32", True), ("mck4", "bf16", False), ("mcc2", "x3", True),
                                                   ("mlp", "bf16", True)])
def test_a_symmetrised_training_step_equals_the_manual_composition(kind, plan, on_instance, monkeypatch):
    """Symmetrised(w).training_step on an orbit-complete batch: loss and the WHOLE flat gradient equal, by torch.equal, engine forward -> the mirror's average ->
    the wrappers' device loss (`mse_loss` / `ce_loss` of metrics.StepMetrics, what the two-call route of every wrapper returns) -> the mirror's backward ->
    engine backward.  One FlatAdam step then changes the parameters; the one-call fused step is not taken -- also not when the wrapper carries
    `fused_training_step = True` on the INSTANCE (on_instance: wrappers.py documents the attribute as set per wrapper or on the class), through each of the three
    `training_step`s that look at it (_HGNNWrapper's, HGNN_C2_Lightning_Reg's, MLP_Lightning's)."""
    from morphsym_hgnn_amd import symmetrise as sym
    from morphsym_hgnn_amd.metrics import StepMetrics
    w, orbit, act, spec, B = _wrapper(kind, plan, monkeypatch)
    K, dev = act.n_elements, torch.device("cuda")
    ei = spec.topology.edge_index_dict(K * B, device=dev) if spec is not None else None
    if on_instance:
        w.fused_training_step = True
    s = sym.Symmetrised(w, act)
    assert ("fused_training_step" in w.__dict__) == on_instance and s.__dict__["fused_training_step"] is False
    assert s.raw is w and s.model is w.model and s.fused_training_step is False and w.fused_training_step is True and type(w).__name__ in type(s).__name__
    wb = orbit.orbit_batch(_starts(len(orbit), B), ei)
    assert wb.batch_size == K * B and torch.equal(wb.elements.cpu(), torch.arange(K).repeat_interleave(B))
    w.model.zero_grad()
    loss = s.training_step(wb, 0)
    assert w.model._gpend_id == 0                                  # not the one-call engine step
    assert loss is (s.mse_loss if w.regression else s.ce_loss) and w.mse_loss is None and w.ce_loss is None      # the view keeps its own metric state
    loss.backward()
    torch.cuda.synchronize()
    got_loss, got_flat = loss.detach().clone(), w.model._gflat.clone()
    assert bool(got_flat.any()) and bool(torch.isfinite(got_flat).all())

    # the manual composition
    m = w.model
    pdev = next(m.parameters()).device      # (cuda:0 -- the key of the model's own engine)
    e, flat = m._engine(pdev), m._flat_params(pdev)
    if kind == "mlp":
        x = e.cast_input(wb.x_dict["mlp"][:, :m.in_channels].detach())
        out = e.forward(x, flat, training=True)
    else:
        x = e.cast_inputs(wb.x_dict)
        out = e.forward(x, flat, K * B, training=True)
    o = out.reshape(K * B, act.row).cpu().numpy()
    avg = torch.from_numpy(orb.average(o, act.perm, act.sign, act.width, B)).to(dev).requires_grad_()
    y = wb.y[:B]
    sm = StepMetrics(regression=w.regression)
    sm.calculate_losses_step(y.reshape(B, -1), avg)
    want_loss = sm.mse_loss if w.regression else sm.ce_loss
    (g,) = torch.autograd.grad(want_loss, avg)
    go = torch.from_numpy(orb.average_backward(g.cpu().numpy(), act.perm, act.sign, act.width, B)).to(dev).reshape(out.shape).contiguous()
    want_flat = e.backward(x, flat, go) if kind == "mlp" else e.backward(x, flat, go, K * B)
    torch.cuda.synchronize()
    assert torch.equal(got_loss, want_loss.detach()) and torch.equal(got_flat, want_flat)
    if kind in ("mi", "mlp"):      # not the raw model's step on the same batch (an equivariant model's two losses agree up to rounding)
        w.model.zero_grad()
        w.fused_training_step = False
        raw_loss = w.training_step(wb, 0)
        assert not torch.equal(raw_loss.detach(), got_loss)
        raw_loss.backward()
        if on_instance:      # ... nor the one-call step the raw wrapper takes with the flag set: the route the view must not take
            w.model.zero_grad()
            w.fused_training_step = True
            fused_loss = w.training_step(orbit.orbit_batch(_starts(len(orbit), B), ei), 0)
            assert w.model._gpend_id == 1 and not torch.equal(fused_loss.detach().reshape(()).double(), got_loss.reshape(()).double())
            fused_loss.backward()

    # Adam on the flat buffers, driven through the view
    w.model.zero_grad()
    s.training_step(wb, 1).backward()
    opt = s.configure_optimizers()
    before = [p.detach().clone() for p in w.model.parameters()]
    opt.step()
    torch.cuda.synchronize()
    assert any(not torch.equal(a, p.detach()) for a, p in zip(before, w.model.parameters()))
    # evaluation under no_grad: the labels of the first B windows, the averaged prediction in the wrapper's own shape
    with torch.no_grad():
        yv, pv = s.step_helper_function(orbit.orbit_batch(_starts(len(orbit), B), ei))
        v = s.validation_step(orbit.orbit_batch(_starts(len(orbit), B), ei), 0)
    assert yv.shape[0] == B and pv.shape == (B, act.row) and not pv.requires_grad and bool(torch.isfinite(v))


@pytest.mark.parametrize("plan", ["bf16", "x3"])
def test_evaluate_sequence_symmetrised_equals_the_batch_by_batch_composition(plan, monkeypatch):
    """Two sequences in one ResidentDataset, the C2 orbit, every third base window, 4 base windows per batch (4, 4, ..., ragged): predictions bit for bit,
    the report that of one EquivarianceDefect fed the same batches."""
    from morphsym_hgnn_amd import symmetrise as sym, wrappers
    from morphsym_hgnn_amd.windows import ResidentDataset
    from oracle.gen_window_golden import synthetic_sequence
    w, _, _, spec, _ = _wrapper("mi", plan, monkeypatch)
    recipe = _kind("mi")[0]
    ds = ResidentDataset([synthetic_sequence(7100, 160), synthetic_sequence(7113, 171)], recipe, dtype=plan)
    orbit = ds.orbit(ws.A1, ("gs",))
    act = sym.OutputAction.from_store(orbit.view(), True)
    view, K = orbit.view(), 2
    assert view.n_windows == 11 + 22 and len(view) == K * 33
    dev = torch.device("cuda")
    ei1 = spec.topology.edge_index_dict(1, device=dev)
    preds, report = sym.evaluate_sequence_symmetrised(w, view, ei1, 4, stride=3)
    base = torch.arange(0, 33, 3, device=dev)
    d, want = sym.EquivarianceDefect(act), []
    with torch.no_grad():
        for lo in range(0, int(base.numel()), 4):
            ix = base[lo:lo + 4]
            b = int(ix.numel())
            wb = view.orbit_batch(ix, spec.topology.edge_index_dict(K * b, device=dev))
            assert torch.equal(wb.starts.cpu(), view.starts(torch.cat([ix.cpu(), ix.cpu() + 33])).cpu())
            _, yp = w.step_helper_function(wb)
            d.update(yp, b)
            want.append(sym.orbit_average(yp, act, b).clone())
    assert preds.shape == (11, 12) and torch.equal(preds, torch.cat(want)) and report == d.report()
    assert report["gs"]["n"] == 11 * 12 and report["gs"]["rms"] > 0
    # the Symmetrised view gives the same sweep, through its own action; the whole dataset stands for its view
    p2, r2 = sym.evaluate_sequence_symmetrised(sym.Symmetrised(w, act), orbit, ei1, 4, stride=3)
    assert torch.equal(p2, preds) and r2 == report
    view.check()


def test_refusals(monkeypatch):
    from morphsym_hgnn_amd import symmetrise as sym, wrappers
    from morphsym_hgnn_amd.windows import SequenceStore
    w, orbit, act, spec, B = _wrapper("a1c2", "bf16", monkeypatch)
    dev = torch.device("cuda")
    com = wrappers.COM_MLP_Lightning(24, 128, 6, 2, batch_size=4, stats=(np.zeros(6), np.ones(6)))
    with pytest.raises(ValueError, match="COM"):
        sym.Symmetrised(com, act)
    s = sym.Symmetrised(w, act)
    wb = orbit.batch(_starts(len(orbit), 2 * B - 1), spec.topology.edge_index_dict(2 * B - 1, device=dev))
    with pytest.raises(ValueError, match="no multiple"):
        with torch.no_grad():
            s.step_helper_function(wb)
    recipe, _, seq, group, ops, _, _ = _kind("a1c2")
    store = SequenceStore(seq, recipe, dtype="bf16")
    with pytest.raises(ValueError, match="identity=False"):
        sym.OutputAction.from_store(store.orbit(group, ("gs", "gt"), identity=False), True)
    with pytest.raises(ValueError, match="single group element"):
        sym.OutputAction.from_store(store, True)
    with pytest.raises(ValueError, match="one group element"):
        store.orbit_batch([0, 1], None)
    with pytest.raises(IndexError):
        orbit.orbit_batch([0, len(orbit)], None)
    cls_act = sym.OutputAction.from_tables([[0, 1, 2, 3], [1, 0, 3, 2]], [[1] * 4] * 2, 2)
    with pytest.raises(ValueError, match="width"):
        sym.Symmetrised(w, cls_act)
