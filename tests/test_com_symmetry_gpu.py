"""The Solo centroidal-momentum windows under the symmetry group on the GPU: the stores' transformed / orbit windows against the action stated from the yaml
(tests/com_symmetry_reference.py), the K4 model on orbit batches against the fp64 oracle, `wrappers.evaluate_table` for the COM wrappers and `Symmetrised`
on the baselines.

Fixture: three synthetic Solo sequences of 120, 97 and 83 rows (X, Y random, the base series zeros as in the dataset) in one ResidentDataset; batches of 5, 64
and 257 windows.  Tolerances -- no new number: 1e-4 max|out| is the split plan's contract against the fp64 oracle (tests/test_symmetrised_gpu.py's TOL), the
sums are compared within the summation bounds tests/test_com_segmented_gpu.py derives."""
import io
import types

import numpy as np
import pytest
import torch

from morphsym_hgnn_amd import metrics as M
from tests import com_symmetry_reference as cr
from tests import helpers
from tests import metrics_reference as mr
from tests import orbit_reference as orb
from tests import test_windows as tw

pytestmark = pytest.mark.gpu
ROWS, NAMES = (120, 97, 83), ["trot", "walk", "bound"]
OPS = cr.OPS
JP = tw.JP
STATS = (np.zeros(6), np.ones(6))
TOL = 1e-4          # the split plan against the fp64 oracle, relative to max|out|
_CACHE = {}


def _seqs():
    from morphsym_hgnn_amd.windows import solo_com_arrays
    if "seqs" not in _CACHE:
        rng = np.random.default_rng(2024)
        _CACHE["seqs"] = [solo_com_arrays(rng.standard_normal((n, 24)).astype(np.float32), rng.standard_normal((n, 6)).astype(np.float32)) for n in ROWS]
        _CACHE["cat"] = {s: np.concatenate([q[s] for q in _CACHE["seqs"]], 0) for s in _CACHE["seqs"][0]}
    return _CACHE["seqs"], _CACHE["cat"]


def _recipe(kind, history=1):
    from morphsym_hgnn_amd.windows import solo_com_mlp_recipe, solo_com_recipe
    name = cr.KINDS[kind][0]
    return solo_com_mlp_recipe(JP, history, symmetry=True) if name is None else solo_com_recipe(name, JP, history, symmetry=True)


def _dataset(kind, history=1, dtype="x3"):
    from morphsym_hgnn_amd.windows import GroupAction, ResidentDataset
    return ResidentDataset(_seqs()[0], _recipe(kind, history), dtype=dtype, names=NAMES), GroupAction.load(cr.KINDS[kind][2])


# ---- 1. the stores ---------------------------------------------------------------------------------------------------------------------------------------
def _check_windows(recipe, dtype, xs, y, want):
    """xs / y of an assembly against `want` = [(x by type, labels)] per window, bit for bit (a copy with sign flips; bf16: the one rounding of the copy)."""
    B = len(want)
    for ti, t in enumerate(recipe.node_types):
        ref = torch.from_numpy(np.stack([w[0][t] for w in want]).astype(np.float32)).reshape(B * recipe.num_nodes[t], -1)
        got = xs[ti][:, :recipe.width(t)].cpu()
        assert torch.equal(got, ref.to(got.dtype)), t
        assert not bool(xs[ti][:, recipe.width(t):].any())
    assert torch.equal(y.cpu(), torch.from_numpy(np.stack([w[1] for w in want]).astype(np.float32)))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("history", [1, 4])
@pytest.mark.parametrize("kind", list(cr.KINDS))
def test_transformed_and_orbit_stores_assemble_the_yaml_action(kind, history, dtype):
    ds, group = _dataset(kind, history, dtype)
    raw, cat = cr.load(cr.KINDS[kind][2]), _seqs()[1]
    recipe = ds.recipe
    view = ds.view()
    base = [0, 3, view.cum[1] - 1, view.cum[1], view.n_windows - 1]          # dataset indices: first / last windows of sequences
    rows = [int(r) for r in view.starts(base).cpu()]
    want = {op: [cr.window(raw, op, kind, cat, r, history, JP) for r in rows] for op in (None,) + OPS}
    _check_windows(recipe, dtype, *ds.assemble(rows)[:2], want[None])
    orbit = ds.orbit(group)
    assert orbit.n_elements == 4 and orbit.operators == [None, "gs", "gt", "gr"]
    for e, op in enumerate((None,) + OPS):
        if op is not None:
            _check_windows(recipe, dtype, *ds.transformed(op, group).assemble(rows)[:2], want[op])
        _check_windows(recipe, dtype, *orbit.assemble(rows, elements=[e] * len(rows))[:2], want[op])
    every = [w for op in (None,) + OPS for w in want[op]]          # element-major: window e * B + w
    wb = orbit.orbit_batch(rows, None)
    _check_windows(recipe, dtype, [wb.x_dict[t] for t in recipe.node_types], wb.y, every)
    oview = orbit.view()
    assert oview.segment_shape == (4, 3) and len(oview) == 4 * view.n_windows
    wb = oview.orbit_batch(torch.tensor(base, device=ds.device), None)
    _check_windows(recipe, dtype, [wb.x_dict[t] for t in recipe.node_types], wb.y, every)
    oview.check()
    assert oview.segments(torch.tensor([0, view.cum[1], 3 * view.n_windows + view.cum[2]], device=ds.device)).tolist() == [0, 1, 11]


# ---- 2. the K4 model on orbit batches --------------------------------------------------------------------------------------------------------------------
def _dummy(ds, spec):
    xs, _, _ = ds.assemble([0, 1])
    r = ds.recipe
    return types.SimpleNamespace(edge_index_dict=spec.topology.edge_index_dict(2, device=ds.device),
                                 x_dict={t: x[:, :r.width(t)].float().contiguous() for t, x in zip(r.node_types, xs)})


def _com_wrapper(kind, ds, layers, symmetric=True, seed=6):
    """A COM wrapper on the default (split) plan with deterministic `synth` parameters: (wrapper, spec, parameters)."""
    from morphsym_hgnn_amd import synth, wrappers
    torch.set_default_dtype(torch.float32)
    dev = ds.device
    if kind == "mlp":
        torch.manual_seed(seed)
        return wrappers.COM_MLP_Lightning(24 * ds.recipe.history, 128, 6, layers, batch_size=64, stats=STATS).to(dev), None, None
    topo = {"k4": "solo-k4-com", "c2": "solo-c2-com", "s4": "solo-s4-com"}[kind]
    cfg_name = {"k4": "solo-k4", "c2": "solo-c2", "s4": None}[kind] if symmetric else None
    spec = helpers.make_spec(cr.KINDS[kind][0], topo, cfg_name, 128, layers)
    _, cfg = helpers.load_group(cfg_name)
    meta, dummy = spec.topology.metadata(), _dummy(ds, spec)
    if kind == "s4":
        w = wrappers.COM_HGNN_Lightning(128, layers, meta, dummy, stats=STATS)
    else:
        w = wrappers.COM_HGNN_SYM_Lightning(128, layers, meta, dummy, symmetry_mode="MorphSym" if cfg else None, group_operator_path=cfg,
                                            model_type=f"heterogeneous_gnn_{kind}_com", stats=STATS)
    w = w.to(dev)
    params = synth.make_params(seed, spec.param_shapes())
    w.model.load_state_dict(params)
    return w, spec, params


def _oracle_on(batch, recipe, spec, params):
    from oracle import ms_hgnn_oracle as orc
    n = batch.batch_size
    x = {t: batch.x_dict[t][:, :recipe.width(t)].double().cpu() for t in recipe.node_types}
    with torch.no_grad():
        return orc.forward(helpers.oracle_config(spec), params, x, spec.topology.edge_index_dict(n)).reshape(n, -1)


def _max_defect(o, act, B):
    """max over the operators of max |f(g x) - rho(g) f(x)| of fp64 outputs o [K B, row] (a signed permutation: the same maximum as the report's mapped-back form)"""
    return max(float((o[e * B:(e + 1) * B] - o[:B][:, act.perm[e]] * torch.tensor(act.sign[e], dtype=torch.float64)).abs().max()) for e in range(1, act.n_elements))


@pytest.mark.parametrize("layers,B", [(2, 64), (3, 5), (3, 257)])
def test_the_k4_model_on_orbit_batches_is_the_oracles_and_equivariant(layers, B):
    from morphsym_hgnn_amd import symmetrise as sym
    ds, group = _dataset("k4")
    orbit = ds.orbit(group)
    act = sym.OutputAction.from_store(orbit, True)
    assert (act.n_elements, act.row, act.width) == (4, 24, 1)
    view = orbit.view()
    ix = torch.randperm(view.n_windows, generator=torch.Generator().manual_seed(B))[:B].to(ds.device)
    w, spec, params = _com_wrapper("k4", orbit, layers)
    ei = spec.topology.edge_index_dict(4 * B, device=ds.device)
    batch = view.orbit_batch(ix, ei)
    with torch.no_grad():
        y, pred = w.step_helper_function(batch)
    assert pred.shape == (4 * B, 24) and torch.equal(y, batch.y.reshape(4 * B, 24))
    want = _oracle_on(batch, ds.recipe, spec, params)
    scale = float(want.abs().max())
    err = float((pred.double().cpu() - want).abs().max())
    assert _max_defect(want, act, B) == 0.0          # the oracle: exactly equivariant on the zero base series
    d = sym.EquivarianceDefect(act)
    d.update(pred, B)
    rep = d.report()
    worst = max(r["max_abs"] for r in rep.values())
    print(f"K4 L{layers} B{B}: output error {err / scale:.3e}, defect {worst / scale:.3e} of max|out| = {scale:.3e}")
    assert err <= TOL * scale
    assert worst <= 2 * TOL * scale          # both sides of a difference are within TOL of an exactly equivariant function
    # the same parameters without the architecture's symmetry: the defect is at least half the oracle's own on these windows
    w0, spec0, _ = _com_wrapper("k4", orbit, layers, symmetric=False)
    with torch.no_grad():
        _, pred0 = w0.step_helper_function(view.orbit_batch(ix, ei))
    own = _max_defect(_oracle_on(batch, ds.recipe, spec0, params), act, B)
    d0 = sym.EquivarianceDefect(act)
    d0.update(pred0, B)
    got0 = max(r["max_abs"] for r in d0.report().values())
    print(f"   symmetry_mode=None: defect {got0:.3e}, the oracle's own {own:.3e}")
    assert own > 0.1 * scale and got0 >= 0.5 * own
    view.check()


# ---- 3. evaluate_table -----------------------------------------------------------------------------------------------------------------------------------
def _epoch(w):
    return {k: float(getattr(w, k)) for k in ("mse_loss", "mse_loss_lin", "mse_loss_ang", "cos_sim_lin", "cos_sim_ang")}


@pytest.mark.parametrize("kind,batch", [("k4", 64), ("mlp", 257)])
def test_evaluate_table_over_an_orbit_view(kind, batch, tmp_path):
    from morphsym_hgnn_amd import wrappers
    ds, group = _dataset(kind)
    orbit = ds.orbit(group)
    w, spec, _ = _com_wrapper(kind, orbit, 2)
    nb = w.model.num_bases
    ei1 = spec.topology.edge_index_dict(1, device=ds.device) if spec is not None else {}
    view = orbit.view()
    n, K, S = view.n_windows, 4, 3
    assert n == sum(ROWS) and view.names == NAMES
    want = wrappers.evaluate_sequence(w, view, ei1, batch).clone()
    epoch = _epoch(w)
    res = wrappers.evaluate_table(w, view, ei1, batch)
    assert torch.equal(res.predictions, want) and _epoch(w) == epoch          # the sweep of evaluate_sequence, the wrapper's own epoch metrics as it leaves them
    assert res.com and res.operators == ["None", "gs", "gt", "gr"] and res.names == NAMES and res.metrics.overflow() == 0
    assert set(res.table) == {"MSE", "MSE_lin", "MSE_ang", "cos_sim_lin", "cos_sim_ang", "avg_cos_sim", "n"}
    assert all(v.shape == (K, S) and v.dtype == torch.float64 for v in res.table.values())
    assert res.table["n"].tolist() == [[float(r) for r in ROWS]] * K and res.totals["n"].tolist() == [float(n)] * K          # n is exact
    # the whole table is the epoch the wrapper saw
    st = res.metrics.state[:K * S].sum(0)
    assert abs(float((st[0] + st[1]) / (st[2] + st[3])) - epoch["mse_loss"]) <= 1e-12 * epoch["mse_loss"]
    # every operator's row against evaluate_sequence over the corresponding transformed dataset: the same predictions, the sums within the bounds
    u = mr.U
    for e, op in enumerate((None,) + OPS):
        dse = ds if op is None else ds.transformed(op, group)
        p_e = wrappers.evaluate_sequence(w, dse, ei1, batch)
        assert torch.equal(p_e, res.predictions[e * n:(e + 1) * n]), op
        ep = _epoch(w)
        y_e = dse.assemble(view.starts(torch.arange(n)) & ((1 << 56) - 1))[1]
        wb = mr.com_window_bound(p_e.cpu().numpy(), y_e.cpu().numpy(), nb, *STATS)
        _, cos = M.com_window_terms(y_e, p_e, nb, *STATS)
        m = 6 * nb * n
        tot = {k: float(v[e]) for k, v in res.totals.items()}
        assert abs(tot["MSE"] - ep["mse_loss"]) <= 2 * mr.gamma(m + 8) * ep["mse_loss"], op
        assert abs(tot["MSE_lin"] - ep["mse_loss_lin"]) <= 2 * mr.gamma(m + 8) * ep["mse_loss_lin"], op
        assert abs(tot["MSE_ang"] - ep["mse_loss_ang"]) <= 2 * mr.gamma(m + 8) * ep["mse_loss_ang"], op
        for h, name in enumerate(("cos_sim_lin", "cos_sim_ang")):
            bound = (2.0 * wb[:, h].sum() + 2 * mr.gamma(n + 8) * np.abs(cos[:, h]).sum()) / n + 4 * u * abs(ep[name])
            assert abs(tot[name] - ep[name]) <= bound, (op, name, tot[name], ep[name], bound)
        if op is None:          # the identity row is the plain dataset's epoch
            assert abs(tot["MSE"] - ep["mse_loss"]) <= 1e-12 * ep["mse_loss"]
    # per sequence: the table's entry is the mirror's on the sweep's own predictions and the store's labels
    seg = view.segments(np.arange(K * n)).cpu().numpy()
    y_all = torch.cat([(ds if op is None else ds.transformed(op, group)).assemble(view.starts(torch.arange(n)) & ((1 << 56) - 1))[1].clone() for op in (None,) + OPS])
    mirror = M.com_table_from_state(torch.from_numpy(M.com_segmented_reference(y_all, res.predictions, seg, K * S, nb, *STATS)[:K * S]))
    assert torch.equal(mirror["n"].view(K, S), res.table["n"].cpu())
    assert float((mirror["MSE"].view(K, S) - res.table["MSE"].cpu()).abs().max()) <= 1e-12 * float(mirror["MSE"].max())
    assert float((mirror["cos_sim_ang"].view(K, S) - res.table["cos_sim_ang"].cpu()).abs().max()) <= 1e-12
    # the CSV is the reference evaluator's
    buf = io.StringIO()
    res.to_csv(buf)
    lines = buf.getvalue().splitlines()
    assert lines[0] == "Symmetry Operator,Test Loss,Test Cos Sim Lin,Test Cos Sim Ang" and [l.split(",")[0] for l in lines[1:]] == res.operators
    assert [float(v) for v in lines[2].split(",")[1:]] == [float(res.totals[k][1]) for k in ("MSE", "cos_sim_lin", "cos_sim_ang")]
    path = tmp_path / "com.csv"
    res.to_csv(str(path))
    assert open(path).read() == buf.getvalue()
    # K = 1 on the plain dataset: one row, the identity's
    res1 = wrappers.evaluate_table(w, ds, ei1, batch, stride=3)
    assert res1.operators == ["None"] and res1.table["MSE"].shape == (1, S) and float(res1.totals["n"][0]) == len(range(0, n, 3))
    assert abs(float(res1.totals["MSE"][0]) - float(w.mse_loss)) <= 1e-12 * float(w.mse_loss)


def test_evaluate_table_keeps_its_refusal_for_anything_but_a_view():
    from morphsym_hgnn_amd import wrappers
    ds, _ = _dataset("mlp")
    w, _, _ = _com_wrapper("mlp", ds, 2)
    for bad in (None, object(), [ds]):
        with pytest.raises(ValueError, match="COM"):
            wrappers.evaluate_table(w, bad, {}, 8)


# ---- 4. Symmetrised baselines ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,B", [("mlp", 64), ("s4", 5), ("mlp", 257)])
def test_symmetrised_com_baselines(kind, B):
    """Symmetrised(COM_MLP_Lightning) / Symmetrised(COM_HGNN_Lightning) on an orbit-complete batch: the averaged prediction is the mirror's fp32 average of the raw
    predictions bit for bit; loss and the WHOLE flat gradient `torch.equal` the two-call composition engine forward -> the mirror's average -> the wrappers'
    device loss -> the mirror's backward -> engine backward (the tolerance of tests/test_symmetrised_gpu.py for the GRF wrappers: none)."""
    from morphsym_hgnn_amd import symmetrise as sym
    from morphsym_hgnn_amd.metrics import StepMetrics
    ds, group = _dataset(kind)
    orbit = ds.orbit(group)
    act = sym.OutputAction.from_store(orbit, True)
    K, dev = 4, ds.device
    assert (act.n_elements, act.row, act.width) == (K, 6, 1) and all(p == list(range(6)) for p in act.perm)
    w, spec, _ = _com_wrapper(kind, orbit, 2)
    ei = spec.topology.edge_index_dict(K * B, device=dev) if spec is not None else None
    s = sym.Symmetrised(w, act)
    assert s.raw is w and s.model is w.model and s.fused_training_step is False and s.output_action is act
    view = orbit.view()
    ix = torch.randperm(view.n_windows, generator=torch.Generator().manual_seed(B))[:B].to(dev)
    with torch.no_grad():
        y_raw, p_raw = w.step_helper_function(view.orbit_batch(ix, ei))
        y_sym, p_sym = s.step_helper_function(view.orbit_batch(ix, ei))
    avg = orb.average(p_raw.reshape(K * B, 6).cpu().numpy(), act.perm, act.sign, act.width, B)
    assert p_sym.shape == (B, 6) and torch.equal(p_sym.cpu(), torch.from_numpy(avg).view(B, 6)) and torch.equal(y_sym, y_raw[:B])
    assert not torch.equal(p_sym, p_raw[:B])          # a baseline is not equivariant: the average differs from the raw prediction

    wb = view.orbit_batch(ix, ei)
    w.model.zero_grad()
    loss = s.training_step(wb, 0)
    assert w.model._gpend_id == 0 and loss is s.loss and w.loss is None          # the two-call route; the view keeps its own metric state
    assert float(s.cos_sim_lin) == float(s.cos_sim_lin) and abs(float(s.cos_sim_lin)) <= 1.0 + 1e-12          # through ComStepMetrics as any batch
    loss.backward()
    torch.cuda.synchronize()
    got_loss, got_flat = loss.detach().clone(), w.model._gflat.clone()
    assert bool(got_flat.any()) and bool(torch.isfinite(got_flat).all())
    m = w.model
    pdev = next(m.parameters()).device
    e, flat = m._engine(pdev), m._flat_params(pdev)
    if kind == "mlp":
        x = e.cast_input(wb.x_dict["mlp"][:, :m.in_channels].detach())
        out = e.forward(x, flat, training=True)
    else:
        x = e.cast_inputs(wb.x_dict)
        out = e.forward(x, flat, K * B, training=True)
    o = out.reshape(K * B, act.row).cpu().numpy()
    avg_t = torch.from_numpy(orb.average(o, act.perm, act.sign, act.width, B)).to(dev).requires_grad_()
    sm = StepMetrics(regression=True)
    sm.calculate_losses_step(wb.y[:B].reshape(B, -1), avg_t)
    (g,) = torch.autograd.grad(sm.mse_loss, avg_t)
    go = torch.from_numpy(orb.average_backward(g.cpu().numpy(), act.perm, act.sign, act.width, B)).to(dev).reshape(out.shape).contiguous()
    want_flat = e.backward(x, flat, go) if kind == "mlp" else e.backward(x, flat, go, K * B)
    torch.cuda.synchronize()
    assert torch.equal(got_loss, sm.mse_loss.detach()) and torch.equal(got_flat, want_flat)

    # the sweep: the same predictions through the raw wrapper and through its view
    ei1 = spec.topology.edge_index_dict(1, device=dev) if spec is not None else {}
    p1, r1 = sym.evaluate_sequence_symmetrised(w, orbit, ei1, B, stride=2)
    p2, r2 = sym.evaluate_sequence_symmetrised(s, view, ei1, B, stride=2)
    assert p1.shape == (len(range(0, view.n_windows, 2)), 6) and torch.equal(p1, p2) and r1 == r2 and r1["gs"]["max_abs"] > 0


def test_symmetrised_keeps_refusing_an_action_of_another_row():
    from morphsym_hgnn_amd import symmetrise as sym
    ds, group = _dataset("mlp")
    w, _, _ = _com_wrapper("mlp", ds, 2)
    k4 = sym.OutputAction.from_recipes(_recipe("k4").orbit(group), True)          # 24 units: the K4 model's row, not the MLP's 6
    with pytest.raises(ValueError, match="COM"):
        sym.Symmetrised(w, k4)
    with pytest.raises(ValueError, match="COM"):
        sym.Symmetrised(w, sym.OutputAction.from_tables([[0, 1, 2], [1, 0, 2]], [[1] * 3] * 2, 2))
    assert sym.Symmetrised(w, sym.OutputAction.from_store(ds.orbit(group), True)).output_action.row == 6
