"""Group-transformed windows on the device: a `transformed` sibling store over the same resident series, through `assemble` (both gather kernels, both
dtypes) against the reference's vectors (tests/golden/windows_symmetry.npz) and against permuting and negating the plain store's windows in torch; through
the fused evaluation and training routes against assemble-then-call on the same sibling store, bit for bit; the sharing of the series; the refusals."""
import numpy as np
import pytest
import torch

from tests import helpers
from tests import test_window_symmetry as ws
from tests import test_series_eval_gpu as se
from tests import test_series_train_std_gpu as ts
from tests import test_windows as tw

pytestmark = pytest.mark.gpu
T = ws.T
OPS = ws.OPS


def _group(name):
    return ws.A1 if name.startswith("a1") else ws.K4


def _torch_transform(recipe0, recipe1, xs0, y0):
    """g . (assembled windows): the runs of `recipe1` picked out of the plain store's windows by (series, column) and negated, in torch; labels likewise
    (unrotated recipes: a label is a column of the label series)."""
    Tn, out = recipe0.history, []
    for ti, t in enumerate(recipe0.node_types):
        x0, n = xs0[ti], recipe0.num_nodes[t]
        x1 = torch.zeros_like(x0)
        if not recipe0.variables.get(t):
            x1[:, 0] = 1
            out.append(x1)
            continue
        where = {}
        for node in range(n):
            f = 0
            for s, cols in recipe0.variables[t]:
                for c in cols[node]:
                    where.setdefault((s, c), (node, f)); f += Tn
        v0, v1 = x0.view(-1, n, x0.shape[1]), x1.view(-1, n, x0.shape[1])
        for node in range(n):
            f = 0
            for vi, (s, cols) in enumerate(recipe1.variables[t]):
                for ai, c in enumerate(cols[node]):
                    n0, f0 = where[(s, c)]
                    run = v0[:, n0, f0:f0 + Tn]
                    v1[:, node, f:f + Tn] = -run if recipe1.variable_signs[t][vi][node][ai] < 0 else run
                    f += Tn
        out.append(x1)
    pos = {c: k for k, c in enumerate(recipe0.label_cols)}
    y1 = torch.stack([y0[:, pos[c]] * sg for c, sg in zip(recipe1.label_cols, recipe1.label_signs)], 1)
    return out, y1


@pytest.mark.parametrize("fast", [True, False], ids=["chunk-gather", "run-gather"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", ws.CASES, ids=[c["name"] for c in ws.CASES])
def test_a1_assembly_of_the_sibling_matches_the_reference(case, dtype, fast):
    """The tolerances are those tests/test_windows.py applies to the untransformed fixture: none for raw values, one fp32 (bf16: one bf16) rounding for standardised ones."""
    from morphsym_hgnn_amd.windows import SequenceStore, quadsdk_a1_c2_recipe
    parent = SequenceStore(ws.SEQ, quadsdk_a1_c2_recipe(ws.JP, ws.FP, T, 3 if case["body"] else case["grf"], case["body"], case["norm"]), dtype=dtype, fast=fast)
    for op in OPS:
        for mode in ws.MODES:
            store = parent.transformed(op, ws.A1, mode)
            xs, y, q = store.assemble(ws.STARTS)
            for b, st in enumerate(ws.STARTS):
                key = f"a1:{case['name']}:{op}:{mode}:{st}"
                host_x, host_y = ws.evaluate(store.recipe, ws.SEQ, st)
                for ti, (name, n, stride) in enumerate((("base", 2, 7), ("joint", 12, 11))):
                    got = xs[ti][b * n:(b + 1) * n].float().cpu().numpy().astype(np.float64)
                    F = host_x[name].shape[1]
                    assert not got[:, F:].any()
                    for ref, g in ((ws.FX[f"{key}:{name}"], got[:, :F][:, ::stride]), (host_x[name], got[:, :F])):
                        if dtype == "f32":
                            assert np.abs(g - ref).max() <= (0.0 if not case["norm"] else 2e-7 * np.abs(ref).max()), (key, name)
                        else:
                            want_bf = torch.from_numpy(np.ascontiguousarray(ref)).to(torch.bfloat16).double().numpy()
                            assert np.abs(g - want_bf).max() <= (0.0 if not case["norm"] else 2.0 ** -7 * np.abs(ref).max()), (key, name)
                assert torch.equal(xs[2][b * 4:(b + 1) * 4, :1].float().cpu(), torch.ones(4, 1))
                for ref in (ws.FX[key + ":y"], host_y):
                    assert np.abs(y[b].cpu().numpy() - ref).max() <= (1e-6 * np.abs(ref).max() if case["body"] else 0.0), key
                assert np.array_equal(q[b].cpu().numpy().astype(np.float64), np.asarray(ws.SEQ["r_o"])[st + T - 1])      # not transformed


@pytest.mark.parametrize("fast", [True, False], ids=["chunk-gather", "run-gather"])
@pytest.mark.parametrize("mode", ws.MODES)
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("normalize", [False, True], ids=["plain", "norm"])
def test_k4_assembly_of_the_sibling_matches_the_reference(normalize, dtype, mode, fast):
    """As the A1 test: against the reference's vectors and against the host evaluator of the recipe, both gather kernels, both modes."""
    from morphsym_hgnn_amd.windows import SequenceStore, minicheetah_k4_recipe
    parent = SequenceStore(ws.SEQ4, minicheetah_k4_recipe(ws.JP, ws.FP, T, normalize), dtype=dtype, fast=fast)
    for op in OPS:
        store = parent.transformed(op, ws.K4, mode)
        xs, y, q = store.assemble(ws.STARTS)
        for b, st in enumerate(ws.STARTS):
            key = f"k4:{'norm' if normalize else 'plain'}:{op}:{mode}:{st}"
            host_x, host_y = ws.evaluate(store.recipe, ws.SEQ4, st)
            assert np.array_equal(y[b].cpu().numpy(), ws.FX[key + ":y"]) and np.array_equal(y[b].cpu().numpy(), host_y)
            for ti, (name, n, stride) in enumerate((("base", 4, 7), ("joint", 12, 11), ("foot", 4, 13))):
                full = xs[ti][b * n:(b + 1) * n].float().cpu().numpy().astype(np.float64)
                F = store.recipe.width(name)
                assert not full[:, F:].any()
                for ref, got in ((ws.FX[f"{key}:{name}"], full[:, :F][:, ::stride]), (host_x[name], full[:, :F])):
                    if dtype == "f32":
                        assert np.abs(got - ref).max() <= (0.0 if not normalize else 2e-7 * np.abs(ref).max()), (key, name)
                    else:
                        want_bf = torch.from_numpy(np.ascontiguousarray(ref)).to(torch.bfloat16).double().numpy()
                        assert np.abs(got - want_bf).max() <= (0.0 if not normalize else 2.0 ** -7 * np.abs(ref).max()), (key, name)


@pytest.mark.parametrize("fast", [True, False], ids=["chunk-gather", "run-gather"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("normalize", [False, True], ids=["plain", "norm"])
@pytest.mark.parametrize("history,B", [(150, 17), (8, 257), (9, 3), (2, 17), (5, 3)])
def test_assembly_commutes_with_the_transform(history, B, normalize, dtype, fast):
    """Fixture-free: assembling g . window equals permuting and negating, in torch, what the plain store assembles -- bit for bit (-0 == 0), standardised
    windows included (the sign is an XOR, the statistics of a negated run are the negated statistics).  Histories that put a chunk's split point
    everywhere (9, 5, 2: several runs per 16-byte chunk on the general route), a whole chunk per run (8) and the datasets' 150."""
    from morphsym_hgnn_amd.windows import SequenceStore, minicheetah_k4_recipe
    parent = SequenceStore(ws.SEQ4, minicheetah_k4_recipe(ws.JP, ws.FP, history, normalize), dtype=dtype, fast=fast)
    n = len(parent)
    starts = torch.randint(0, n, (B,), generator=torch.Generator().manual_seed(history * 1000 + B))
    starts[0], starts[-1] = 0, n - 1
    xs0, y0, _ = parent.assemble(starts)
    for op in OPS:
        store = parent.transformed(op, ws.K4)
        xs1, y1, _ = store.assemble(starts)
        want_x, want_y = _torch_transform(parent.recipe, store.recipe, xs0, y0)
        for a, b in zip(xs1, want_x):
            assert torch.equal(a, b)
        assert torch.equal(y1, want_y)
        assert not torch.equal(xs1[1], xs0[1])


def test_siblings_share_the_series():
    from morphsym_hgnn_amd.windows import SequenceStore, ResidentDataset, minicheetah_k4_recipe
    seqs = [{k: np.asarray(v)[lo:hi] for k, v in ws.SEQ4.items()} for lo, hi in ((0, 160), (160, 330), (330, 400))]
    ds = ResidentDataset(seqs, minicheetah_k4_recipe(ws.JP, ws.FP, 50), dtype="bf16")      # (the shortest of the three sequences has 70 rows)
    ds.series_step_args(bf16=True)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    sibs = [ds.transformed(op, ws.K4) for op in OPS] + [ds.transformed("gs", ws.K4, "Euclidean")]
    series_bytes = sum(a.numel() * a.element_size() for a in ds.series)
    assert torch.cuda.memory_allocated() - before < series_bytes // 4      # tables only: no series memory
    for k, sib in enumerate(sibs):
        assert [a.data_ptr() for a in sib.series] == [a.data_ptr() for a in ds.series]
        assert [a.data_ptr() for a in sib.series16] == [a.data_ptr() for a in ds.series16] and len(sib.series16) == len(ds.series)
        assert sib.runs.data_ptr() != ds.runs.data_ptr() and sib.label_cols.data_ptr() != ds.label_cols.data_ptr()
        assert sib.seq_rows == ds.seq_rows and len(sib) == len(ds) and ds.desc.sign_flags == 0
        assert sib.desc.sign_flags == (1 if k < 3 else 0)      # (mode "Euclidean" permutes only: an unsigned descriptor, the code unsigned recipes always ran)
        tr, va = sib.split()
        tr0, va0 = ds.split()
        assert tr.ranges == tr0.ranges and va.ranges == va0.ranges and tr.dataset is sib
        ix = next(iter(sib.view().epoch(7, generator=torch.Generator().manual_seed(3))))
        assert torch.equal(sib.view().starts(ix), ds.view().starts(ix))
    late = SequenceStore(ws.SEQ4, minicheetah_k4_recipe(ws.JP, ws.FP, T), dtype="bf16")      # a sibling made BEFORE the bf16 copies exist shares them too
    sib = late.transformed("gt", ws.K4)
    sib.series_step_args(bf16=True)
    assert late.series16 and [a.data_ptr() for a in late.series16] == [a.data_ptr() for a in sib.series16]


def test_bad_sign_tables_are_refused_before_anything_is_written():
    from morphsym_hgnn_amd import engine as eng
    from morphsym_hgnn_amd.windows import SequenceStore, quadsdk_a1_c2_recipe
    FLAG = SequenceStore.SIGN_FLAG
    for what in ("constant run", "label column"):
        store = SequenceStore(ws.SEQ, quadsdk_a1_c2_recipe(ws.JP, ws.FP, T), dtype="f32").transformed("gs", ws.A1)
        if what == "constant run":
            r = int((store.runs[:, 3] == -1).nonzero()[0, 0])
            store.runs[r, 3] = -1 - FLAG      # "minus the constant one": a negative word that is not -1
        else:
            store.label_cols[1] = FLAG | 300
        xs, y, q = store._buffers(3)
        for t in xs + [y, q]:
            t.fill_(7.0)
        with pytest.raises(eng.MshgnnError) as ei:
            store.assemble([0, 1, 2], reuse_buffers=True)
        torch.cuda.synchronize()
        assert ("cannot carry a sign" if what == "constant run" else "column part out of range") in str(ei.value)
        assert all(bool((t == 7.0).all()) for t in xs + [y, q])
        assert store.desc.sign_flags == 1      # never vouched for


def _sibling_setup(name, plan, op, normalize=False):
    recipe, spec, seq, n, store, e, flat = se._setup(name, plan, normalize=normalize, constant=normalize)
    return spec, n, store.transformed(op, _group(name)), store, e, flat


@pytest.mark.parametrize("plan", ["bf16", "x3"])
@pytest.mark.parametrize("normalize", [False, True], ids=["plain", "norm"])
@pytest.mark.parametrize("name,B,op", [("a1c2_L3", 17, "gs"), ("a1c2_L3", 257, "gr"), ("a1c2_L2", 3, "gt"), ("mck4_cls", 257, "gs"), ("mck4_cls", 17, "gr")])
def test_forward_series_on_the_sibling_is_bit_identical_to_assemble_then_forward(name, B, op, normalize, plan):
    spec, n, sib, parent, e, flat = _sibling_setup(name, plan, op, normalize)
    if name == "a1c2_L3" and plan == "bf16":
        assert e.specialised == "A1C2_L3"      # the compile-time stack program; a1c2_L2: interpreted
    starts = se._starts(n, B, force=(se.CONST_START,) if normalize else ())
    _, y_a, q_a, out_a = se._yardstick(sib, e, flat, starts)
    out_p = se._yardstick(parent, e, flat, starts)[3]
    y, q, li, out = e.forward_series(sib, starts, flat)
    torch.cuda.synchronize()
    assert torch.equal(out, out_a) and torch.equal(y, y_a) and not torch.equal(out_a, out_p)
    if sib.recipe.quat_series:
        assert torch.equal(q, q_a)
    if not spec.regression:
        assert torch.equal(li, (y_a != 0).to(torch.int32).reshape(B, 4))
    assert sib.desc.sign_flags == 3
    out2 = e.forward_series(sib, starts, flat)[3]      # vouched tables and run pointers: the same bits
    torch.cuda.synchronize()
    assert torch.equal(out2, out_a)


@pytest.mark.parametrize("plan", ["bf16", "x3"])
@pytest.mark.parametrize("name,B,op", [("a1c2", 17, "gs"), ("a1c2_body", 257, "gr"), ("mck4_cls", 3, "gt"), ("mck4_cls", 257, "gs")])
def test_standardised_series_step_on_the_sibling(name, B, op, plan):
    recipe, spec, n, store, e, flat = ts._setup(name, plan)
    sib = store.transformed(op, _group(name))
    starts = se._starts(n, B, force=(se.CONST_START,))
    want = ts._yardstick(sib, e, spec, flat, starts)
    ts._poison(sib, B)
    got = (e.step_mse_series_std if spec.regression else e.step_ce_series_std)(sib, starts, flat)
    ts._check_step(sib, e, spec, starts, want, got)      # windows written out, labels / flags / quaternion, output, loss, the whole flat gradient
    assert not torch.equal(want[0][1], ts._yardstick(store, e, spec, flat, starts)[0][1])


# (the split plan's weight-gradient kernel reads materialised windows: x_out == NULL is a bf16-plan route)
@pytest.mark.parametrize("plan,materialize", [("bf16", True), ("bf16", False), ("x3", True)], ids=["bf16-x_out", "bf16-no-x_out", "x3-x_out"])
@pytest.mark.parametrize("name,B,op", [("a1c2", 17, "gs"), ("a1c2_body", 257, "gr"), ("mck4_cls", 3, "gt"), ("mck4_cls", 257, "gs")])
def test_series_step_on_the_sibling(name, B, op, plan, materialize):
    recipe, spec, n, store, e, flat = ts._setup(name, plan, normalize=False)
    sib = store.transformed(op, _group(name))
    starts = se._starts(n, B)
    want = ts._yardstick(sib, e, spec, flat, starts)
    ts._poison(sib, B)
    xs, second, out, loss, g = (e.step_mse_series if spec.regression else e.step_ce_series)(sib, starts, flat, materialize=materialize)
    torch.cuda.synchronize()
    if materialize:
        ts._check_step(sib, e, spec, starts, want, (xs, second, out, loss, g))
    else:
        assert xs is None and torch.equal(out, want[4]) and torch.equal(loss, want[5]) and torch.equal(g, want[6])
        assert torch.equal(sib._buffers(B)[1], want[1])
    g_parent = ts._yardstick(store, e, spec, flat, starts)[6]
    assert not torch.equal(g_parent, want[6])


# --- the wrappers, a dataset of three sequences, a captured step ---------------------------------------------------------------------------------

from tests import test_dataset_gpu as td      # noqa: E402


def _sibling_dataset(kind, normalize, plan, op):
    """A ResidentDataset of three sequences and its transformed sibling (the K4 wrappers are fixed at the reference's 150 steps)."""
    from morphsym_hgnn_amd.windows import ResidentDataset, minicheetah_k4_recipe
    from oracle.gen_window_golden import minicheetah_sequence
    if kind == "a1c2":
        ds = td._dataset("a1c2", normalize, plan)
    else:
        ds = ResidentDataset([minicheetah_sequence(7100 + 13 * s, n) for s, n in enumerate((150, 151, 207))], minicheetah_k4_recipe(ws.JP, ws.FP, T, normalize), dtype=plan)
    return ds, ds.transformed(op, _group(kind))


@pytest.mark.parametrize("kind,plan,op,normalize", [("a1c2", "bf16", "gs", False), ("a1c2", "x3", "gr", True), ("mck4", "bf16", "gt", True), ("mck4", "x3", "gs", False)])
def test_wrapper_steps_on_a_window_batch_of_the_sibling(kind, plan, op, normalize, monkeypatch):
    """training_step and validation_step of HGNN_C2_Lightning_Reg / HGNN_K4_Lightning on `sibling.view().batch(device indices)` -- the fused series routes,
    nothing assembled -- against the same steps on the sibling's assembled batch: loss and the whole flat gradient; not the parent's."""
    import types
    ds, sib = _sibling_dataset(kind, normalize, plan, op)
    w, spec, dev = td._wrapper(kind, plan, sib)
    view, B = sib.view(), 17
    ix = td._mixed_indices(view, B)
    ei = spec.topology.edge_index_dict(B, device=dev)
    rows = td._mirror(view, ix).tolist()
    xs, y, _ = sib.assemble(rows)
    plain = types.SimpleNamespace(x_dict={t: x.clone() for t, x in zip(sib.recipe.node_types, xs)}, edge_index_dict=ei, y=y.clone(), batch_size=B)
    xs_p, y_p, _ = ds.assemble(rows)
    parent = types.SimpleNamespace(x_dict={t: x.clone() for t, x in zip(ds.recipe.node_types, xs_p)}, edge_index_dict=ei, y=y_p.clone(), batch_size=B)

    def run(batch):
        w.model.zero_grad()
        loss = w.training_step(batch, 0)
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach().clone(), w.model._gflat.clone()

    loss_a, flat_a = run(plain)
    loss_p, flat_p = run(parent)
    assert bool(flat_a.any()) and bool(torch.isfinite(flat_a).all()) and not torch.equal(flat_a, flat_p)
    with torch.no_grad():
        val_a = w.validation_step(plain, 0).detach().clone()
    wb = view.batch(ix.cuda(), ei)
    assert wb.store is sib
    with monkeypatch.context() as m:
        m.setattr(sib, "assemble", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the fused route assembles nothing")))
        loss_b, flat_b = run(wb)
        with torch.no_grad():
            val_b = w.validation_step(view.batch(ix.cuda(), ei), 0).detach().clone()
    assert torch.equal(wb.y, y)
    assert torch.equal(loss_b, loss_a) and torch.equal(flat_b, flat_a) and torch.equal(val_b, val_a)
    view.check()


@pytest.mark.parametrize("normalize,plan,op", [(False, "bf16", "gr"), (True, "x3", "gs"), (True, "bf16", "gt")])
def test_evaluate_sequence_over_a_view_of_the_sibling_dataset(normalize, plan, op):
    from morphsym_hgnn_amd import wrappers
    from morphsym_hgnn_amd.windows import SequenceStore
    ds, sib = _sibling_dataset("a1c2", normalize, plan, op)
    w, spec, dev = td._wrapper("a1c2", plan, sib)
    ei1 = spec.topology.edge_index_dict(1, device=dev)
    per_seq = [wrappers.evaluate_sequence(w, SequenceStore(seq, ds.recipe, dtype=plan).transformed(op, ws.A1), ei1, 64).clone() for seq in td._sequences("a1c2")]
    assert [p.shape[0] for p in per_seq] == sib.seq_windows
    train, val = sib.split()
    for view in (val, train, sib):
        ranges = view.ranges if view is not sib else [(0, n) for n in sib.seq_windows]
        want = torch.cat([p[lo:hi] for p, (lo, hi) in zip(per_seq, ranges)])
        assert torch.equal(wrappers.evaluate_sequence(w, view, ei1, 17), want)
    assert not torch.equal(wrappers.evaluate_sequence(w, ds, ei1, 64), torch.cat(per_seq))


def test_graphed_training_step_replays_new_indices_on_the_sibling():
    """GraphedTrainingStep(index_source=a view of the sibling): mapping + signed series step + Adam captured once (the sign tables were checked by the eager
    warm-up and are vouched for inside the capture); two replays on new indices == the eager steps of a twin."""
    from morphsym_hgnn_amd import wrappers
    B, twins = 17, []
    for _ in range(2):
        ds, sib = _sibling_dataset("a1c2", False, "bf16", "gs")
        w, spec, dev = td._wrapper("a1c2", "bf16", sib)
        w.lr = 1e-3
        w.graph_safe_optimizer = True
        twins.append((w, w.configure_optimizers(), sib.split()[0]))
    (a, oa, va), (b, ob, vb) = twins
    ei = spec.topology.edge_index_dict(B, device=dev)
    batches = [td._mixed_indices(va, B, seed=k).cuda() for k in range(3)]
    gs = wrappers.GraphedTrainingStep(a, oa, va.batch(batches[0], ei), index_source=va)
    assert va.dataset.desc.sign_flags == 3
    for k, ix in enumerate(batches[1:]):
        loss_a = gs(ix)
        ob.zero_grad(set_to_none=True)
        loss_b = b.training_step(vb.batch(ix, ei), 0); loss_b.backward(); ob.step()
        torch.cuda.synchronize()
        assert torch.equal(loss_a.detach().reshape(-1), loss_b.detach().reshape(-1)), k
        for p, q in zip(a.model.parameters(), b.model.parameters()):
            assert torch.equal(p.detach(), q.detach()), k
    va.check()


# --- equivariance end to end, on rounding-free data --------------------------------------------------------------------------------------------------

def _exact_series(kind, seed, N=160):
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.integers(-1, 2, size=s).astype(np.float64)
    if kind == "a1c2":
        return {"imu_acc": f(N, 3), "imu_omega": f(N, 3), "q": f(N, 12), "qd": f(N, 12), "tau": f(N, 12), "F": f(N, 12), "r_o": f(N, 4) + 3}
    return {"imu_acc": f(N, 3), "imu_omega": f(N, 3), "q": f(N, 12), "qd": f(N, 12), "p": f(N, 12), "v": f(N, 12), "contacts": rng.integers(0, 2, size=(N, 4)).astype(np.float64)}


@pytest.mark.parametrize("plan", ["bf16", "x3"])
@pytest.mark.parametrize("kind", ["a1c2", "mck4"])
def test_equivariance_end_to_end_on_rounding_free_data(kind, plan):
    """The rounding-free parameters of tests/exact_data.py and series of -1 / 0 / 1: every hidden state of the fp64 oracle is a bf16 value, so the plans
    equal the oracle bit for bit and no tolerance is needed.  `forward_series` on the sibling store == the fp64 oracle on the transformed windows, for the
    three operators; and == g . (the output on x) wherever the model family is equivariant: MiniCheetah-K4 under all three, A1-C2 (a C2 model: one
    non-trivial element) under gs -- under gt and gr the C2 model is not equivariant, in the oracle either (asserted), and the oracle comparison stands alone."""
    from morphsym_hgnn_amd import engine as eng
    from morphsym_hgnn_amd.windows import SequenceStore, quadsdk_a1_c2_recipe, minicheetah_k4_recipe
    from tests import exact_data as xd
    if kind == "a1c2":
        spec, knobs, recipe, n_out = helpers.make_spec("c2", "a1-c2", "a1-c2", 128, 4, True), dict(rel_scales=(1.0,)), quadsdk_a1_c2_recipe(ws.JP, ws.FP, T, 3), 12
    else:
        spec, knobs = helpers.make_spec("k4", "mini_cheetah-k4", "mini_cheetah-k4", 128, 3, False), dict(rel_scales=(1.0,), bias_range=(0, 1))
        recipe, n_out = minicheetah_k4_recipe(ws.JP, ws.FP, T), 8
    group, seed, starts = _group(kind), 3, [0, 3, 10]
    case = xd.exact_case(spec, 1, seed, mse=False, **knobs)
    seq = _exact_series(kind, seed)

    def oracle(r):
        rows = [ws.evaluate(r, seq, st)[0] for st in starts]
        c = dict(case, B=len(starts), x={t: torch.cat([torch.from_numpy(x[t]) for x in rows]).double() for t in r.node_types})
        ref = xd.reference(spec, c)
        assert all(bool(xd.bf16_exact(h)) for h in ref["hidden"])      # rounding-free at every layer
        return ref["out"].reshape(len(starts), n_out)

    def g_of(out, op):
        if kind == "a1c2":
            P, c = group.table("fs", op)
            return out[:, P] * torch.tensor(c, dtype=out.dtype, device=out.device)
        P, _ = group.table("ls", op)
        return out.reshape(-1, 4, 2)[:, P, :].reshape(-1, 8)

    store = SequenceStore(seq, recipe, dtype=plan)
    e = eng.Engine(spec, plan)
    flat = eng.flatten_params(spec, case["params"], e.device)
    st = torch.tensor(starts, dtype=torch.int64).cuda()
    out0 = e.forward_series(store, st, flat, labels=False)[3].double().cpu().reshape(len(starts), n_out).clone()
    o0 = oracle(recipe)
    assert torch.equal(out0, o0) and int((o0 != 0).sum()) > o0.numel() // 2
    for op in OPS:
        sib = store.transformed(op, group)
        out1 = e.forward_series(sib, st, flat, labels=False)[3].double().cpu().reshape(len(starts), n_out).clone()
        o1 = oracle(sib.recipe)
        assert torch.equal(out1, o1), op
        equivariant = kind == "mck4" or op == "gs"
        assert torch.equal(o1, g_of(o0, op)) == equivariant, op
        if equivariant:
            assert torch.equal(out1, g_of(out0, op)) and not torch.equal(out1, out0), op


# --- the fused routes at short histories: a chunk's split point n0 = min(8, T - k0 % T) takes every value ------------------------------------------

def _short_setup(kind, history, normalize, plan):
    """A1-C2 (regression) / MiniCheetah-K4 (contact classification) models whose input widths are those of `history`-step windows (the engine's own
    steps: the wrappers are fixed at the reference's 150), on the sequences of tests/test_windows.py."""
    from morphsym_hgnn_amd import engine as eng, synth, topology
    from morphsym_hgnn_amd.spec import ModelSpec
    from morphsym_hgnn_amd.windows import SequenceStore, quadsdk_a1_c2_recipe, minicheetah_k4_recipe
    if kind == "a1c2":
        r, seq, name = quadsdk_a1_c2_recipe(ws.JP, ws.FP, history, 3, normalize=normalize), ws.SEQ, "a1-c2"
    else:
        r, seq, name = minicheetah_k4_recipe(ws.JP, ws.FP, history, normalize), ws.SEQ4, "mini_cheetah-k4"
    group, _ = helpers.load_group(name)
    spec = ModelSpec(kind="c2" if kind == "a1c2" else "k4", topology=topology.TOPOLOGIES[name](), hidden=128, num_layers=2,
                     widths={t: r.width(t) for t in r.node_types}, regression=kind == "a1c2", grf_dimension=3, group=group, num_timesteps=history)
    store = SequenceStore(seq, r, dtype=plan)
    e = eng.Engine(spec, plan)
    assert not e.generic
    return spec, store, e, eng.flatten_params(spec, synth.make_params(8, spec.param_shapes()), e.device)


@pytest.mark.parametrize("plan", ["bf16", "x3"])
@pytest.mark.parametrize("history", [9, 8])
@pytest.mark.parametrize("kind", ["a1c2", "mck4"])
def test_fused_routes_on_the_sibling_at_short_histories(kind, history, plan):
    """History 9: n0 runs through 1 .. 8, odd values included -- opposite signs in the two bf16 halves of one 32-bit word of the encoders' and the
    weight-gradient fetch's masks (the A1 base rows alternate in sign, the K4 foot rows too).  History 8: a whole chunk per run.  forward_series plain and
    standardised, step_*_series with and (bf16 plan) without x_out, step_*_series_std: windows written out, labels / flags, output, loss and the whole flat
    gradient against assemble-then-call on the same sibling, bit for bit, for the three operators and 17 / 257 windows."""
    for normalize in (False, True):
        spec, parent, e, flat = _short_setup(kind, history, normalize, plan)
        n = len(parent)
        for op, B in zip(OPS, (17, 257, 17)):
            sib = parent.transformed(op, _group(kind))
            starts = torch.randint(0, n, (B,), generator=torch.Generator().manual_seed(B + history))
            starts[0], starts[-1] = 0, n - 1
            starts = starts.cuda()
            # evaluation
            _, y_a, q_a, out_a = se._yardstick(sib, e, flat, starts)
            out_p = se._yardstick(parent, e, flat, starts)[3]
            y, q, li, out = e.forward_series(sib, starts, flat)
            torch.cuda.synchronize()
            assert torch.equal(out, out_a) and torch.equal(y, y_a) and not torch.equal(out_a, out_p), (normalize, op)
            # training
            want = ts._yardstick(sib, e, spec, flat, starts)
            assert bool(want[6].any()) and not torch.equal(want[6], ts._yardstick(parent, e, spec, flat, starts)[6])
            ts._poison(sib, B)
            if normalize:
                got = (e.step_mse_series_std if spec.regression else e.step_ce_series_std)(sib, starts, flat)
                ts._check_step(sib, e, spec, starts, want, got)
            else:
                step = e.step_mse_series if spec.regression else e.step_ce_series
                ts._check_step(sib, e, spec, starts, want, step(sib, starts, flat))
                if plan == "bf16":      # x_out == NULL: the weight-gradient kernel gathers (and negates) its raw operands itself
                    xs, second, out, loss, g = step(sib, starts, flat, materialize=False)
                    torch.cuda.synchronize()
                    assert xs is None and torch.equal(out, want[4]) and torch.equal(loss, want[5]) and torch.equal(g, want[6]), op


@pytest.mark.parametrize("plan", ["bf16", "x3"])
def test_history_2_is_refused_by_the_fused_routes_for_a_sibling_as_for_any_store(plan):
    """Node rows of several runs need history >= 8 on mshgnn_forward_series and the standardised steps (a chunk takes its elements from at most two runs):
    the sibling is refused like its parent, before any launch, and assembles instead (test_assembly_commutes_with_the_transform covers 2 and 5 there)."""
    from morphsym_hgnn_amd import engine as eng
    spec, parent, e, flat = _short_setup("mck4", 2, True, plan)
    sib = parent.transformed("gs", ws.K4)
    starts = torch.tensor([0, 5, len(sib) - 1], dtype=torch.int64).cuda()
    for store in (parent, sib):
        with pytest.raises(eng.MshgnnError, match="history >= 8"):
            e.forward_series(store, starts, flat)
        with pytest.raises(eng.MshgnnError, match="history >= 8"):
            e.step_ce_series_std(store, starts, flat)
    xs, y, _ = sib.assemble(starts)
    assert torch.isfinite(xs[1].float()).all()
