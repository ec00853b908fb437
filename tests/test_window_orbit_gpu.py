"""Orbit batches on the device: a group element per window on every window route.  Everything here is bit for bit (`torch.equal`): row b of an orbit batch
against row b of the sibling store of its element (`store.transformed`), the fused routes against assemble-then-call on the orbit store itself, equivariance
on rounding-free data inside ONE batch, the wrappers over an orbit view, and the refusals of the checking call.
Shapes: 3 windows (several elements inside one tile), 17 (a ragged second tile), 1000 (many workgroups); histories 150, 9 and 8; both plans."""
import types

import numpy as np
import pytest
import torch

from tests import helpers
from tests import test_window_symmetry as ws
from tests import test_window_symmetry_gpu as wsg
from tests import test_series_eval_gpu as se
from tests import test_series_train_std_gpu as ts
from tests import test_dataset_gpu as td

pytestmark = pytest.mark.gpu
T, OPS = ws.T, ws.OPS
K = 1 + len(OPS)
SHIFT = 56
BATCHES = (3, 17, 1000)
PATTERNS = ("random", "identity", "tile", "alternating")


def _elements(pattern, B, seed=0):
    """One group element per window: random with every element present (as far as B allows), all identity, one element per 16-window tile, alternating."""
    if pattern == "identity":
        return torch.zeros(B, dtype=torch.int64)
    if pattern == "tile":
        return (torch.arange(B) // 16 + 1) % K
    if pattern == "alternating":
        return (torch.arange(B) + 1) % K
    el = torch.randint(0, K, (B,), generator=torch.Generator().manual_seed(7 * B + seed))
    k = min(K, B)
    el[:k] = torch.arange(K - k, K).flip(0)      # (B = 3: elements 3, 2, 1 inside one tile)
    return el


def _recipe(robot, history, normalize=False):
    from morphsym_hgnn_amd.windows import quadsdk_a1_c2_recipe, minicheetah_k4_recipe
    if robot == "a1c2":      # regression, rotated 3-D labels with quaternion
        return quadsdk_a1_c2_recipe(ws.JP, ws.FP, history, 3, body_frame_labels=True, normalize=normalize), ws.SEQ, ws.A1
    return minicheetah_k4_recipe(ws.JP, ws.FP, history, normalize), ws.SEQ4, ws.K4


def _starts(n, B, seed=0):
    st = torch.randint(0, n, (B,), generator=torch.Generator().manual_seed(B + 31 * seed))
    st[0], st[-1] = 0, n - 1
    return st


def _pick(per_element, el):
    """rows of the K per-element tensors [B, ...] chosen window by window"""
    return torch.stack(per_element)[el.to(per_element[0].device), torch.arange(el.numel(), device=per_element[0].device)]


# --- 1. assembly, both kernels ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fast", [True, False], ids=["chunk-gather", "run-gather"])
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("history", [150, 9, 8])
@pytest.mark.parametrize("robot,normalize", [("a1c2", False), ("mck4", False), ("mck4", True)], ids=["a1c2", "mck4", "mck4-norm"])
def test_orbit_assembly_rows_are_the_siblings_rows(robot, normalize, history, dtype, fast):
    from morphsym_hgnn_amd.windows import SequenceStore
    recipe, seq, group = _recipe(robot, history, normalize)
    store = SequenceStore(seq, recipe, dtype=dtype, fast=fast)
    orbit = store.orbit(group)
    assert orbit.n_elements == K and len(orbit) == len(store) and orbit.operators == [None, "gs", "gt", "gr"]
    assert [a.data_ptr() for a in orbit.series] == [a.data_ptr() for a in store.series] and orbit.desc.sign_flags == (1 | K << 8)
    sibs = [store] + [store.transformed(op, group) for op in OPS]
    for B in BATCHES:
        starts = _starts(len(store), B, history)
        per = [s.assemble(starts) for s in sibs]
        for pattern in PATTERNS:
            el = _elements(pattern, B, history)
            # host elements / device elements / packed device starts: the same batch
            xs, y, q = orbit.assemble(starts, elements=el.tolist())
            xs_d, y_d, q_d = orbit.assemble(starts.cuda(), elements=el.cuda())
            xs_p, y_p, _ = orbit.assemble(starts.cuda() | (el.cuda() << SHIFT))
            for ti, t in enumerate(recipe.node_types):
                n_t = recipe.num_nodes[t]
                want = _pick([p[0][ti].view(B, n_t, -1) for p in per], el).reshape(B * n_t, -1)
                assert torch.equal(xs[ti], want), (B, pattern, t)
                assert torch.equal(xs_d[ti], want) and torch.equal(xs_p[ti], want)
            want_y = _pick([p[1] for p in per], el)
            assert torch.equal(y, want_y) and torch.equal(y_d, want_y) and torch.equal(y_p, want_y), (B, pattern)
            if recipe.quat_series:
                assert torch.equal(q, per[0][2]) and torch.equal(q_d, per[0][2])      # r_o is untouched, as for siblings
            if pattern == "identity":      # ... equals the plain store's batch
                assert all(torch.equal(a, b) for a, b in zip(xs, per[0][0])) and torch.equal(y, per[0][1])
            elif B > 3:
                assert not torch.equal(xs[1], per[0][0][1])
    assert orbit.desc.sign_flags == (3 | K << 8)      # checked once, vouched for afterwards


@pytest.mark.parametrize("fast", [True, False], ids=["chunk-gather", "run-gather"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_orbit_assembly_matches_the_reference_fixture(dtype, fast):
    """The fixture's windows, read as tests/test_window_symmetry_gpu.py reads them: every operator of every start in ONE orbit batch (raw windows: no tolerance;
    body-frame labels within the 1e-6 the existing test gives the fp64 rotation)."""
    from morphsym_hgnn_amd.windows import SequenceStore, quadsdk_a1_c2_recipe, minicheetah_k4_recipe
    starts = [st for st in ws.STARTS for _ in OPS]
    el = [1 + k for _ in ws.STARTS for k in range(len(OPS))]

    def check(xs, b, key, layout):
        for ti, (name, n, stride) in enumerate(layout):      # (xs: the feature columns only; the fixture keeps every stride-th)
            ref = ws.FX[f"{key}:{name}"]
            got = xs[ti][b * n:(b + 1) * n].float().cpu().numpy().astype(np.float64)[:, ::stride]
            want = ref if dtype == "f32" else torch.from_numpy(np.ascontiguousarray(ref)).to(torch.bfloat16).double().numpy()
            assert np.array_equal(got, want), (key, name)

    for mode in ws.MODES:
        for case in [c for c in ws.CASES if not c["norm"]]:
            recipe = quadsdk_a1_c2_recipe(ws.JP, ws.FP, T, 3 if case["body"] else case["grf"], case["body"], False)
            orbit = SequenceStore(ws.SEQ, recipe, dtype=dtype, fast=fast).orbit(ws.A1, mode=mode)
            xs, y, q = orbit.assemble(starts, elements=el)
            for b, (st, e) in enumerate(zip(starts, el)):
                key = f"a1:{case['name']}:{OPS[e - 1]}:{mode}:{st}"
                check([x[:, :recipe.width(t)] for x, t in zip(xs, recipe.node_types)], b, key, (("base", 2, 7), ("joint", 12, 11)))
                ref = ws.FX[key + ":y"]
                assert np.abs(y[b].cpu().numpy() - ref).max() <= (1e-6 * np.abs(ref).max() if case["body"] else 0.0), key
                assert np.array_equal(q[b].cpu().numpy().astype(np.float64), np.asarray(ws.SEQ["r_o"])[st + T - 1])
        recipe = minicheetah_k4_recipe(ws.JP, ws.FP, T, False)
        orbit = SequenceStore(ws.SEQ4, recipe, dtype=dtype, fast=fast).orbit(ws.K4, mode=mode)
        xs, y, _ = orbit.assemble(starts, elements=el)
        for b, (st, e) in enumerate(zip(starts, el)):
            key = f"k4:plain:{OPS[e - 1]}:{mode}:{st}"
            assert np.array_equal(y[b].cpu().numpy(), ws.FX[key + ":y"])
            check([x[:, :recipe.width(t)] for x, t in zip(xs, recipe.node_types)], b, key, (("base", 4, 7), ("joint", 12, 11), ("foot", 4, 13)))


# --- 2. the fused routes against assemble-then-call on the orbit store -----------------------------------------------------------------------------------

def _packed(store, B, pattern, seed=0, force=()):
    n = len(store)
    st = _starts(n, B, seed)
    for i, s in enumerate(force):
        st[1 + i] = s
    return (st | (_elements(pattern, B, seed) << SHIFT)).cuda()


def _fused_routes(spec, orbit, e, flat, normalize, batches=BATCHES, force=()):
    """forward_series, then the training step of the recipe's kind (materialised windows) -- each against assemble-then-call on the same orbit store, then once
    more on vouched tables and run pointers."""
    for B in batches:
        for pattern in (PATTERNS if B == 17 else ("random",)):
            starts = _packed(orbit, B, pattern, force=force)
            _, y_a, q_a, out_a = se._yardstick(orbit, e, flat, starts)
            for again in range(2):
                y, q, li, out = e.forward_series(orbit, starts, flat)
                torch.cuda.synchronize()
                assert torch.equal(out, out_a) and torch.equal(y, y_a), (B, pattern, again)
                if orbit.recipe.quat_series:
                    assert torch.equal(q, q_a)
                if not spec.regression:
                    assert torch.equal(li, (y_a != 0).to(torch.int32).reshape(B, 4))
            assert orbit.desc.run_ptrs_ready == 1      # (the second call vouched for the run pointers the first resolved)
            want = ts._yardstick(orbit, e, spec, flat, starts)
            assert bool(want[6].any())
            if normalize:
                step = e.step_mse_series_std if spec.regression else e.step_ce_series_std
            else:
                step = e.step_mse_series if spec.regression else e.step_ce_series
            for again in range(2):
                ts._poison(orbit, B)
                ts._check_step(orbit, e, spec, starts, want, step(orbit, starts, flat))      # windows written, labels / flags / quaternion, output, loss, gradient
            if pattern == "random" and B > 3:      # (not the identity's results)
                plain = (starts & ((1 << SHIFT) - 1))
                assert not torch.equal(ts._yardstick(orbit, e, spec, flat, plain)[6], want[6])


@pytest.mark.parametrize("spec_programs", [True, False], ids=["compiled", "interpreted"])
@pytest.mark.parametrize("plan", ["bf16", "x3"])
@pytest.mark.parametrize("name,normalize", [("a1c2_L3", False), ("a1c2_L3", True), ("mck4_cls", False), ("mck4_cls", True)],
                         ids=["a1c2", "a1c2-norm", "mck4", "mck4-norm"])
def test_fused_routes_on_orbit_batches(name, normalize, plan, spec_programs, monkeypatch):
    if not spec_programs:
        monkeypatch.setenv("MSHGNN_SPEC", "0")
    recipe, spec, seq, n, store, e, flat = se._setup(name, plan, normalize=normalize, constant=normalize)
    if name == "a1c2_L3":
        assert e.specialised == (("X3_" if plan == "x3" else "") + "A1C2_L3" if spec_programs else "")      # the compile-time program / the interpreting kernels
    orbit = store.orbit(wsg._group(name))
    _fused_routes(spec, orbit, e, flat, normalize, batches=BATCHES if spec_programs else (17,), force=(se.CONST_START,) if normalize else ())


@pytest.mark.parametrize("plan", ["bf16", "x3"])
@pytest.mark.parametrize("history", [9, 8])
@pytest.mark.parametrize("kind", ["a1c2", "mck4"])
def test_fused_routes_on_orbit_batches_at_short_histories(kind, history, plan):
    """History 9: a chunk's split point takes every value and the two runs of a chunk may differ in sign per window row; history 8: a whole chunk per run."""
    for normalize in (False, True):
        spec, parent, e, flat = wsg._short_setup(kind, history, normalize, plan)
        _fused_routes(spec, parent.orbit(wsg._group(kind)), e, flat, normalize, batches=(3, 17))


def test_a_step_without_window_buffers_is_refused_for_an_orbit_store():
    """x_out == NULL: the weight-gradient kernel's own series gather takes one table for the whole batch -- refused (MSHGNN_EUNSUPPORTED), the wrappers materialise."""
    from morphsym_hgnn_amd import engine as eng
    recipe, spec, n, store, e, flat = ts._setup("a1c2", "bf16", normalize=False)
    orbit = store.orbit(ws.A1)
    starts = _packed(orbit, 17, "random")
    e.step_mse_series(orbit, starts, flat)
    g = torch.full_like(flat, 7.0)
    with pytest.raises(eng.MshgnnError, match="materialised windows"):
        e.step_mse_series(orbit, starts, flat, grad_flat=g, materialize=False)
    torch.cuda.synchronize()
    assert bool((g == 7.0).all())
    e.step_mse_series(store, starts & ((1 << SHIFT) - 1), flat, materialize=False)      # (a single table: accepted as before)


# --- 3. equivariance inside one orbit batch, on rounding-free data ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("plan", ["bf16", "x3"])
@pytest.mark.parametrize("kind", ["a1c2", "mck4"])
def test_equivariance_inside_one_orbit_batch_on_rounding_free_data(kind, plan):
    """As test_equivariance_end_to_end_on_rounding_free_data (tests/test_window_symmetry_gpu.py), with the whole orbit of every window in ONE batch:
    out[g . w] == g . out[w] exactly wherever the model family is equivariant (MiniCheetah-K4 under all three, the C2 model under gs), and every block equals
    the fp64 oracle on the transformed windows."""
    from morphsym_hgnn_amd import engine as eng
    from morphsym_hgnn_amd.windows import SequenceStore, quadsdk_a1_c2_recipe, minicheetah_k4_recipe
    from tests import exact_data as xd
    if kind == "a1c2":      # depth 4: the base nodes are live
        spec, knobs, recipe, n_out = helpers.make_spec("c2", "a1-c2", "a1-c2", 128, 4, True), dict(rel_scales=(1.0,)), quadsdk_a1_c2_recipe(ws.JP, ws.FP, T, 3), 12
    else:
        spec, knobs = helpers.make_spec("k4", "mini_cheetah-k4", "mini_cheetah-k4", 128, 3, False), dict(rel_scales=(1.0,), bias_range=(0, 1))
        recipe, n_out = minicheetah_k4_recipe(ws.JP, ws.FP, T), 8
    group, seed, starts = wsg._group(kind), 3, [0, 3, 10]
    case = xd.exact_case(spec, 1, seed, mse=False, **knobs)
    seq = wsg._exact_series(kind, seed)
    n = len(starts)

    def oracle(r):
        rows = [ws.evaluate(r, seq, st)[0] for st in starts]
        c = dict(case, B=n, x={t: torch.cat([torch.from_numpy(x[t]) for x in rows]).double() for t in r.node_types})
        ref = xd.reference(spec, c)
        assert all(bool(xd.bf16_exact(h)) for h in ref["hidden"])
        return ref["out"].reshape(n, n_out)

    def g_of(out, op):
        if kind == "a1c2":
            P, c = group.table("fs", op)
            return out[:, P] * torch.tensor(c, dtype=out.dtype, device=out.device)
        P, _ = group.table("ls", op)
        return out.reshape(-1, 4, 2)[:, P, :].reshape(-1, 8)

    orbit = SequenceStore(seq, recipe, dtype=plan).orbit(group)
    e = eng.Engine(spec, plan)
    flat = eng.flatten_params(spec, case["params"], e.device)
    # window-major: the four elements of one window sit next to each other inside a tile
    st = torch.tensor([s for s in starts for _ in range(K)], dtype=torch.int64)
    el = torch.tensor([k for _ in starts for k in range(K)], dtype=torch.int64)
    out = e.forward_series(orbit, (st | (el << SHIFT)).cuda(), flat, labels=False)[3].double().cpu().reshape(n, K, n_out)
    out0 = out[:, 0]
    assert torch.equal(out0, oracle(recipe)) and int((out0 != 0).sum()) > out0.numel() // 2
    for k, op in enumerate(OPS, 1):
        assert torch.equal(out[:, k], oracle(recipe.transformed(op, group))), op
        if kind == "mck4" or op == "gs":
            assert torch.equal(out[:, k], g_of(out0, op)) and not torch.equal(out[:, k], out0), op


# --- 4. the wrappers over an orbit dataset ----------------------------------------------------------------------------------------------------------------

def _orbit_dataset(kind, normalize, plan):
    ds, _ = wsg._sibling_dataset(kind, normalize, plan, "gs")
    return ds, ds.orbit(wsg._group(kind))


def _orbit_indices(view, B, seed=0):
    """B indices of an orbit view: the first and last index of every element block in front, then random ones"""
    n = view.n_windows
    ix = torch.randint(0, len(view), (B,), generator=torch.Generator().manual_seed(B + seed))
    edge = [e * n + k for e in range(view.n_elements) for k in (0, n - 1)][:B]
    ix[:len(edge)] = torch.tensor(edge)
    return ix


@pytest.mark.parametrize("kind,plan,normalize", [("a1c2", "bf16", False), ("a1c2", "x3", True), ("mck4", "bf16", True), ("mck4", "x3", False)])
def test_wrapper_steps_on_an_orbit_batch(kind, plan, normalize, monkeypatch):
    """training_step / validation_step on `orbit.view().batch(device indices)` take the fused series routes -- nothing assembled -- and equal the same steps on
    the orbit store's assembled batch: loss and the whole flat gradient.  The batch's labels are those of the transformed windows."""
    ds, orbit = _orbit_dataset(kind, normalize, plan)
    w, spec, dev = td._wrapper(kind, plan, orbit)
    view, B = orbit.view(), 17
    assert len(view) == K * len(ds.view()) and view.n_windows == len(ds)
    ix = _orbit_indices(view, B)
    ei = spec.topology.edge_index_dict(B, device=dev)
    el, rows = ix // view.n_windows, td._mirror(ds.view(), ix % view.n_windows)
    assert torch.equal(view.starts(ix).cpu(), rows | (el << SHIFT)) and torch.equal(view.starts(ix.cuda()).cpu(), rows | (el << SHIFT))
    xs, y, _ = orbit.assemble(rows.tolist(), elements=el.tolist())
    plain = types.SimpleNamespace(x_dict={t: x.clone() for t, x in zip(orbit.recipe.node_types, xs)}, edge_index_dict=ei, y=y.clone(), batch_size=B)
    sib_y = [s.assemble(rows.tolist())[1].clone() for s in [ds] + [ds.transformed(op, wsg._group(kind)) for op in OPS]]
    assert torch.equal(y, _pick(sib_y, el))

    def run(batch):
        w.model.zero_grad()
        loss = w.training_step(batch, 0)
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach().clone(), w.model._gflat.clone()

    loss_a, flat_a = run(plain)
    assert bool(flat_a.any()) and bool(torch.isfinite(flat_a).all())
    with torch.no_grad():
        val_a = w.validation_step(plain, 0).detach().clone()
    wb = view.batch(ix.cuda(), ei)
    assert wb.store is orbit and torch.equal(wb.elements.cpu(), el)
    with monkeypatch.context() as m:
        m.setattr(orbit, "assemble", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the fused route assembles nothing")))
        loss_b, flat_b = run(wb)
        with torch.no_grad():
            wv = view.batch(ix.cuda(), ei)
            val_b = w.validation_step(wv, 0).detach().clone()
            assert wv._x is None      # evaluation materialises nothing
    assert torch.equal(wb.y, y)
    assert torch.equal(loss_b, loss_a) and torch.equal(flat_b, flat_a) and torch.equal(val_b, val_a)
    # host elements on a WindowBatch of the store itself: the same step
    wh = orbit.batch(rows.tolist(), ei, elements=el.tolist())
    assert torch.equal(wh.starts, wb.starts)
    loss_c, flat_c = run(wh)
    assert torch.equal(loss_c, loss_a) and torch.equal(flat_c, flat_a)
    with pytest.raises(IndexError):
        orbit.batch(rows.tolist(), ei, elements=[K] * B)
    view.check()


@pytest.mark.parametrize("normalize,plan", [(False, "bf16"), (True, "x3")])
def test_evaluate_sequence_over_an_orbit_view_returns_the_orbits_blocks(normalize, plan):
    from morphsym_hgnn_amd import wrappers
    ds, orbit = _orbit_dataset("a1c2", normalize, plan)
    w, spec, dev = td._wrapper("a1c2", plan, orbit)
    ei1 = spec.topology.edge_index_dict(1, device=dev)
    sibs = [ds] + [ds.transformed(op, ws.A1) for op in OPS]
    train, val = orbit.split()
    for view, pick in ((val, lambda s: s.split()[1]), (orbit, lambda s: s)):
        got = wrappers.evaluate_sequence(w, view, ei1, 17).clone()
        want = [wrappers.evaluate_sequence(w, pick(s), ei1, 64).clone() for s in sibs]
        n = want[0].shape[0]
        assert got.shape[0] == K * n
        for e in range(K):
            assert torch.equal(got[e * n:(e + 1) * n], want[e]), e
        assert not torch.equal(want[1], want[0])
    assert train.ranges == ds.split()[0].ranges and len(train) == K * len(ds.split()[0])      # the same windows under every element


def test_graphed_training_step_replays_new_indices_on_an_orbit_view():
    """GraphedTrainingStep(index_source=an orbit view): (element, window) split + mapping kernel + orbit series step + Adam captured once; replays on fresh
    indices equal the eager steps of a twin.  A shuffled epoch over such a view is augmented training."""
    from morphsym_hgnn_amd import wrappers
    B, twins = 17, []
    for _ in range(2):
        ds, orbit = _orbit_dataset("a1c2", False, "bf16")
        w, spec, dev = td._wrapper("a1c2", "bf16", orbit)
        w.lr = 1e-3
        w.graph_safe_optimizer = True
        twins.append((w, w.configure_optimizers(), orbit.split()[0]))
    (a, oa, va), (b, ob, vb) = twins
    ei = spec.topology.edge_index_dict(B, device=dev)
    batches = [_orbit_indices(va, B, seed=k).cuda() for k in range(3)]
    gs = wrappers.GraphedTrainingStep(a, oa, va.batch(batches[0], ei), index_source=va)
    assert va.dataset.desc.sign_flags == (3 | K << 8)
    for k, ix in enumerate(batches[1:]):
        loss_a = gs(ix)
        ob.zero_grad(set_to_none=True)
        loss_b = b.training_step(vb.batch(ix, ei), 0); loss_b.backward(); ob.step()
        torch.cuda.synchronize()
        assert torch.equal(loss_a.detach().reshape(-1), loss_b.detach().reshape(-1)), k
        for p, q in zip(a.model.parameters(), b.model.parameters()):
            assert torch.equal(p.detach(), q.detach()), k
    va.check()
    seen = torch.cat([ix for ix in va.epoch(64, generator=torch.Generator().manual_seed(1))]).cpu()
    assert torch.equal(seen.sort().values, torch.arange(len(va)))


def test_an_out_of_range_index_of_an_orbit_view_raises_the_flag():
    ds, orbit = _orbit_dataset("a1c2", False, "bf16")
    view = orbit.split()[1]
    n = view.n_windows
    for bad in (K * n, -1, K * n + 5):
        ix = torch.tensor([0, n, bad, K * n - 1], dtype=torch.int64).cuda()
        st = view.starts(ix).cpu()
        good = view.starts([0, n, K * n - 1])
        assert torch.equal(st[[0, 1, 3]], good.cpu()) and int(st[2]) == 0      # row 0 of element 0
        with pytest.raises(IndexError):
            view.check()
        view.check()      # (cleared)
    with pytest.raises(IndexError):
        view.starts([K * n])


# --- 5. refusals before any launch; 6. an element index one beyond --------------------------------------------------------------------------------------

def test_bad_orbit_tables_are_refused_before_anything_is_written():
    from morphsym_hgnn_amd import engine as eng
    from morphsym_hgnn_amd.windows import SequenceStore, quadsdk_a1_c2_recipe
    FLAG = SequenceStore.SIGN_FLAG
    for what in ("nine elements", "another structure", "signed constant run", "capture"):
        orbit = SequenceStore(ws.SEQ, quadsdk_a1_c2_recipe(ws.JP, ws.FP, T), dtype="f32").orbit(ws.A1)
        n_runs = int(orbit.desc.n_runs)
        runs = orbit.runs.view(K, n_runs, 5)
        if what == "nine elements":
            orbit.desc.sign_flags = 1 | 9 << 8
        elif what == "another structure":
            runs[2, 5, 4] -= 1      # one run of element 2 is a step shorter
        elif what == "signed constant run":
            r = int((runs[0, :, 3] == -1).nonzero()[0, 0])
            runs[3, r, 3] = -1 - FLAG
        xs, y, q = orbit._buffers(3)
        for t in xs + [y, q]:
            t.fill_(7.0)
        starts = (torch.tensor([0, 1, 2]) | (torch.tensor([1, 2, 3]) << SHIFT)).cuda()
        torch.cuda.synchronize()
        with pytest.raises(eng.MshgnnError) as ei:
            if what == "capture":      # the check is a synchronous read-back: it cannot run inside a capture, and nothing vouches yet
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    with torch.cuda.graph(torch.cuda.CUDAGraph(), stream=side):
                        orbit.assemble(starts, reuse_buffers=True)
            else:
                orbit.assemble(starts, reuse_buffers=True)
        torch.cuda.synchronize()
        msg = {"nine elements": "at most 8", "another structure": "differs from element 0's", "signed constant run": "constant-1", "capture": "stream capture"}[what]
        assert msg in str(ei.value), str(ei.value)
        assert all(bool((t == 7.0).all()) for t in xs + [y, q])
        assert orbit.desc.sign_flags & 2 == 0      # never vouched for
    # the fused routes run the same check
    recipe, spec, seq, n, store, e, flat = se._setup("a1c2_L2", "bf16")
    orbit = store.orbit(ws.A1)
    orbit.runs.view(K, -1, 5)[1, 7, 2] += 2
    out = torch.full((3 * e.n_out, spec.out_channels), 7.0, device="cuda")
    with pytest.raises(eng.MshgnnError, match="differs from element 0's"):
        e.forward_series(orbit, starts, flat, out=out)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


@pytest.mark.parametrize("fast", [True, False], ids=["chunk-gather", "run-gather"])
def test_an_element_index_one_beyond_yields_the_last_element(fast):
    """A device `starts` entry whose element index is K (and 255): clamped to K - 1 inside the kernels -- the rows of the last element, never a read past the tables."""
    from morphsym_hgnn_amd.windows import SequenceStore
    recipe, seq, group = _recipe("mck4", T, True)
    for dtype in ("bf16", "x3"):
        store = SequenceStore(seq, recipe, dtype=dtype, fast=fast)
        orbit = store.orbit(group)
        rows = _starts(len(store), 17)
        el = _elements("alternating", 17)
        beyond = el.clone(); beyond[el == K - 1] = K; beyond[5] = 255
        el[5] = K - 1
        want = orbit.assemble(rows.cuda() | (el.cuda() << SHIFT))
        got = orbit.assemble(rows.cuda() | (beyond.cuda() << SHIFT))
        for a, b in zip(want[0] + [want[1]], got[0] + [got[1]]):
            assert torch.equal(a, b)
        if fast:      # the fused routes clamp alike
            spec = ts._model("mck4_cls", True)[1]
            from morphsym_hgnn_amd import engine as eng, synth
            e = eng.Engine(spec, dtype)
            flat = eng.flatten_params(spec, synth.make_params(8, spec.param_shapes()), e.device)
            a = ts._yardstick(orbit, e, spec, flat, rows.cuda() | (el.cuda() << SHIFT))
            ts._poison(orbit, 17)
            ts._check_step(orbit, e, spec, rows.cuda() | (beyond.cuda() << SHIFT), a, e.step_ce_series_std(orbit, rows.cuda() | (beyond.cuda() << SHIFT), flat))
            out = e.forward_series(orbit, rows.cuda() | (beyond.cuda() << SHIFT), flat)[3]
            torch.cuda.synchronize()
            assert torch.equal(out, se._yardstick(orbit, e, flat, rows.cuda() | (el.cuda() << SHIFT))[3])
