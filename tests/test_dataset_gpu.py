"""A resident dataset of several sequences (windows.ResidentDataset / DatasetView, mshgnn_dataset_starts, wrappers.evaluate_sequence on a view,
wrappers.GraphedTrainingStep(index_source=...)).  The dataset is ONE SequenceStore over the concatenated series, so every comparison is torch.equal:
against the host mirror of the index map (tests/test_dataset_index.py pins that to ConcatDataset of Subsets), against per-sequence SequenceStores, and
against assemble-then-step.

Sizes: A1-C2, hidden 128, 3 layers, history 150, sequences of 150 / 151 / 407 rows (1, 2 and 258 windows: the first has exactly one);
minicheetah_k4_recipe(normalize=True), history 8, sequences of 8 / 9 / 40 rows; batches of 17 and 64 windows."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

from oracle.gen_window_golden import synthetic_sequence, minicheetah_sequence
from tests import helpers
from tests import test_windows as tw

pytestmark = pytest.mark.gpu
ROWS = {"a1c2": (150, 151, 407), "mck4": (8, 9, 40)}
HISTORY = {"a1c2": 150, "mck4": 8}
EINVAL = -1


def _sequences(kind):
    make = synthetic_sequence if kind == "a1c2" else minicheetah_sequence
    return [make(7100 + 13 * s, n) for s, n in enumerate(ROWS[kind])]


def _recipe(kind, normalize):
    from morphsym_hgnn_amd.windows import quadsdk_a1_c2_recipe, minicheetah_k4_recipe
    if kind == "a1c2":
        return quadsdk_a1_c2_recipe(tw.JP, tw.FP, HISTORY[kind], 3, normalize=normalize)
    return minicheetah_k4_recipe(tw.JP, tw.FP, HISTORY[kind], normalize)


def _dataset(kind, normalize, dtype="bf16"):
    from morphsym_hgnn_amd.windows import ResidentDataset
    return ResidentDataset(_sequences(kind), _recipe(kind, normalize), dtype=dtype)


def _mirror(view, indices):
    from morphsym_hgnn_amd.windows import dataset_lookup
    return torch.tensor([dataset_lookup(view.cum, view.first_row, int(i)) for i in indices], dtype=torch.int64)


def _edge_indices(view):
    """first and last index of every non-empty range, then every index of the view"""
    edge = [i for s in range(len(view.first_row)) if view.cum[s + 1] > view.cum[s] for i in (view.cum[s], view.cum[s + 1] - 1)]
    return edge + list(range(len(view)))


def _mixed_indices(view, B, seed=0):
    """B indices of the view with repeats, the first and last window of every non-empty range in front"""
    ix = torch.randint(0, len(view), (B,), generator=torch.Generator().manual_seed(B + seed))
    edge = _edge_indices(view)[:2 * len(view.first_row)]
    edge = edge[:min(len(edge), B)]
    ix[:len(edge)] = torch.tensor(edge)
    return ix


# --- 1. the mapping kernel -----------------------------------------------------------------------------------------------------------------------

def test_device_indices_map_to_the_host_mirrors_start_rows():
    from morphsym_hgnn_amd.windows import ResidentDataset
    ds = _dataset("a1c2", False)
    assert len(ds) == 1 + 2 + 258 and ds.n_rows == sum(ROWS["a1c2"]) and ds.seq_first_row == [0, 150, 301]
    train, val = ds.split()
    assert train.ranges == [(0, 0), (0, 1), (0, 218)] and val.ranges == [(0, 0), (1, 1), (218, 257)]
    assert len(train) == 219 and len(val) == 39
    one = ResidentDataset(_sequences("a1c2")[2:], _recipe("a1c2", False))      # n_seq = 1
    views = [ds.view(), train, val, ds.subset([(0, 1), (2, 2), (100, 258)]), ds.subset([(1, 1), (1, 2), (0, 0)]), one.view(), one.split()[1]]
    assert len(one.view()) == 258 and len(one.view().first_row) == 1
    for view in views:
        ix = _edge_indices(view)
        want = _mirror(view, ix)
        got = view.starts(torch.tensor(ix, dtype=torch.int64).cuda())
        assert got.is_cuda and got.dtype == torch.int64 and torch.equal(got.cpu(), want)
        assert torch.equal(view.starts(ix).cpu(), want)                          # host indices: mapped on the host
        assert torch.equal(view.starts(np.asarray(ix)[::-1].copy()).cpu(), want.flip(0))
        view.check()
        assert int(want.min()) >= 0 and int(want.max()) + ds.recipe.history <= view.dataset.n_rows
        with pytest.raises(IndexError):
            view.starts([0, len(view)])
        with pytest.raises(IndexError):
            view.starts([-1])
    # no window of the whole dataset straddles two sequences: index 0 is sequence 0's only window, index 1 the first of sequence 1
    assert _mirror(ds.view(), [0, 1, 2, 3, 260]).tolist() == [0, 150, 151, 301, 301 + 257]


@pytest.mark.parametrize("B", [17, 64])
def test_out_of_range_device_indices_get_row_zero_and_raise_the_flag(B):
    ds = _dataset("a1c2", False)
    view = ds.split()[0]
    ix = _mixed_indices(view, B)
    want = _mirror(view, ix)
    ix[3], ix[B - 2] = -1, len(view)
    want[3], want[B - 2] = 0, 0
    got = view.starts(ix.cuda())
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), want)
    assert int(view.bad.item()) == 1
    # the flag accumulates: a good batch behind the bad one does not clear it
    good = _mixed_indices(view, B, seed=1)
    assert torch.equal(view.starts(good.cuda()).cpu(), _mirror(view, good)) and int(view.bad.item()) == 1
    with pytest.raises(IndexError, match=f"outside \\[0, {len(view)}\\)"):
        view.check()
    view.check()      # cleared by the raise
    # a batch made from such indices is safe to gather: every start is a whole window of the store
    wb = view.batch(ix.cuda(), None)
    assert int(wb.starts.min()) >= 0 and int(wb.starts.max()) + ds.recipe.history <= ds.n_rows
    with pytest.raises(IndexError):
        view.check()


def _raw_call(lib, cum, first, index, out, bad, n_seq=None, batch=None):
    p = lambda t: t.data_ptr() if t is not None else None
    return lib.mshgnn_dataset_starts(p(cum), p(first), len(first) if n_seq is None else n_seq, p(index), index.numel() if batch is None else batch,
                                     p(out), p(bad), C.c_void_p(torch.cuda.current_stream().cuda_stream))


@pytest.mark.parametrize("n_seq", [1, 3, 1024, 1025, 5000])
def test_mapping_kernel_on_both_sides_of_its_lds_threshold_and_past_2_to_the_31(n_seq):
    """The C-ABI directly: up to 1024 sequences the cumulative counts are staged in LDS, beyond that searched in global memory; counts of 2^32 .. 2^33 windows
    per sequence put the indices and rows far past 2^31; every third range is empty; 1000 indices are several workgroups with a ragged last one."""
    from morphsym_hgnn_amd import engine as eng
    lib = eng.load_library()
    rng = np.random.default_rng(n_seq)
    counts = rng.integers(1 << 32, 1 << 33, size=n_seq)
    if n_seq > 2:
        counts[::3] = 0
        counts[-1] = 0
    cum = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    first = (np.arange(n_seq, dtype=np.int64) * (1 << 35) + rng.integers(0, 1 << 20, size=n_seq)).astype(np.int64)
    B = 1000
    ix = rng.integers(0, cum[-1], size=B).astype(np.int64)
    nz = np.flatnonzero(counts)
    edge = np.concatenate([cum[nz], cum[nz + 1] - 1])[:B // 2]      # first and last index of non-empty ranges
    ix[:len(edge)] = edge
    ix[-1], ix[-2], ix[-3] = cum[-1] - 1, cum[-1], -5
    s = np.searchsorted(cum, ix, side="right") - 1
    want = first[np.clip(s, 0, n_seq - 1)] + (ix - cum[np.clip(s, 0, n_seq - 1)])
    want[-2] = want[-3] = 0
    assert (ix > (1 << 31)).any() and (counts[s[:-3]] > 0).all()
    d = lambda a: torch.from_numpy(a).cuda()
    out, bad = torch.full((B,), -7, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    assert _raw_call(lib, d(cum), d(first), d(ix), out, bad) == 0
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), torch.from_numpy(want)) and int(bad.item()) == 1
    # the same indices without the two bad ones: the flag stays down (the kernel does not write it otherwise)
    bad.zero_(); out.fill_(-7)
    assert _raw_call(lib, d(cum), d(first), d(ix[:-3]), out[:-3], bad) == 0
    torch.cuda.synchronize()
    assert torch.equal(out[:-3].cpu(), torch.from_numpy(want[:-3])) and int(bad.item()) == 0 and bool((out[-3:] == -7).all())


def test_mapping_entry_point_refuses_null_pointers_and_empty_batches_before_any_launch():
    from morphsym_hgnn_amd import engine as eng
    lib = eng.load_library()
    assert "mshgnn_dataset_starts" in eng.EXPORTS
    cum, first = torch.tensor([0, 4, 9]).cuda(), torch.tensor([0, 100]).cuda()
    ix = torch.tensor([0, 5, 8, 99]).cuda()
    out, bad = torch.full((4,), -7, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    for args, kw in (((None, first, ix, out, bad), dict(n_seq=2)), ((cum, None, ix, out, bad), dict(n_seq=2)), ((cum, first, None, out, bad), dict(batch=4)),
                     ((cum, first, ix, None, bad), {}), ((cum, first, ix, out, None), {}), ((cum, first, ix, out, bad), dict(batch=0)),
                     ((cum, first, ix, out, bad), dict(batch=-3)), ((cum, first, ix, out, bad), dict(n_seq=0))):
        if args[2] is None:
            rc = lib.mshgnn_dataset_starts(cum.data_ptr(), first.data_ptr(), 2, None, 4, out.data_ptr(), bad.data_ptr(), None)
        else:
            rc = _raw_call(lib, *args, **kw)
        assert rc == EINVAL and b"mshgnn_dataset_starts" in lib.mshgnn_last_error(), (kw, lib.mshgnn_last_error())
    torch.cuda.synchronize()
    assert bool((out == -7).all()) and int(bad.item()) == 0      # nothing was written
    assert _raw_call(lib, cum, first, ix, out, bad) == 0
    torch.cuda.synchronize()
    assert out.tolist() == [0, 101, 104, 0] and int(bad.item()) == 1


# --- 2. windows ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("normalize", [False, True], ids=["plain", "standardised"])
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("kind", ["a1c2", "mck4"])
def test_dataset_windows_are_the_per_sequence_stores_windows(kind, dtype, normalize):
    """dataset.assemble at mapped starts == SequenceStore.assemble of the same window of the same sequence alone (windows, labels, quaternion): the last
    window of sequence 0 (its only one) and the first of sequence 1 are among them, so nothing reads across a boundary that it keeps."""
    from morphsym_hgnn_amd.windows import SequenceStore
    ds = _dataset(kind, normalize, dtype)
    recipe = ds.recipe
    stores = [SequenceStore(seq, recipe, dtype=dtype) for seq in _sequences(kind)]
    assert [len(s) for s in stores] == ds.seq_windows
    view = ds.view()
    for B in (17, 64):
        ix = _mixed_indices(view, B)
        assert ix[:6].tolist() == [0, 0, 1, 2, 3, len(view) - 1]
        xs, y, q = ds.assemble(view.starts(ix.cuda()))
        seq_of = np.searchsorted(np.asarray(view.cum), ix.numpy(), side="right") - 1
        assert set(seq_of.tolist()) == {0, 1, 2}
        for s, store in enumerate(stores):
            pos = np.flatnonzero(seq_of == s)
            xs_s, y_s, q_s = store.assemble((ix.numpy()[pos] - view.cum[s]).tolist())
            for x, x_s, t in zip(xs, xs_s, recipe.node_types):
                n = recipe.num_nodes[t]
                assert torch.equal(x.view(B, n, -1)[pos], x_s.view(len(pos), n, -1)), (s, t)
            assert torch.equal(y[pos], y_s)
            if recipe.quat_series:
                assert torch.equal(q[pos], q_s)
            else:
                assert q is None and q_s is None


# --- 3. / 4. / 6. the wrappers ----------------------------------------------------------------------------------------------------------------------

def _wrapper(kind, plan, dataset):
    from morphsym_hgnn_amd import wrappers
    dev = torch.device("cuda")
    torch.set_default_dtype(torch.float32)
    recipe = dataset.recipe
    if kind == "a1c2":
        spec = helpers.make_spec("c2", "a1-c2", "a1-c2", 128, 3)
        _, cfg = helpers.load_group("a1-c2")
        make = lambda dummy: wrappers.HGNN_C2_Lightning_Reg(128, 3, spec.topology.metadata(), dummy, symmetry_mode="MorphSym", group_operator_path=cfg)
    else:
        spec = helpers.make_spec("k4", "mini_cheetah-k4", "mini_cheetah-k4", 128, 2, regression=False)
        _, cfg = helpers.load_group("mini_cheetah-k4")
        make = lambda dummy: wrappers.HGNN_K4_Lightning(128, 2, spec.topology.metadata(), dummy, regression=False, symmetry_mode="MorphSym",
                                                        group_operator_path=cfg)
    xs, _, _ = dataset.assemble([0, dataset.seq_first_row[1]])
    dummy = types.SimpleNamespace(edge_index_dict=spec.topology.edge_index_dict(2, device=dev),
                                  x_dict={t: x[:, :recipe.width(t)].float().contiguous() for t, x in zip(recipe.node_types, xs)})
    prev = os.environ.get("MSHGNN_DTYPE")
    os.environ["MSHGNN_DTYPE"] = plan
    try:
        torch.manual_seed(3)
        w = make(dummy).to(dev)
    finally:
        os.environ.pop("MSHGNN_DTYPE", None) if prev is None else os.environ.__setitem__("MSHGNN_DTYPE", prev)
    return w, spec, dev


@pytest.mark.parametrize("plan", ["bf16", "x3"])
@pytest.mark.parametrize("kind,normalize", [("a1c2", False), ("a1c2", True)], ids=["a1c2-plain", "a1c2-std"])
def test_training_step_on_a_view_batch_equals_assemble_then_step(kind, normalize, plan, monkeypatch):
    """training_step on view.batch(device indices) that mixes all three sequences -- the fused series route (plain: mshgnn_step_*_series, standardised:
    their _std forms; store.assemble raises during the call) -- against the step on the assembled plain batch: loss and the whole flat gradient."""
    ds = _dataset(kind, normalize, plan)
    w, spec, dev = _wrapper(kind, plan, ds)
    view = ds.view()
    for B in (17, 64):
        ix = _mixed_indices(view, B)
        ei = spec.topology.edge_index_dict(B, device=dev)
        xs, y, _ = ds.assemble(_mirror(view, ix).tolist())
        plain = types.SimpleNamespace(x_dict={t: x.clone() for t, x in zip(ds.recipe.node_types, xs)}, edge_index_dict=ei, y=y.clone(), batch_size=B)

        def run(batch):
            w.model.zero_grad()
            loss = w.training_step(batch, 0)
            loss.backward()
            torch.cuda.synchronize()
            return loss.detach().clone(), w.model._gflat.clone()

        loss_a, flat_a = run(plain)
        assert bool(flat_a.any()) and bool(torch.isfinite(flat_a).all())
        wb = view.batch(ix.cuda(), ei)
        assert wb.store is ds and wb._x is None and torch.equal(wb.indices.cpu(), ix)
        with monkeypatch.context() as m:
            m.setattr(ds, "assemble", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the fused route assembles nothing")))
            loss_b, flat_b = run(wb)
        assert wb._x is not None and torch.equal(wb.y, y)
        assert torch.equal(loss_b, loss_a) and torch.equal(flat_b, flat_a)
        view.check()


@pytest.mark.parametrize("plan", ["bf16", "x3"])
def test_standardised_series_step_on_the_short_window_dataset_equals_assemble_then_step(plan):
    """The MiniCheetah-K4 dataset at history 8 (sequences of 8 / 9 / 40 rows; the K4 wrappers are fixed at the reference's 150 steps, so this is the
    engine's own step): step_ce_series_std at device-mapped starts that mix all three sequences == dataset.assemble + step_ce -- contact flags, outputs,
    loss and the whole flat gradient."""
    from morphsym_hgnn_amd import engine as eng, synth, topology
    from morphsym_hgnn_amd.spec import ModelSpec
    ds = _dataset("mck4", True, plan)
    r = ds.recipe
    group, _ = helpers.load_group("mini_cheetah-k4")
    spec = ModelSpec(kind="k4", topology=topology.TOPOLOGIES["mini_cheetah-k4"](), hidden=128, num_layers=2, widths={t: r.width(t) for t in r.node_types},
                     regression=False, grf_dimension=3, group=group, num_timesteps=HISTORY["mck4"])
    e = eng.Engine(spec, plan)
    assert not e.generic
    flat = eng.flatten_params(spec, synth.make_params(8, spec.param_shapes()), e.device)
    view = ds.view()
    assert len(view) == 1 + 2 + 33
    for B in (17, 64):
        ix = _mixed_indices(view, B)
        starts = view.starts(ix.cuda())
        assert torch.equal(starts.cpu(), _mirror(view, ix))
        xs, y, _ = ds.assemble(starts)
        lab = (y != 0).to(torch.int32).reshape(B, 4).contiguous()
        out_a, loss_a, g_a = [t.clone() for t in e.step_ce([x.clone() for x in xs], flat, lab, B)]
        xs_b, lab_b, out_b, loss_b, g_b = e.step_ce_series_std(ds, starts, flat)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(xs, xs_b)) and torch.equal(lab_b, lab) and 0 < int(lab.sum()) < lab.numel()
        assert torch.equal(out_b, out_a) and torch.equal(loss_b, loss_a) and torch.equal(g_b, g_a) and bool(g_a.any())
    view.check()


@pytest.mark.parametrize("kind,normalize,plan", [("a1c2", False, "bf16"), ("a1c2", True, "x3"), ("a1c2", True, "bf16")])
def test_evaluate_sequence_on_a_view_is_the_per_sequence_sweeps_cut_to_its_ranges(kind, normalize, plan):
    from morphsym_hgnn_amd import wrappers
    from morphsym_hgnn_amd.windows import SequenceStore
    ds = _dataset(kind, normalize, plan)
    w, spec, dev = _wrapper(kind, plan, ds)
    ei1 = spec.topology.edge_index_dict(1, device=dev)
    per_seq = [wrappers.evaluate_sequence(w, SequenceStore(seq, ds.recipe, dtype=plan), ei1, 64).clone() for seq in _sequences(kind)]
    assert [p.shape[0] for p in per_seq] == ds.seq_windows
    train, val = ds.split()
    n2 = ds.seq_windows[2]
    for view in (val, train, ds.subset([(0, 1), (1, 2), (n2 - 20, n2)]), ds):
        ranges = view.ranges if view is not ds else [(0, n) for n in ds.seq_windows]
        want = torch.cat([p[lo:hi] for p, (lo, hi) in zip(per_seq, ranges)])
        got = wrappers.evaluate_sequence(w, view, ei1, 17)
        assert got.shape[0] == (len(view)) and got.shape[0] % 17 != 0 and torch.equal(got, want)
        assert torch.equal(wrappers.evaluate_sequence(w, view, ei1, 64, stride=3), want[::3])
    assert any(k.startswith("test_") for k in w.logged)


def test_graphed_training_step_replays_dataset_indices_like_the_eager_step():
    """GraphedTrainingStep(index_source=view): index mapping + step from the resident series + FlatAdam(graph_safe) captured once; three index batches through the
    replayed graph == the same three through the eager step on a twin with a dataset of its own (losses, and every parameter after each replay); building the
    graph does not train; the existing constructor without index_source is tests/test_wrappers.py's."""
    from morphsym_hgnn_amd import wrappers
    from morphsym_hgnn_amd.optim import FlatAdam
    B = 17
    twins = []
    for _ in range(2):
        ds = _dataset("a1c2", False, "bf16")
        w, spec, dev = _wrapper("a1c2", "bf16", ds)
        w.lr = 1e-3
        w.graph_safe_optimizer = True
        twins.append((w, w.configure_optimizers(), ds.split()[0]))
    (a, oa, va), (b, ob, vb) = twins
    assert isinstance(oa, FlatAdam) and oa._graph_safe
    for p, q in zip(a.model.parameters(), b.model.parameters()):
        assert torch.equal(p.detach(), q.detach())
    ei = spec.topology.edge_index_dict(B, device=dev)
    batches = [_mixed_indices(va, B, seed=k).cuda() for k in range(4)]
    before = [p.detach().clone() for p in a.parameters()]
    gs = wrappers.GraphedTrainingStep(a, oa, va.batch(batches[0], ei), index_source=va)
    for p, q in zip(a.parameters(), before):
        assert torch.equal(p.detach().float(), q.float()), "building the graph must not train"
    assert int(oa._t_dev.item()) == 0
    for k, ix in enumerate(batches[1:]):
        loss_a = gs(ix if k else ix.cpu())      # host or device indices
        ob.zero_grad(set_to_none=True)
        loss_b = b.training_step(vb.batch(ix, ei), 0); loss_b.backward(); ob.step()
        torch.cuda.synchronize()
        assert torch.equal(gs._starts.cpu(), _mirror(va, ix.cpu()))
        assert torch.equal(loss_a.detach().reshape(-1), loss_b.detach().reshape(-1)), k
        for p, q in zip(a.model.parameters(), b.model.parameters()):
            assert torch.equal(p.detach(), q.detach()), k
    assert int(oa._t_dev.item()) == 3
    assert not all(torch.equal(p.detach().float(), q.float()) for p, q in zip(a.parameters(), before))
    va.check()
    # an index outside the view inside a replay: row 0 is stepped on, the flag tells
    ix = batches[1].clone(); ix[5] = len(va)
    gs(ix)
    torch.cuda.synchronize()
    assert int(gs._starts[5]) == 0
    with pytest.raises(IndexError):
        va.check()
    with pytest.raises(ValueError, match="indices for a step captured on 17"):
        gs(batches[1][:5])


# --- 5. epochs -----------------------------------------------------------------------------------------------------------------------------------

def test_an_epoch_yields_every_index_of_the_view_once():
    ds = _dataset("mck4", True)
    train, val = ds.split()
    assert len(train) == 0 + 1 + 27 and len(val) == 0 + 0 + 5
    big = _dataset("a1c2", False).split()[0]
    for view in (train, big):
        n = len(view)
        for dev in ("cuda", "cpu"):
            runs = []
            for _ in range(2):
                g = torch.Generator(device=dev).manual_seed(5)
                batches = list(view.epoch(32, g))
                assert all(b.is_cuda and b.dtype == torch.int64 for b in batches)
                assert [b.numel() for b in batches] == [32] * (n // 32) + ([n % 32] if n % 32 else [])
                runs.append(torch.cat(batches).cpu())
            assert torch.equal(runs[0], runs[1])                                   # two generators with one seed agree
            assert torch.equal(runs[0].sort().values, torch.arange(n))             # every index exactly once
            other = torch.cat(list(view.epoch(32, torch.Generator(device=dev).manual_seed(6)))).cpu()
            assert n < 3 or not torch.equal(other, runs[0])
        assert n < 3 or not torch.equal(runs[0], torch.arange(n))                  # shuffled
        assert torch.equal(torch.cat(list(view.epoch(32, shuffle=False))).cpu(), torch.arange(n))
        assert sum(b.numel() for b in view.epoch(5, drop_last=True)) == n - n % 5
        assert torch.equal(torch.cat(list(view.epoch(7))).cpu().sort().values, torch.arange(n))      # no generator: the device's default one
    # the end of an epoch reads the flag once: a bad device index mapped during the epoch surfaces there
    it = big.epoch(64, torch.Generator(device="cuda").manual_seed(1))
    first = next(it)
    big.starts(first + len(big))
    with pytest.raises(IndexError):
        for _ in it:
            pass
