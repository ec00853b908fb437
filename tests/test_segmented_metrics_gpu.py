"""Per-segment step metrics on the GPU (mshgnn_metrics_regression_segmented / _classification_segmented, metrics.SegmentedMetrics,
DatasetView.segments on device indices, wrappers.evaluate_table) against the numpy mirror `metrics.segmented_reference` (tests/test_segmented_metrics.py
pins that to the plain formulas).

Exact cases: y and y_pred hold integers of magnitude <= 64, so every term and every partial sum is an integer below 2^53 and each fp64 addition is
exact whatever its order -- the state must equal the mirror bit for bit.  Rounded cases: the kernel adds a segment's m terms in SOME fixed order (a
lane's terms, a butterfly over the wave, the entries of the merge, the state), each term carrying at most the roundings of its own formation; against
the correctly rounded `math.fsum` of the same terms that is within gamma_(m + 4) * sum |terms|, gamma_k = k u / (1 - k u), u = 2^-53 (Higham, Accuracy
and Stability of Numerical Algorithms, section 4.2: any order of recursive summation).  The bound is computed here from the inputs."""
import ctypes as C
import math
import os
import types

import numpy as np
import pytest
import torch

from morphsym_hgnn_amd import metrics as M
from tests import helpers
from tests import test_windows as tw

pytestmark = pytest.mark.gpu
EINVAL = -1
U = 2.0 ** -53


def _gamma(k):
    return k * U / (1.0 - k * U)


def _ids(pattern, B, n_seg, seed):
    """The id arrangements the kernel must be right for (int32 [B])."""
    rng = np.random.default_rng(seed)
    if pattern == "equal":
        return np.full(B, n_seg - 1, dtype=np.int32)
    if pattern == "runs":          # sorted runs whose borders fall inside a wave: run lengths 1, 37, 64, 100, ...
        out, k = [], 0
        while len(out) < B:
            out += [k % n_seg] * (1, 37, 64, 100)[k % 4]
            k += 1
        return np.asarray(out[:B], dtype=np.int32)
    if pattern == "alternate":     # two ids alternating: one id has an entry in every wave
        return (np.arange(B) % 2 * min(1, n_seg - 1) * (n_seg - 1)).astype(np.int32)
    if pattern == "shuffled":      # all distinct where n_seg >= B, shuffled
        return (rng.permutation(B) % n_seg).astype(np.int32)
    assert pattern == "overflow"   # in-range ids mixed with ids on every side of the range
    out = rng.integers(-2, n_seg + 3, B).astype(np.int64)
    edge = [-1, n_seg, 2 ** 31 - 1, -(2 ** 31), 0, n_seg - 1]
    out[:min(B, len(edge))] = edge[:min(B, len(edge))]
    return out.astype(np.int32)


PATTERNS = ("equal", "runs", "alternate", "shuffled", "overflow")


def _int_pair(B, per, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(-64, 65, (B, per), generator=g).float(), torch.randint(-64, 65, (B, per), generator=g).float())


@pytest.mark.parametrize("B", [1, 63, 64, 65, 257, 8193])
def test_exact_sums_equal_the_mirror_for_every_arrangement_of_ids(B):
    """Integer data: the state `torch.equal`s the mirror; a second call on other data and another arrangement accumulates (same scratch: the ticket
    was reset), the overflow row holds what the out-of-range ids carried."""
    for per in (1, 4, 12):
        y, yp = _int_pair(B, per, 10 * B + per)
        y2, yp2 = _int_pair(B, per, 10 * B + per + 5)
        for n_seg in (1, 3, 8200):
            for i, pattern in enumerate(PATTERNS):
                seg, seg2 = _ids(pattern, B, n_seg, B + i), _ids(PATTERNS[(i + 3) % 5], B, n_seg, B + i + 1)
                m = M.SegmentedMetrics(n_seg, True)
                m.update(y.cuda(), yp.cuda(), torch.from_numpy(seg).cuda())
                want = M.segmented_reference(y, yp, seg, n_seg, True)
                assert torch.equal(m.state.cpu(), torch.from_numpy(want)), (per, n_seg, pattern)
                m.update(y2.cuda(), yp2.cuda(), torch.from_numpy(seg2).cuda())
                want2 = want + M.segmented_reference(y2, yp2, seg2, n_seg, True)
                assert torch.equal(m.state.cpu(), torch.from_numpy(want2)), (per, n_seg, pattern, "second call")
                bad = int(((seg < 0) | (seg >= n_seg)).sum() + ((seg2 < 0) | (seg2 >= n_seg)).sum())
                assert m.overflow() == bad and int(want2[n_seg, 2]) == bad * per
                if bad:
                    with pytest.raises(IndexError):
                        m.check()
                else:
                    m.check()
                t = m.table()
                assert torch.equal(t["n"].cpu(), torch.from_numpy(want2[:n_seg, 2] / per))
                m.reset()
                assert not bool(m.state.any())


def test_one_scratch_serves_calls_of_different_batch_sizes():
    """The ticket is reset and no slot of an earlier, larger call is read: 8193, 65, 1, 257 windows through one SegmentedMetrics."""
    n_seg, per = 7, 12
    m = M.SegmentedMetrics(n_seg, True)
    want = np.zeros((n_seg + 1, 3))
    for k, B in enumerate((8193, 65, 1, 257, 8193)):
        y, yp = _int_pair(B, per, 77 + k)
        seg = _ids(PATTERNS[k], B, n_seg, k)
        m.update(y.cuda(), yp.cuda(), torch.from_numpy(seg).cuda())
        want = want + M.segmented_reference(y, yp, seg, n_seg, True)
        assert torch.equal(m.state.cpu(), torch.from_numpy(want)), B
    assert m._scratch.numel() * 8 == 16 + 1544 * ((8193 + 63) // 64) == int(m.lib.mshgnn_metrics_segmented_scratch_bytes(8193))


@pytest.mark.parametrize("B,n_seg,pattern", [(8193, 3, "runs"), (8193, 8200, "shuffled"), (257, 3, "alternate"), (65, 1, "equal"), (8193, 40, "overflow")])
def test_rounded_sums_are_within_the_summation_bound_and_reproducible(B, n_seg, pattern):
    per = 12
    g = torch.Generator().manual_seed(B + n_seg)
    y, yp = torch.randn(B, per, generator=g), torch.randn(B, per, generator=g)
    seg = _ids(pattern, B, n_seg, 5)
    want = M.segmented_reference(y, yp, seg, n_seg, True)
    states = []
    for _ in range(2):
        m = M.SegmentedMetrics(n_seg, True)
        m.update(y.cuda(), yp.cuda(), torch.from_numpy(seg).cuda())
        states.append(m.state.cpu())
    assert torch.equal(states[0], states[1])          # the reproducibility claim: the same call twice, the same bits
    got = states[0].numpy()
    assert np.array_equal(got[:, 2], want[:, 2])
    terms = want[:, 2]
    bound = np.array([_gamma(k + 4) for k in terms])[:, None] * want[:, :2]          # (the terms are >= 0: sum |terms| is the sum itself)
    err = np.abs(got[:, :2] - want[:, :2])
    print(f"B {B} n_seg {n_seg} {pattern}: worst error / bound {np.max(err / np.maximum(bound, 1e-300)):.3e}")
    assert (err <= bound).all(), (err.max(), bound[err > bound])


def _cls_inputs(B, seed):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(B * 4, 2, generator=g)
    logits[::7, 1] = logits[::7, 0]                     # equal logits: p = 1/2 exactly, the first maximum (no contact) wins ...
    logits.view(B, 8)[1::11] = 0.0                      # ... and whole windows of them: all 16 products tie, class 0 wins
    logits[3::13, 0] = -logits[3::13, 1]
    labels = torch.randint(0, 2, (B, 4), generator=g, dtype=torch.int32)
    return logits, labels


@pytest.mark.parametrize("B,n_seg,pattern", [(1000, 5, "runs"), (1000, 5, "overflow"), (257, 300, "shuffled"), (64, 1, "equal"), (513, 2, "alternate"),
                                                (1153, 1200, "shuffled")])      # (19 slots with 1153 entries: more than one stage of the merge, the staged walk)
def test_classification_counters_are_exact_and_the_cross_entropy_within_the_bound(B, n_seg, pattern):
    logits, labels = _cls_inputs(B, B + n_seg)
    seg = _ids(pattern, B, n_seg, 9)
    want_ce, want_c = M.segmented_reference(labels, logits, seg, n_seg, False)
    m = M.SegmentedMetrics(n_seg, False)
    m.update(labels.cuda(), logits.cuda(), torch.from_numpy(seg).cuda())
    m.update(labels.cuda(), logits.cuda(), torch.from_numpy(seg).cuda())          # twice: the sums double
    counts, ce = m.counts.cpu(), m.state.cpu().numpy()
    assert torch.equal(counts, torch.from_numpy(2 * want_c))
    assert np.array_equal(ce[:, 1], 2 * want_ce[:, 1])
    bound = np.array([_gamma(k + 4) for k in 2 * want_ce[:, 1]]) * 2 * want_ce[:, 0]          # (every per-foot cross entropy is >= 0)
    err = np.abs(ce[:, 0] - 2 * want_ce[:, 0])
    print(f"B {B} n_seg {n_seg} {pattern}: worst CE error / bound {np.max(err / np.maximum(bound, 1e-300)):.3e}")
    assert (err <= bound).all(), (err, bound)
    # the column sums over the segments (overflow row included) are the whole batch's counters, as mshgnn_metrics_classification keeps them
    whole_ce = torch.zeros(2, dtype=torch.float64, device="cuda")
    whole_c = torch.zeros(18, dtype=torch.int64, device="cuda")
    lg, lb = logits.cuda().contiguous(), labels.cuda().contiguous()
    assert m.lib.mshgnn_metrics_classification(lg.data_ptr(), lb.data_ptr(), B, whole_ce.data_ptr(), whole_c.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert torch.equal(counts.sum(0), 2 * whole_c.cpu())
    bad = int(((seg < 0) | (seg >= n_seg)).sum())
    assert m.overflow() == 2 * bad
    t = m.table()
    assert torch.equal(t["n"].cpu(), torch.from_numpy(2.0 * want_c[:n_seg, 0]))
    acc = want_c[:n_seg, 1] / want_c[:n_seg, 0].astype(np.float64) if want_c[:n_seg, 0].all() else None
    if acc is not None:
        assert torch.equal(t["accuracy"].cpu(), torch.from_numpy((2 * want_c[:n_seg, 1]) / (2.0 * want_c[:n_seg, 0])))


def test_bad_arguments_are_refused_before_any_launch():
    B, per, n_seg = 65, 4, 3
    m = M.SegmentedMetrics(n_seg, True)
    lib = m.lib
    y, yp = [t.cuda() for t in _int_pair(B, per, 1)]
    seg = torch.zeros(B, dtype=torch.int32, device="cuda")
    state = torch.full((n_seg + 1, 3), 5.0, dtype=torch.float64, device="cuda")
    ce = torch.full((n_seg + 1, 2), 5.0, dtype=torch.float64, device="cuda")
    counts = torch.full((n_seg + 1, 18), 5, dtype=torch.int64, device="cuda")
    logits, labels = [t.cuda() for t in _cls_inputs(B, 2)]
    m.reserve(B)
    sc = m._scratch
    p = lambda t: t.data_ptr()
    good = [p(yp), p(y), B, per, p(seg), n_seg, p(state), p(sc), None]
    for pos, bad in ((0, None), (1, None), (4, None), (6, None), (7, None), (2, 0), (2, -3), (3, 0), (5, 0), (5, -1), (7, p(sc) + 4)):
        args = list(good)
        args[pos] = bad
        assert lib.mshgnn_metrics_regression_segmented(*args) == EINVAL, (pos, bad)
        assert b"mshgnn_metrics_regression_segmented" in lib.mshgnn_last_error()
    good = [p(logits), p(labels), B, p(seg), n_seg, p(ce), p(counts), p(sc), None]
    for pos, bad in ((0, None), (1, None), (3, None), (5, None), (6, None), (7, None), (2, 0), (4, 0), (7, p(sc) + 4)):
        args = list(good)
        args[pos] = bad
        assert lib.mshgnn_metrics_classification_segmented(*args) == EINVAL, (pos, bad)
        assert b"mshgnn_metrics_classification_segmented" in lib.mshgnn_last_error()
    torch.cuda.synchronize()
    assert bool((state == 5.0).all()) and bool((ce == 5.0).all()) and bool((counts == 5).all()) and not bool(sc.any())
    assert int(lib.mshgnn_metrics_segmented_scratch_bytes(0)) == 0 and int(lib.mshgnn_metrics_segmented_scratch_bytes(64)) == 16 + 1544
    with pytest.raises(ValueError):
        M.SegmentedMetrics(0)
    with pytest.raises(ValueError):
        m.update(y, yp[:-1], seg)


# --- evaluate_table ----------------------------------------------------------------------------------------------------------------------------------
ROWS, T, K = (700, 400, 163), 150, 4          # 551, 251 and 14 windows: batch borders (256) fall inside sequences, the last sequence inside one batch
NAMES = ["forest", "sidewalk", "small_pebbles"]
_CACHE = {}


def _a1_dataset(plan, normalize=False):
    from oracle.gen_window_golden import synthetic_sequence
    from morphsym_hgnn_amd.windows import ResidentDataset, quadsdk_a1_c2_recipe
    if "seqs" not in _CACHE:
        _CACHE["seqs"] = [synthetic_sequence(8100 + 13 * s, n) for s, n in enumerate(ROWS)]
    return ResidentDataset(_CACHE["seqs"], quadsdk_a1_c2_recipe(tw.JP, tw.FP, T, 3, normalize=normalize), dtype=plan, names=NAMES)


def _make_wrapper(kind, plan, dataset, layers=3, **kw):
    from morphsym_hgnn_amd import wrappers
    dev = torch.device("cuda")
    torch.set_default_dtype(torch.float32)
    recipe = dataset.recipe
    if kind == "a1c2":
        spec = helpers.make_spec("c2", "a1-c2", "a1-c2", 128, layers)
        _, cfg = helpers.load_group("a1-c2")
        make = lambda dummy: wrappers.HGNN_C2_Lightning_Reg(128, layers, spec.topology.metadata(), dummy, symmetry_mode="MorphSym", group_operator_path=cfg, **kw)
    else:
        spec = helpers.make_spec("k4", "mini_cheetah-k4", "mini_cheetah-k4", 128, layers, regression=False)
        _, cfg = helpers.load_group("mini_cheetah-k4")
        make = lambda dummy: wrappers.HGNN_K4_Lightning(128, layers, spec.topology.metadata(), dummy, regression=False, symmetry_mode="MorphSym",
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


def _labels_of(orbit, view, k, s):
    """(labels, quaternions) of element k of sequence s of the view, from the store's own assembly"""
    rows = [view.first_row[s] + j for j in range(view.cum[s + 1] - view.cum[s])]
    _, y, q = orbit.assemble(rows, elements=[k] * len(rows)) if orbit.n_elements > 1 else orbit.assemble(rows)
    return y.clone(), (q.clone() if q is not None else None)


def _check_regression_table(res, orbit, view, preds, rotate=None, cols=None):
    Kv, S = view.segment_shape
    n = view.n_windows
    table = res.table if rotate is None else res.table_world
    state = (res.metrics if rotate is None else res.metrics_world).state.cpu().numpy()
    for k in range(Kv):
        for s in range(S):
            y, q = _labels_of(orbit, view, k, s)
            p = preds[k * n + view.cum[s]:k * n + view.cum[s + 1]].reshape(y.shape)
            if rotate is not None:
                y, p = rotate(q, y), rotate(q, p)
                if cols is not None:
                    y, p = y[:, cols], p[:, cols]
            d = p.double().cpu().numpy() - y.double().cpu().numpy()
            sq, ab, m = math.fsum((d * d).ravel()), math.fsum(np.abs(d).ravel()), d.size
            row = state[k * S + s]
            assert row[2] == m and float(table["n"][k, s]) == y.shape[0] == view.cum[s + 1] - view.cum[s]
            assert abs(row[0] - sq) <= _gamma(m + 4) * sq and abs(row[1] - ab) <= _gamma(m + 4) * ab, (k, s)
            assert abs(float(table["MSE"][k, s]) - sq / m) <= _gamma(m + 4) * sq / m, (k, s)
            assert abs(float(table["L1"][k, s]) - ab / m) <= _gamma(m + 4) * ab / m, (k, s)
            assert float(table["RMSE"][k, s]) == math.sqrt(float(table["MSE"][k, s]))


@pytest.mark.parametrize("plan", ["bf16", "x3"])
def test_evaluate_table_over_an_orbit_view(plan, tmp_path):
    from morphsym_hgnn_amd import wrappers
    ds = _a1_dataset(plan)
    orbit = ds.orbit(tw_group())
    w, spec, dev = _make_wrapper("a1c2", plan, orbit)
    ei1 = spec.topology.edge_index_dict(1, device=dev)
    view = orbit.view()
    assert view.segment_shape == (K, 3) and view.n_windows == 551 + 251 + 14 and view.names == NAMES
    want = wrappers.evaluate_sequence(w, view, ei1, 256).clone()
    epoch = (float(w.mse_loss), float(w.rmse_loss), float(w.l1_loss))
    res = wrappers.evaluate_table(w, view, ei1, 256)
    assert torch.equal(res.predictions, want)
    assert (float(w.mse_loss), float(w.rmse_loss), float(w.l1_loss)) == epoch      # the wrapper's own epoch metrics, as evaluate_sequence leaves them
    assert res.operators == ["None", "gs", "gt", "gr"] and res.names == NAMES and res.metrics.overflow() == 0
    assert all(v.shape == (K, 3) and v.dtype == torch.float64 for v in res.table.values()) and set(res.table) == {"MSE", "RMSE", "L1", "n"}
    _check_regression_table(res, orbit, view, want)
    # the whole table is the epoch the wrapper saw: sums over the segments against its epoch MSE
    st = res.metrics.state[:K * 3].sum(0)
    assert abs(float(st[0] / st[2]) - float(w.mse_loss)) <= 1e-12 * float(w.mse_loss)
    path = tmp_path / "table.csv"
    res.to_csv(str(path))
    lines = open(path).read().splitlines()
    assert lines[0] == "Swap," + ",".join(f"{n}-{m}" for n in NAMES for m in ("MSE", "RMSE", "L1")) and [l.split(",")[0] for l in lines[1:]] == res.operators
    assert float(lines[2].split(",")[4]) == float(res.table["MSE"][1, 1])
    # K = 1 on the plain dataset: one row; a strided sweep keeps n exact
    res1 = wrappers.evaluate_table(w, ds, ei1, 256, stride=3)
    assert res1.operators == ["None"] and res1.table["MSE"].shape == (1, 3)
    assert res1.table["n"].tolist() == [[len(range(0, 551, 3)), len([i for i in range(0, 816, 3) if 551 <= i < 802]), len([i for i in range(0, 816, 3) if i >= 802])]]
    assert torch.equal(res1.predictions, wrappers.evaluate_sequence(w, ds, ei1, 256, stride=3))


def tw_group():
    from tests import test_window_symmetry as ws
    return ws.A1


def test_evaluate_table_in_the_world_frame():
    from morphsym_hgnn_amd import wrappers
    ds = _a1_dataset("bf16")
    orbit = ds.orbit(tw_group())
    w, spec, dev = _make_wrapper("a1c2", "bf16", orbit, grf_body_to_world_frame=True)
    assert w.body_to_world_frame
    ei1 = spec.topology.edge_index_dict(1, device=dev)
    view = orbit.split()[1]          # the validation ranges: a view that does not start at a sequence's first window
    res = wrappers.evaluate_table(w, view, ei1, 256, test_only_on_z=True)
    assert torch.equal(res.predictions, wrappers.evaluate_sequence(w, view, ei1, 256))
    _check_regression_table(res, orbit, view, res.predictions)
    _check_regression_table(res, orbit, view, res.predictions, rotate=w.body_frame_to_world_frame, cols=[2, 5, 8, 11])
    assert res.metrics_world.overflow() == 0 and float(res.table_world["n"][0, 0]) == float(res.table["n"][0, 0])


def test_evaluate_table_of_a_classification_wrapper():
    """MiniCheetah-K4 at 3 layers: the per-segment counters against the mirror on the sweep's own predictions and the store's labels; the CSV row is the
    operator's total over the sequences."""
    from oracle.gen_window_golden import minicheetah_sequence
    from morphsym_hgnn_amd import wrappers
    from morphsym_hgnn_amd.windows import ResidentDataset, minicheetah_k4_recipe
    from tests import test_window_symmetry as ws
    ds = ResidentDataset([minicheetah_sequence(7100 + 13 * s, n) for s, n in enumerate((150, 151, 207))], minicheetah_k4_recipe(ws.JP, ws.FP, T, True), dtype="bf16")
    orbit = ds.orbit(ws.K4)
    w, spec, dev = _make_wrapper("mck4", "bf16", orbit)
    ei1 = spec.topology.edge_index_dict(1, device=dev)
    view = orbit.view()
    res = wrappers.evaluate_table(w, view, ei1, 64)
    n, S = view.n_windows, 3
    assert n == 1 + 2 + 58 and res.names == ["seq0", "seq1", "seq2"] and res.predictions.shape[0] == K * n
    assert torch.equal(res.predictions, wrappers.evaluate_sequence(w, view, ei1, 64))
    ids = view.segments(torch.arange(K * n, device=dev))
    assert torch.equal(ids.cpu(), view.segments(np.arange(K * n)).cpu())
    labels = torch.cat([_labels_of(orbit, view, k, s)[0] for k in range(K) for s in range(S)])
    want_ce, want_c = M.segmented_reference(labels.cpu().numpy() != 0, res.predictions.cpu().numpy().reshape(-1, 2), ids.cpu().numpy(), K * S, False)
    assert torch.equal(res.metrics.counts.cpu(), torch.from_numpy(want_c)) and not want_c[K * S].any()
    ce = res.metrics.state.cpu().numpy()
    assert (np.abs(ce[:, 0] - want_ce[:, 0]) <= np.array([_gamma(k + 4) for k in want_ce[:, 1]]) * want_ce[:, 0]).all()
    assert res.table["n"].tolist() == [[1.0, 2.0, 58.0]] * K
    tot = M.table_from_state(torch.from_numpy(want_ce[:K * S]).view(K, S, 2).sum(1), torch.from_numpy(want_c[:K * S]).view(K, S, 18).sum(1))
    assert torch.equal(res.totals["accuracy"].cpu(), tot["accuracy"]) and torch.equal(res.totals["f1_avg_legs"].cpu(), tot["f1_avg_legs"])
    rows = res.rows()
    assert [r[0] for r in rows] == ["None", "gs", "gt", "gr"] and rows[2][1] == float(tot["accuracy"][2]) and len(rows[0]) == 7


def test_com_wrappers_and_plain_stores_are_refused():
    from morphsym_hgnn_amd import wrappers
    com = object.__new__(wrappers.COM_HGNN_Lightning)
    with pytest.raises(ValueError, match="COM"):
        wrappers.evaluate_table(com, None, None, 8)
    with pytest.raises(TypeError, match="DatasetView"):
        wrappers.evaluate_table(types.SimpleNamespace(regression=True), object(), None, 8)


def test_segments_and_update_replay_in_a_graph_on_new_indices():
    """torch.cuda.graph over DatasetView.segments (device indices) + SegmentedMetrics.update: replayed on new indices it equals the eager calls bit for bit;
    indices outside [0, K n) map to -1 and land in the overflow row."""
    ds = _a1_dataset("bf16")
    view = ds.orbit(tw_group()).view()
    n, B, per = view.n_windows, 300, 12
    g = torch.Generator().manual_seed(4)
    batches = [torch.randint(0, K * n, (B,), generator=g) for _ in range(3)]
    batches[2][:4] = torch.tensor([-1, K * n, K * n - 1, 0])
    y, yp = torch.randn(B, per, generator=g).cuda(), torch.randn(B, per, generator=g).cuda()
    ix = batches[0].cuda().clone()
    seg = torch.empty(B, dtype=torch.int32, device="cuda")
    m = M.SegmentedMetrics(view.n_segments, True)
    m.reserve(B)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):          # warm-up off the capture
        view.segments(ix, out=seg)
        m.update(y, yp, seg)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    m.reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        view.segments(ix, out=seg)
        m.update(y, yp, seg)
    m.reset()
    eager = M.SegmentedMetrics(view.n_segments, True)
    for b in batches:
        ix.copy_(b.cuda())
        graph.replay()
        eager.update(y, yp, view.segments(b.cuda()))
        torch.cuda.synchronize()
        assert torch.equal(m.state, eager.state)
    host = view.segments(batches[1])
    assert torch.equal(host, view.segments(batches[1].cuda()))
    assert view.segments(batches[2].cuda())[:4].tolist() == [-1, -1, (K - 1) * 3 + 2, 0]
    assert m.overflow() == 2
