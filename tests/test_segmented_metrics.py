"""Per-segment metrics without a GPU: the numpy mirror `metrics.segmented_reference` (the GPU tests' yardstick) against a per-segment call of the plain
fp64 formulas, its overflow row, `DatasetView.segments` on host indices against `dataset_lookup` plus the ConcatDataset order, and the CSV layout of
`wrappers.EvaluationTable` from a hand-made table."""
import csv
import io
import math
import types

import numpy as np
import pytest
import torch

from morphsym_hgnn_amd import metrics as M
from morphsym_hgnn_amd import windows as W
from morphsym_hgnn_amd import wrappers


def _plain_regression(y, y_pred):
    d = y_pred.astype(np.float64) - y.astype(np.float64)
    return math.fsum((d * d).ravel()), math.fsum(np.abs(d).ravel()), float(d.size)


def _plain_classification(logits, labels):
    """One segment's sums by the textbook formulas, window by window in Python floats (fp64): log-sum-exp cross entropy, argmax with the first maximum,
    the 16-class product rule."""
    ce, c = [], np.zeros(18, dtype=np.int64)
    for lg, lab in zip(logits.reshape(-1, 4, 2).astype(np.float64), labels.reshape(-1, 4)):
        p1, state = [], 0
        for k in range(4):
            l0, l1 = float(lg[k, 0]), float(lg[k, 1])
            m = max(l0, l1)
            e0, e1 = float(np.exp(l0 - m)), float(np.exp(l1 - m))
            ce.append((m + float(np.log(e0 + e1))) - (l1 if lab[k] else l0))
            p0, pk = e0 / (e0 + e1), e1 / (e0 + e1)
            p1.append(pk)
            pred = pk > p0
            c[2 + 4 * k + (0 if pred and lab[k] else 1 if pred else 2 if lab[k] else 3)] += 1
            state = state * 2 + int(bool(lab[k]))
        best, bestv = 0, -1.0
        for j in range(16):
            f = [p1[k] if (j >> (3 - k)) & 1 else 1.0 - p1[k] for k in range(4)]
            v = (f[0] * f[1]) * (f[2] * f[3])
            if v > bestv:
                best, bestv = j, v
        c[0] += 1
        c[1] += best == state
    return math.fsum(ce), float(len(ce)), c


def test_regression_mirror_is_the_plain_formulas_per_segment():
    rng = np.random.default_rng(0)
    B, per, n_seg = 301, 12, 5
    y, yp = rng.standard_normal((B, per)).astype(np.float32), rng.standard_normal((B, per)).astype(np.float32)
    seg = rng.integers(0, n_seg - 1, B).astype(np.int32)          # (segment n_seg - 1 stays empty)
    state = M.segmented_reference(y, yp, seg, n_seg, True)
    assert state.shape == (n_seg + 1, 3) and state.dtype == np.float64
    for s in range(n_seg - 1):
        assert tuple(state[s]) == _plain_regression(y[seg == s], yp[seg == s])
    assert not state[n_seg - 1].any() and not state[n_seg].any()
    assert state[:, 2].sum() == B * per
    # torch tensors are taken as well
    assert np.array_equal(M.segmented_reference(torch.from_numpy(y), torch.from_numpy(yp), torch.from_numpy(seg), n_seg, True), state)


def test_classification_mirror_is_the_plain_formulas_per_segment():
    rng = np.random.default_rng(1)
    B, n_seg = 97, 3
    logits = rng.standard_normal((B * 4, 2)).astype(np.float32)
    logits[::5, 1] = logits[::5, 0]                              # equal logits: p = 1/2, the first maximum (no contact) wins, 16-class products tie
    labels = rng.integers(0, 2, (B, 4)).astype(np.int32)
    seg = rng.integers(0, n_seg, B).astype(np.int32)
    ce_state, counts = M.segmented_reference(labels, logits, seg, n_seg, False)
    assert ce_state.shape == (n_seg + 1, 2) and counts.shape == (n_seg + 1, 18) and counts.dtype == np.int64
    for s in range(n_seg):
        ce, rows, c = _plain_classification(logits.reshape(B, 8)[seg == s], labels[seg == s])
        assert ce_state[s, 1] == rows and np.array_equal(counts[s], c)
        assert abs(ce_state[s, 0] - ce) <= (rows + 4) * 2.0 ** -53 * ce          # gamma_(m + 4) sum |terms|: the terms differ only by numpy's vector exp / log against the scalar ones
    assert counts[:, 0].sum() == B and not counts[n_seg].any()
    for k in range(4):
        assert (counts[:, 2 + 4 * k:6 + 4 * k].sum(1) == counts[:, 0]).all()


def test_out_of_range_ids_go_to_the_overflow_row():
    y = np.arange(24, dtype=np.float32).reshape(6, 4)
    yp = y + np.array([1, 2, 3, 4, 5, 6], dtype=np.float32)[:, None]
    n_seg = 2
    seg = np.array([0, -1, n_seg, 2 ** 31 - 1, 1, -(2 ** 31)], dtype=np.int64)
    state = M.segmented_reference(y, yp, seg, n_seg, True)
    assert state.tolist() == [[4.0, 4.0, 4.0], [100.0, 20.0, 4.0], [4.0 * (4 + 9 + 16 + 36), 4.0 * (2 + 3 + 4 + 6), 16.0]]
    logits, labels = np.zeros((6 * 4, 2), dtype=np.float32), np.ones((6, 4), dtype=np.int32)
    ce_state, counts = M.segmented_reference(labels, logits, seg.astype(np.int32), n_seg, False)
    assert counts[:, 0].tolist() == [1, 1, 4] and ce_state[:, 1].tolist() == [4.0, 4.0, 16.0]
    with pytest.raises(ValueError):
        M.segmented_reference(y, yp, seg, 0, True)


def _fake_view(lengths, history, ranges=None, n_elements=1, names=None):
    """A DatasetView over a stand-in for a ResidentDataset that holds only what the index maps read (no series, no device)."""
    counts = W.dataset_window_counts(lengths, history)
    ds = types.SimpleNamespace(seq_rows=list(lengths), recipe=types.SimpleNamespace(history=history), device=torch.device("cpu"), n_elements=n_elements,
                               seq_names=names or [f"seq{k}" for k in range(len(lengths))], operators=[None, "gs", "gt", "gr"][:n_elements])
    return W.DatasetView(ds, ranges if ranges is not None else [(0, n) for n in counts])


@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("ranges", [None, [(0, 3), (5, 5), (100, 251), (0, 1)]])
def test_segments_of_host_indices_follow_the_concat_order(K, ranges):
    lengths, history = [200, 170, 400, 150], 150          # 51, 21, 251 and 1 windows
    view = _fake_view(lengths, history, ranges, K)
    n, S = view.n_windows, view.n_sequences
    assert (view.n_sequences, view.segment_shape, view.n_segments) == (4, (K, 4), K * 4) and len(view) == K * n
    assert view.names == ["seq0", "seq1", "seq2", "seq3"]
    # ConcatDataset order: element-major, then the sequences' ranges one after the other; the sequence of a window is the one whose rows hold its start
    bounds = np.concatenate([[0], np.cumsum(lengths)])
    want = []
    for i in range(K * n):
        k, w = W.orbit_index_split(i, n, K) if K > 1 else (0, i)
        row = W.dataset_lookup(view.cum, view.first_row, w)
        want.append(k * S + int(np.searchsorted(bounds, row, side="right")) - 1)
    got = view.segments(np.arange(K * n))
    assert got.dtype == torch.int32 and got.tolist() == want
    # the first and the last window of every sequence and element, asked for one by one (and in a shuffled batch)
    for k in range(K):
        for s in range(S):
            lo, hi = view.cum[s], view.cum[s + 1]
            if hi == lo:
                assert k * S + s not in want          # an empty range owns no index, so no id
                continue
            assert view.segments([k * n + lo, k * n + hi - 1]).tolist() == [k * S + s] * 2
    perm = np.random.default_rng(3).permutation(K * n)
    assert view.segments(torch.from_numpy(perm)).tolist() == [want[i] for i in perm]
    out = torch.empty(5, dtype=torch.int32)
    assert view.segments(perm[:5], out=out) is out and out.tolist() == [want[i] for i in perm[:5]]
    for bad in ([-1], [K * n], [0, K * n]):
        with pytest.raises(IndexError):
            view.segments(bad)
    with pytest.raises(ValueError):
        view.segments([])
    with pytest.raises(ValueError):
        view.segments([0, 1], out=torch.empty(2, dtype=torch.int64))


def test_dataset_names_are_checked_before_a_device_is_touched():
    recipe = W.minicheetah_k4_recipe(list(range(12)), list(range(4)), history=8, normalize=True)
    cols = {"imu_acc": 3, "imu_omega": 3, "q": 12, "qd": 12, "p": 12, "v": 12, "contacts": 4}
    seq = lambda n: {s: np.zeros((n, c), dtype=np.float32) for s, c in cols.items()}
    with pytest.raises(ValueError, match="1 names for 2 sequences"):
        W.ResidentDataset([seq(8), seq(9)], recipe, names=["only"])
    assert _fake_view([8, 9], 8, names=["trot", "pronk"]).names == ["trot", "pronk"]


def test_csv_layout_of_a_regression_table():
    ops, names = ["None", "gs", "gt", "gr"], ["forest", "sidewalk"]
    base = torch.arange(8, dtype=torch.float64).view(4, 2)
    table = {"MSE": base + 0.25, "RMSE": base + 0.5, "L1": base + 0.75, "n": torch.full((4, 2), 7.0, dtype=torch.float64)}
    res = wrappers.EvaluationTable(None, table, ops, names, regression=True)
    buf = io.StringIO()
    res.to_csv(buf)
    rows = list(csv.reader(io.StringIO(buf.getvalue())))
    assert rows[0] == ["Swap", "forest-MSE", "forest-RMSE", "forest-L1", "sidewalk-MSE", "sidewalk-RMSE", "sidewalk-L1"]
    assert len(rows) == 5 and [r[0] for r in rows[1:]] == ops
    for k in range(4):
        assert [float(v) for v in rows[1 + k][1:]] == [2 * k + 0.25, 2 * k + 0.5, 2 * k + 0.75, 2 * k + 1.25, 2 * k + 1.5, 2 * k + 1.75]


def test_csv_layout_of_a_classification_table(tmp_path):
    ops = ["None", "gs"]
    cols = ("accuracy", "f1_leg_0", "f1_leg_1", "f1_leg_2", "f1_leg_3", "f1_avg_legs")
    totals = {c: torch.tensor([0.5 + 0.01 * i, 0.25 + 0.01 * i], dtype=torch.float64) for i, c in enumerate(cols)}
    res = wrappers.EvaluationTable(None, {}, ops, ["a", "b", "c"], regression=False, totals=totals)
    path = tmp_path / "cls.csv"
    res.to_csv(str(path))
    rows = list(csv.reader(open(path)))
    assert rows[0] == ["Symmetry Operator", "Model Accuracy", "Rear-Left", "Front-Left", "Rear-Right", "Front-Right", "F1 Avg"]
    assert [r[0] for r in rows[1:]] == ops
    assert [float(v) for v in rows[1][1:]] == [0.5 + 0.01 * i for i in range(6)] and [float(v) for v in rows[2][1:]] == [0.25 + 0.01 * i for i in range(6)]
    with pytest.raises(ValueError, match="totals"):
        wrappers.EvaluationTable(None, {}, ops, ["a"], regression=False).to_csv(io.StringIO())


def test_table_from_state_rules():
    """Means of an empty segment are NaN, F1 follows 0 / 0 -> 0, n counts windows."""
    state = torch.tensor([[8.0, 4.0, 24.0], [0.0, 0.0, 0.0]], dtype=torch.float64)
    t = M.table_from_state(state, None, per_window=12)
    assert t["MSE"][0] == 8.0 / 24.0 and t["RMSE"][0] == math.sqrt(8.0 / 24.0) and t["L1"][0] == 4.0 / 24.0 and t["n"].tolist() == [2.0, 0.0]
    assert all(math.isnan(float(t[k][1])) for k in ("MSE", "RMSE", "L1"))
    counts = torch.zeros(2, 18, dtype=torch.int64)
    counts[0, :2] = torch.tensor([10, 7])
    for k in range(4):
        counts[0, 2 + 4 * k:6 + 4 * k] = torch.tensor([3, 1, 2, 4]) if k else torch.tensor([0, 0, 0, 10])
    ce = torch.tensor([[20.0, 40.0], [0.0, 0.0]], dtype=torch.float64)
    t = M.table_from_state(ce, counts)
    assert t["CE"][0] == 0.5 and t["accuracy"][0] == 0.7 and t["n"].tolist() == [10.0, 0.0]
    assert t["f1_leg_0"].tolist() == [0.0, 0.0]                              # 0 / 0 -> 0
    f1 = 2 * (0.75 * 0.6) / (0.75 + 0.6)
    assert t["f1_leg_1"][0] == f1 and t["f1_avg_legs"][0] == (0.0 + f1 + f1 + f1) / 4.0
    assert math.isnan(float(t["CE"][1])) and math.isnan(float(t["accuracy"][1]))
