"""The index map of a resident dataset of several sequences (windows.dataset_index_map / dataset_split_ranges / dataset_lookup: the host mirror of
mshgnn_dataset_starts) against what the reference's scripts build: `ConcatDataset` of `Subset`s of per-sequence datasets, cut with
int(np.round((len - 1) * 0.85)) (research/train_regression-grf_msgn.py:57-73).  No GPU: the per-sequence datasets are plain `range`s whose item j is
the row of the concatenated series at which window j of that sequence starts."""
import numpy as np
import pytest
from torch.utils.data import ConcatDataset, Subset

from morphsym_hgnn_amd import windows as W


def _per_sequence_datasets(lengths, history):
    """`range` datasets: item j of sequence s = row offset of s in the concatenation + j, one item per window"""
    out, row0 = [], 0
    for n in lengths:
        out.append(range(row0, row0 + n - history + 1))
        row0 += n
    return out


def _script_split(datasets, fraction=0.85, drop_last=True):
    """train_regression-grf_msgn.py:61-69, verbatim arithmetic"""
    train_subsets, val_subsets = [], []
    for dataset in datasets:
        data_len_minus_1 = len(dataset) - 1 if drop_last else len(dataset)
        split_index = int(np.round(data_len_minus_1 * fraction))
        train_subsets.append(Subset(dataset, np.arange(0, split_index)))
        val_subsets.append(Subset(dataset, np.arange(split_index, data_len_minus_1)))
    return ConcatDataset(train_subsets), ConcatDataset(val_subsets)


def _same(concat, cum, first_row):
    assert cum[0] == 0 and cum[-1] == len(concat) and len(cum) == len(first_row) + 1
    assert [W.dataset_lookup(cum, first_row, i) for i in range(len(concat))] == [int(concat[i]) for i in range(len(concat))]
    for i in (-1, len(concat)):
        with pytest.raises(IndexError):
            W.dataset_lookup(cum, first_row, i)


# (rows per sequence, history).  150 / 151 / 407 at history 150: 1, 2 and 258 windows -- m = 0, 1, 257: an empty training AND validation range, a
# validation range that is empty behind one training window.  8 / 9 / 40 at history 8: 1, 2, 33 windows.  The third list has m * 0.85 ending in .5
# on both sides of round-half-even: m = 10 -> 8.5 -> 8, m = 30 -> 25.5 -> 26, m = 50 -> 42.5 -> 42, m = 70 -> 59.5 -> 60 (round-half-up would give 9, 26, 43, 60).
LENGTHS = [([150, 151, 407], 150), ([8, 9, 40], 8), ([11 + 7, 31 + 7, 51 + 7, 71 + 7, 8], 8), ([5], 5), ([300], 150)]


@pytest.mark.parametrize("lengths,history", LENGTHS)
@pytest.mark.parametrize("drop_last", [True, False])
def test_split_views_are_the_scripts_concat_of_subsets(lengths, history, drop_last):
    datasets = _per_sequence_datasets(lengths, history)
    train, val = _script_split(datasets, 0.85, drop_last)
    r_train, r_val = W.dataset_split_ranges(lengths, history, 0.85, drop_last)
    for concat, ranges in ((train, r_train), (val, r_val)):
        cum, first_row = W.dataset_index_map(lengths, history, ranges)
        _same(concat, cum, first_row)
    # every window of every sequence: ConcatDataset of the datasets themselves
    cum, first_row = W.dataset_index_map(lengths, history)
    _same(ConcatDataset(datasets), cum, first_row)
    assert cum[-1] == sum(n - history + 1 for n in lengths)


def test_the_split_rounds_half_to_even_like_numpy():
    lengths, history = LENGTHS[2]
    train, val = W.dataset_split_ranges(lengths, history)
    assert [n - history + 1 - 1 for n in lengths] == [10, 30, 50, 70, 0]
    assert [m * 0.85 for m in (10, 30, 50, 70)] == [8.5, 25.5, 42.5, 59.5]      # the float products are exact halves
    assert [hi for _, hi in train] == [8, 26, 42, 60, 0]
    assert val == [(8, 10), (26, 30), (42, 50), (60, 70), (0, 0)]
    assert W.dataset_split_ranges([150, 151, 407], 150) == ([(0, 0), (0, 1), (0, 218)], [(0, 0), (1, 1), (218, 257)])


def test_empty_ranges_are_skipped_and_no_window_straddles_two_sequences():
    lengths, history = [150, 151, 407], 150
    cum, first_row = W.dataset_index_map(lengths, history, [(1, 1), (0, 2), (0, 0)])
    assert cum == [0, 0, 2, 2] and [W.dataset_lookup(cum, first_row, i) for i in range(2)] == [150, 151]
    cum, first_row = W.dataset_index_map(lengths, history, [(0, 0), (2, 2), (257, 258)])
    assert cum[-1] == 1 and W.dataset_lookup(cum, first_row, 0) == 150 + 151 + 257
    # every window of the whole dataset lies inside ONE sequence's rows
    cum, first_row = W.dataset_index_map(lengths, history)
    bounds = np.concatenate([[0], np.cumsum(lengths)])
    for i in range(cum[-1]):
        st = W.dataset_lookup(cum, first_row, i)
        s = int(np.searchsorted(bounds, st, side="right")) - 1
        assert bounds[s] <= st and st + history <= bounds[s + 1], i
    assert cum[-1] == 1 + 2 + 258 < sum(lengths) - history + 1      # fewer windows than the concatenated rows would give
    # a view of nothing at all
    cum, first_row = W.dataset_index_map(lengths, history, [(0, 0)] * 3)
    assert cum == [0, 0, 0, 0]
    with pytest.raises(IndexError):
        W.dataset_lookup(cum, first_row, 0)


def test_short_sequences_and_bad_ranges_are_refused_by_position():
    with pytest.raises(ValueError, match="sequence 1 .*shorter than one window"):
        W.dataset_index_map([150, 149, 407], 150)
    with pytest.raises(ValueError, match="sequence 2 .*shorter than one window"):
        W.dataset_split_ranges([8, 9, 7], 8)
    with pytest.raises(ValueError, match="sequence 0"):
        W.dataset_index_map([150, 151], 150, [(0, 2), (0, 2)])      # sequence 0 has one window
    with pytest.raises(ValueError, match="sequence 1"):
        W.dataset_index_map([150, 151], 150, [(0, 1), (2, 1)])
    with pytest.raises(ValueError, match="2 sequences"):
        W.dataset_index_map([150, 151], 150, [(0, 1)])


def test_the_dataset_class_is_a_store():
    """ResidentDataset shares SequenceStore's fields by being one; its views carry __len__, batch, starts, epoch and check."""
    assert issubclass(W.ResidentDataset, W.SequenceStore)
    for name in ("__len__", "batch", "starts", "epoch", "check"):
        assert callable(getattr(W.DatasetView, name))
    for name in ("split", "subset", "view"):
        assert callable(getattr(W.ResidentDataset, name))


def test_the_dataset_refuses_short_and_mismatched_sequences_before_it_touches_a_device():
    """A sequence with fewer than `history` rows, or whose series disagree with the first sequence's in column count: ValueError naming its position
    (raised while the sequences are looked over on the host, so it needs no GPU)."""
    recipe = W.minicheetah_k4_recipe(list(range(12)), list(range(4)), history=8, normalize=True)
    cols = {"imu_acc": 3, "imu_omega": 3, "q": 12, "qd": 12, "p": 12, "v": 12, "contacts": 4}
    seq = lambda n, **over: {s: np.zeros((n, over.get(s, c)), dtype=np.float32) for s, c in cols.items()}
    with pytest.raises(ValueError, match="sequence 1 has 7 rows"):
        W.ResidentDataset([seq(8), seq(7), seq(40)], recipe)
    with pytest.raises(ValueError, match=r"sequence 2: series \['p'\] have \[9\] columns"):
        W.ResidentDataset([seq(8), seq(9), seq(40, p=9)], recipe)
    with pytest.raises(ValueError, match="at least one sequence"):
        W.ResidentDataset([], recipe)
    short = seq(40)
    short["q"] = short["q"][:5]          # one series of a sequence shorter than the others: the sequence is as long as its shortest series
    with pytest.raises(ValueError, match="sequence 0 has 5 rows"):
        W.ResidentDataset([short], recipe)
