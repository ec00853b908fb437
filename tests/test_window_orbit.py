"""Orbit batches on the host: the stacked element tables of `SequenceStore.orbit` against the tables of each `WindowRecipe.transformed`, the structures
that are refused, and the (element, window) index mapping of an orbit view against a plain-Python ConcatDataset of per-element views.  No GPU: the tables
are built by `WindowRecipe.tables` / `stack_orbit_tables`, and `SequenceStore._describe` is run on a store whose series are host tensors."""
import types

import numpy as np
import pytest
import torch

from tests import test_window_symmetry as ws
from morphsym_hgnn_amd import windows as W
from morphsym_hgnn_amd.windows import (DatasetView, SequenceStore, dataset_index_map, dataset_lookup, dataset_split_ranges, minicheetah_k4_recipe,
                                       orbit_index_split, quadsdk_a1_c2_recipe, stack_orbit_tables)

OPS = ws.OPS
ROBOTS = {"a1c2": (lambda: quadsdk_a1_c2_recipe(ws.JP, ws.FP, ws.T, 3, True), ws.A1, ws.SEQ),
          "mck4": (lambda: minicheetah_k4_recipe(ws.JP, ws.FP, ws.T), ws.K4, ws.SEQ4)}


def _host_store(recipe, seq):
    """A SequenceStore without a device: what `_describe` needs of one (names, the series as [columns, rows + 8] host tensors)."""
    st = object.__new__(SequenceStore)
    st.device, st.dtype, st._fast = torch.device("cpu"), "bf16", True
    st.names = recipe.series()
    st.series = [torch.zeros(np.asarray(seq[s]).reshape(len(seq[s]), -1).shape[1], len(seq[s]) + 8) for s in st.names]
    return st


@pytest.mark.parametrize("mode", ws.MODES)
@pytest.mark.parametrize("robot", sorted(ROBOTS))
def test_stacked_tables_are_the_elements_tables(robot, mode):
    make, group, seq = ROBOTS[robot]
    recipe = make()
    orbit = _host_store(recipe, seq)
    recipes = recipe.orbit(group, OPS, mode)
    orbit._describe(recipes[0], recipes)
    K = 4
    assert orbit.n_elements == K and orbit.recipe is recipe
    d = orbit.desc
    assert d.sign_flags == (1 | K << 8) and (d.sign_flags >> 8) & 0xff == K
    runs, lab = orbit.runs.reshape(K, d.n_runs, 5), orbit.label_cols.reshape(K, d.n_label)
    flagged = 0
    for e, op in enumerate((None,) + OPS):
        one = _host_store(recipe, seq)
        r_e = recipe if op is None else recipe.transformed(op, group, mode)
        one._describe(r_e)
        assert one.n_elements == 1 and one.desc.sign_flags in (0, 1)
        assert one.desc.n_runs == d.n_runs and one.desc.n_rows == d.n_rows and one.desc.n_label == d.n_label
        assert torch.equal(runs[e], one.runs) and torch.equal(lab[e], one.label_cols) and torch.equal(orbit.rows, one.rows)
        # ... and `_describe` builds what the recipe-level host code builds
        t_runs, t_rows, t_lab, signed = r_e.tables(orbit.names)
        assert one.runs.tolist() == t_runs and one.rows.tolist() == t_rows and one.label_cols.tolist() == t_lab and one.desc.sign_flags == int(signed)
        flagged += int(((one.runs[:, 3] >= 0) & ((one.runs[:, 3] & W.SIGN_FLAG) != 0)).sum())
        if e:
            assert not torch.equal(runs[e], runs[0])      # a transformed element is another table
    assert (flagged > 0) == (mode == "MorphSym")
    # identity=False, one operator: one element, the descriptor of `transformed`
    single = _host_store(recipe, seq)
    rs = recipe.orbit(group, ("gt",), mode, identity=False)
    single._describe(rs[0], rs)
    assert single.n_elements == 1 and single.desc.sign_flags >> 8 == 0


def _tables(robot):
    make, group, _ = ROBOTS[robot]
    return [r.tables()[:3] for r in make().orbit(group)]


def test_refused_structures():
    tabs = _tables("a1c2")
    stack_orbit_tables(tabs)      # (as built: accepted)
    # one run length tampered in one element
    bad = [([list(r) for r in runs], rows, lab) for runs, rows, lab in tabs]
    bad[2][0][5][4] -= 1
    with pytest.raises(ValueError, match="differs from element 0's"):
        stack_orbit_tables(bad)
    # a constant-1 run that is a series run in another element
    bad = [([list(r) for r in runs], rows, lab) for runs, rows, lab in tabs]
    ones = [i for i, r in enumerate(bad[1][0]) if r[3] == -1]
    assert ones
    bad[1][0][ones[0]][3] = 0
    with pytest.raises(ValueError, match="constant-1"):
        stack_orbit_tables(bad)
    # a "signed" constant-1 run
    bad = [([list(r) for r in runs], rows, lab) for runs, rows, lab in tabs]
    bad[3][0][ones[0]][3] = -1 - W.SIGN_FLAG
    with pytest.raises(ValueError, match="constant-1"):
        stack_orbit_tables(bad)
    # another first feature, another node, other rows, other label counts, too many elements
    for col in (1, 2):
        bad = [([list(r) for r in runs], rows, lab) for runs, rows, lab in tabs]
        bad[1][0][3][col] += 1
        with pytest.raises(ValueError, match="differs from element 0's"):
            stack_orbit_tables(bad)
    with pytest.raises(ValueError, match="node rows differ"):
        stack_orbit_tables([tabs[0], (tabs[1][0], tabs[1][1][:-1], tabs[1][2])])
    with pytest.raises(ValueError, match="label columns"):
        stack_orbit_tables([tabs[0], (tabs[1][0], tabs[1][1], tabs[1][2][:-1])])
    with pytest.raises(ValueError, match="1 to 8"):
        stack_orbit_tables([tabs[0]] * 9)
    make, group, _ = ROBOTS["mck4"]
    with pytest.raises(ValueError, match="1 to 8"):
        make().orbit(group, OPS * 3)
    with pytest.raises(ValueError, match="1 to 8"):
        make().orbit(group, (), identity=False)


def _orbit_view(lengths, history, K, ranges):
    ds = types.SimpleNamespace(seq_rows=list(lengths), recipe=types.SimpleNamespace(history=history), device=torch.device("cpu"), n_elements=K)
    return DatasetView(ds, ranges)


@pytest.mark.parametrize("which", ["train", "val", "all"])
def test_index_mapping_is_the_concat_dataset_of_the_element_views(which):
    lengths, history, K = (150, 163, 407, 151), 150, 4      # unequal lengths; the first sequence has one window: its training range is empty
    train, val = dataset_split_ranges(lengths, history)
    ranges = {"train": train, "val": val, "all": [(0, n - history + 1) for n in lengths]}[which]
    view = _orbit_view(lengths, history, K, ranges)
    cum, first = dataset_index_map(lengths, history, ranges)
    n = cum[-1]
    # the reference's order: ConcatDataset([view, view_gs, view_gt, view_gr]), each a ConcatDataset of per-sequence Subsets
    concat = [(e, dataset_lookup(cum, first, i)) for e in range(K) for i in range(n)]
    assert len(view) == len(concat) == K * n and view.n_windows == n and n > 0
    edge = sorted({e * n + k for e in range(K) for k in (0, n - 1)} | {cum[s] + e * n for e in range(K) for s in range(len(lengths)) if cum[s] < n})
    rng = np.random.default_rng(5)
    index = edge + [int(i) for i in rng.integers(0, K * n, 64)]
    packed = view.starts(index).tolist()
    for i, p in zip(index, packed):
        assert (p >> W.ELEMENT_SHIFT, p & W.ROW_MASK) == concat[i], i
        assert orbit_index_split(i, n, K) == (i // n, i % n) == (concat[i][0], i - concat[i][0] * n)
    # the same windows under every element: a split divides windows, not (element, window) pairs
    rows = [p & W.ROW_MASK for p in view.starts(list(range(K * n))).tolist()]
    assert all(rows[e * n:(e + 1) * n] == rows[:n] for e in range(K))
    for bad in (-1, K * n):
        with pytest.raises(IndexError):
            view.starts([0, bad])
        with pytest.raises(IndexError):
            orbit_index_split(bad, n, K)
    # one element: the view it always was
    plain = _orbit_view(lengths, history, 1, ranges)
    assert len(plain) == n and plain.starts(list(range(n))).tolist() == rows[:n]
