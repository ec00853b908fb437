"""The Solo centroidal-momentum windows under the symmetry group, on the host: the `symmetry=True` recipes against the action stated from the yaml
(tests/com_symmetry_reference.py), the equivariance identity of the fp64 oracle that pins that action, `OutputAction.from_recipes` on Solo orbits, and the
numpy mirror of the per-segment sums against a restatement of the reference's metric code."""
import dataclasses
import math

import numpy as np
import pytest
import torch

from morphsym_hgnn_amd import metrics as M
from morphsym_hgnn_amd.symmetrise import OutputAction
from morphsym_hgnn_amd.windows import GroupAction, solo_com_arrays, solo_com_mlp_recipe, solo_com_recipe, stack_orbit_tables
from oracle import ms_hgnn_oracle as orc
from tests import com_symmetry_reference as cr
from tests import helpers
from tests import test_windows as tw
from tests import window_reference as wr

JP = tw.JP
OPS = cr.OPS


def make_recipe(kind, history=1, symmetry=True):
    name = cr.KINDS[kind][0]
    return solo_com_mlp_recipe(JP, history, symmetry=symmetry) if name is None else solo_com_recipe(name, JP, history, symmetry=symmetry)


def solo_series(seed, n, zero_base=True):
    """The series of `solo_com_arrays` on random X, Y; zero_base=False: random base series too (the tables are then visible in the base rows)."""
    rng = np.random.default_rng(seed)
    seq = solo_com_arrays(rng.standard_normal((n, 24)).astype(np.float32), rng.standard_normal((n, 6)).astype(np.float32))
    if not zero_base:
        seq["base_lin"], seq["base_ang"] = rng.standard_normal((n, 3)).astype(np.float32), rng.standard_normal((n, 3)).astype(np.float32)
    return seq


def table_reading(recipe, seq, starts, orbit=None, elements=None):
    """tests/window_reference.py's reading of the recipe's own tables: what mshgnn_assemble_windows must produce."""
    names = recipe.series()
    tables = stack_orbit_tables([r.tables(names)[:3] for r in orbit]) if orbit else None
    tab = wr.recipe_tables(recipe, names, "f32", lambda t: recipe.width(t) + 3, tables)
    series = [wr.f32(seq[s]).reshape(len(seq[s]), -1) for s in names]
    st = list(starts) if elements is None else [(e << wr.ELEMENT_SHIFT) | s for s, e in zip(starts, elements)]
    return wr.reference(tab, series, st)


@pytest.mark.parametrize("history", [1, 4])
@pytest.mark.parametrize("kind", list(cr.KINDS))
def test_the_tables_are_the_action_stated_from_the_yaml(kind, history):
    """Inputs and labels of every operator's recipe, read off its tables, equal the yaml action element for element; so do the stacked tables of the orbit."""
    group, raw = GroupAction.load(cr.KINDS[kind][2]), cr.load(cr.KINDS[kind][2])
    seq = solo_series(5 + history, 40, zero_base=False)
    starts = [0, 7, 40 - history]
    r = make_recipe(kind, history)
    assert r.symmetry_parts == {"q": "js", "qd": "js", "base_lin": "bs_lin", "base_ang": "bs_ang", "Y": "bs_linang"}
    assert r.label_slots == list(range(len(r.label_cols))) and r.label_signs is None
    orbit = r.orbit(group)
    for e, op in enumerate((None,) + OPS):
        rec = orbit[e]
        exps = [table_reading(rec, seq, starts), table_reading(r, seq, starts, orbit, [e] * len(starts))]
        for b, st in enumerate(starts):
            xs, y = cr.window(raw, op, kind, seq, st, history, JP)
            for exp in exps:
                for ti, t in enumerate(rec.node_types):
                    assert np.array_equal(exp.x[ti][b][:, :rec.width(t)], xs[t]), (kind, op, t, st)
                assert np.array_equal(exp.y[b], y), (kind, op, st)
        if op is not None:      # the action is visible: some input and some label differ from the untransformed window's
            plain = table_reading(r, seq, starts)
            assert not np.array_equal(exps[0].y, plain.y) and not np.array_equal(exps[0].x[-1], plain.x[-1])


@pytest.mark.parametrize("kind", list(cr.KINDS))
def test_elements_compose_and_are_involutions(kind):
    group = GroupAction.load(cr.KINDS[kind][2])
    r = make_recipe(kind, 4)
    same = lambda a, b: (a.variables == b.variables and a.variable_signs == b.variable_signs and a.label_cols == b.label_cols and a.label_signs == b.label_signs
                         and a.label_slots == b.label_slots)
    gs, gt, gr = (r.transformed(op, group) for op in OPS)
    assert same(gs.transformed("gt", group), gr) and same(gt.transformed("gs", group), gr)
    for g, op in zip((gs, gt, gr), OPS):
        back = g.transformed(op, group)
        assert back.variables == r.variables and back.label_cols == r.label_cols and back.label_slots == r.label_slots
        assert all(x == 1 for t in back.variable_signs.values() for v in t for n in v for x in n) and all(x == 1 for x in back.label_signs)
    # host-only: the slots enter neither the tables nor anything the descriptor is made of
    assert r.tables() == dataclasses.replace(r, label_slots=None).tables()


IDENTITY_CASES = [("solok4com_h128_L3_B5", "k4", ("gs", "gt", "gr")), ("soloc2com_h128_L2_B4", "c2", ("gs",))]
# max |f(g x) - g f(x)| of the fp64 oracle WITHOUT the architecture's symmetry (symmetry_mode=None), measured on the windows of `_oracle_on_orbit`
CONTROL_MEASURED = {("k4", "gs"): 4.943, ("k4", "gt"): 5.303, ("k4", "gr"): 3.889, ("c2", "gs"): 3.350}


def _oracle_on_orbit(case_name, kind, ops, symmetric):
    """(outputs [K][B][6 n_base] of the fp64 oracle on the orbit's windows, the orbit's OutputAction); symmetric=False: the same parameters under symmetry_mode=None."""
    case, spec, _, _, _, params, ei = helpers.load_case(case_name)
    if not symmetric:
        spec = helpers.make_spec(case["kind"], case["topo"], None, case["hidden"], case["layers"], case["regression"], case["grf"])
    B = case["B"]
    seq = solo_com_arrays(tw.SEQS["X"], tw.SEQS["Y"])          # the dataset's base series: zeros
    assert not np.asarray(seq["base_lin"]).any() and not np.asarray(seq["base_ang"]).any()
    recipes = make_recipe(kind).orbit(GroupAction.load(cr.KINDS[kind][2]), ops)
    action = OutputAction.from_recipes(recipes, True, [None] + list(ops))
    cfg = helpers.oracle_config(spec)
    outs = []
    for rec in recipes:
        exp = table_reading(rec, seq, list(range(3, 3 + B)))
        x_dict = {t: torch.from_numpy(exp.x[ti][:, :, :rec.width(t)].reshape(B * rec.num_nodes[t], -1).copy()) for ti, t in enumerate(rec.node_types)}
        outs.append(orc.forward(cfg, params, x_dict, ei).reshape(B, -1))
    return outs, action


def _defects(outs, action):
    return [float((outs[e] - outs[0][:, action.perm[e]] * torch.tensor(action.sign[e], dtype=torch.float64)).abs().max()) for e in range(1, len(outs))]


@pytest.mark.parametrize("case_name,kind,ops", IDENTITY_CASES, ids=[c[1] for c in IDENTITY_CASES])
def test_equivariance_identity_of_the_oracle_is_exact(case_name, kind, ops):
    """f(g x) == g f(x) with max-abs difference exactly 0.0 in fp64 on the dataset's zero base series: the identity that pins the action on inputs AND outputs
    independently of the reference's loader (as tests/test_oracle.py::test_c2_equivariance_identity_is_exact does for the GRF model)."""
    outs, action = _oracle_on_orbit(case_name, kind, ops, True)
    assert float(outs[0].abs().max()) > 0.1
    assert _defects(outs, action) == [0.0] * len(ops)


@pytest.mark.parametrize("case_name,kind,ops", IDENTITY_CASES, ids=[c[1] for c in IDENTITY_CASES])
def test_without_the_symmetric_architecture_the_identity_breaks(case_name, kind, ops):
    """Negative control: the same parameters with symmetry_mode=None.  The oracle itself shows max |f(g x) - g f(x)| = 4.943 (gs), 5.303 (gt), 3.889 (gr) for
    the K4 case and 3.350 (gs) for the C2 case on these windows (outputs of magnitude 2.6 .. 3.7): the test asks for more than half of each."""
    outs, action = _oracle_on_orbit(case_name, kind, ops, False)
    got = _defects(outs, action)
    print(kind, dict(zip(ops, got)))
    for op, d in zip(ops, got):
        assert d > 0.5 * CONTROL_MEASURED[kind, op], (op, d)


@pytest.mark.parametrize("kind", list(cr.KINDS))
def test_output_action_from_recipes_is_the_yaml_action(kind):
    _, nb, gname = cr.KINDS[kind]
    group, raw = GroupAction.load(gname), cr.load(gname)
    for ops in (OPS, ("gs",), ("gt", "gs")):
        a = OutputAction.from_recipes(make_recipe(kind, 4).orbit(group, ops), True, [None] + list(ops))
        perm, sign = cr.output_action(raw, ops, nb)
        assert (a.perm, a.sign, a.width, a.n_units, a.row) == (perm, sign, 1, 6 * nb, 6 * nb) and a.operators == [None] + list(ops)
    if nb == 1:      # one copy: no permutation, the copy's reflection
        assert all(p == list(range(6)) for p in a.perm)
    else:
        assert a.perm[1 + ops.index("gs")] != list(range(6 * nb))      # (the C2 file's gt leaves the two base nodes in place)
    assert any(s < 0 for s in a.sign[1]) and any(s < 0 for s in a.sign[2])


def test_the_refusals_stay():
    k4 = GroupAction.load("solo-k4")
    plain = solo_com_recipe("k4_com", JP)
    assert plain.symmetry_parts is None and plain.label_slots is None and solo_com_mlp_recipe(JP).symmetry_parts is None
    with pytest.raises(ValueError, match="Solo"):
        plain.transformed("gs", k4)
    # duplicate label columns without slot tracking: still no permutation to read
    sym = make_recipe("k4").orbit(k4)
    with pytest.raises(ValueError, match="duplicate"):
        OutputAction.from_recipes([dataclasses.replace(r, label_slots=None) for r in sym], True)
    with pytest.raises(ValueError, match="duplicate"):
        OutputAction.from_recipes([dataclasses.replace(sym[0], label_slots=None)] + sym[1:], True)      # (every element must track them)
    # the compound label part: base nodes that do not match the group's, a permutation that tears a node triple apart
    with pytest.raises(ValueError, match="tables have"):
        make_recipe("k4").transformed("gs", GroupAction.load("solo-c2"))
    with pytest.raises(ValueError, match="base nodes"):      # (the variables fit the C2 tables, the labels of 4 base nodes do not)
        dataclasses.replace(make_recipe("c2"), label_cols=[0, 1, 2, 3, 4, 5] * 4, label_slots=list(range(24))).transformed("gs", GroupAction.load("solo-c2"))
    torn = GroupAction({**k4.permutation, "bs": [[1, 0, 2] + list(range(3, 12)), k4.permutation["bs"][1]]}, k4.reflection)
    with pytest.raises(ValueError, match="triples"):
        make_recipe("k4").transformed("gs", torn)
    with pytest.raises(ValueError, match="lin"):
        dataclasses.replace(make_recipe("k4"), label_cols=[0, 1, 2, 3, 4], label_slots=None).transformed("gs", k4)


# ---- the mirror of the per-segment sums ------------------------------------------------------------------------------------------------------------------
def _restated(y, y_pred, seg, n_seg, nb, mean, std):
    """gnnLightning_com.py:96-121 per segment in torch fp64: the states of its six metrics (MeanSquaredError: sum of squared errors and count; the cosine
    metric: sum of torch's cosine similarity of base node 0 after un-standardising, and the window count)."""
    y, y_pred = torch.as_tensor(y).double().view(-1, nb, 6), torch.as_tensor(y_pred).double().view(-1, nb, 6)
    mean, std = torch.as_tensor(mean).double(), torch.as_tensor(std).double()
    seg = np.asarray(seg)
    row = np.where((seg >= 0) & (seg < n_seg), seg, n_seg)
    state = torch.zeros(n_seg + 1, 8, dtype=torch.float64)
    for s in range(n_seg + 1):
        g = torch.from_numpy(np.nonzero(row == s)[0])
        if not g.numel():
            continue
        yy, pp = y[g], y_pred[g]
        state[s, 0], state[s, 2] = ((pp[:, :, :3].flatten() - yy[:, :, :3].flatten()) ** 2).sum(), pp[:, :, :3].numel()
        state[s, 1], state[s, 3] = ((pp[:, :, 3:].flatten() - yy[:, :, 3:].flatten()) ** 2).sum(), pp[:, :, 3:].numel()
        yu, pu = yy * std + mean, pp * std + mean
        cos = torch.nn.CosineSimilarity(dim=1)
        state[s, 4] = cos(pu[:, 0, :3].flatten(start_dim=1), yu[:, 0, :3].flatten(start_dim=1)).sum()
        state[s, 5] = cos(pu[:, 0, 3:].flatten(start_dim=1), yu[:, 0, 3:].flatten(start_dim=1)).sum()
        state[s, 6] = g.numel()
    return state.numpy()


@pytest.mark.parametrize("nb", [1, 2, 4])
def test_the_mirror_is_the_reference_metric_code_per_segment(nb):
    B, n_seg = 300, 5
    g = torch.Generator().manual_seed(40 + nb)
    y, yp = torch.randn(B, nb * 6, generator=g), torch.randn(B, nb * 6, generator=g)
    mean, std = torch.randn(6, generator=g).double(), torch.rand(6, generator=g).double() + 0.5
    seg = torch.randint(-1, n_seg + 1, (B,), generator=g).numpy().astype(np.int32)
    got = M.com_segmented_reference(y, yp, seg, n_seg, nb, mean, std)
    want = _restated(y, yp, seg, n_seg, nb, mean, std)
    assert got.shape == (n_seg + 1, 8) and np.array_equal(got[:, [2, 3, 6, 7]], want[:, [2, 3, 6, 7]]) and got[n_seg, 6] > 0
    assert (np.abs(got - want) <= 1e-12 * np.maximum(1.0, np.abs(want))).all(), np.abs(got - want).max()
    # the published values: the reference's MSE is the mean over all 6 nb values
    t = M.com_table_from_state(torch.from_numpy(got[:n_seg]))
    d = (yp.double() - y.double())
    for s in range(n_seg):
        m = torch.from_numpy(seg == s)
        assert abs(float(t["MSE"][s]) - float((d[m] ** 2).mean())) <= 1e-12
        assert float(t["avg_cos_sim"][s]) == (float(t["cos_sim_lin"][s]) + float(t["cos_sim_ang"][s])) / 2 and float(t["n"][s]) == int(m.sum())


def test_the_mirror_on_clamped_and_aligned_vectors():
    """Axis-aligned or zero vectors of base node 0: every cosine is -1, 0 or 1 exactly (a zero vector meets the 1e-8 clamp: 0 / 1e-8 = 0)."""
    y = np.zeros((4, 12), dtype=np.float32)
    yp = np.zeros((4, 12), dtype=np.float32)
    y[0, 0], yp[0, 0] = 2.0, 0.5          # lin: same axis, same sign -> 1
    y[1, 1], yp[1, 1] = 2.0, -0.25        # opposite -> -1
    y[2, 2], yp[2, 0] = 1.0, 1.0          # orthogonal -> 0
    y[3, 3] = 1.0                         # ang: prediction zero -> 0 (clamp)
    y[:, 6:] = 7.0                        # base node 1 never enters a cosine
    st = M.com_segmented_reference(y, yp, np.zeros(4, dtype=np.int32), 1, 2, np.zeros(6), np.ones(6))
    assert st[0, 4] == 1.0 - 1.0 + 0.0 + 0.0 and st[0, 5] == 0.0 and st[0, 6] == 4 and st[0, 2] == st[0, 3] == 3 * 2 * 4 and not st[1].any()
    assert st[0, 0] == math.fsum([1.5 ** 2, 2.25 ** 2, 1.0, 1.0] + [49.0] * 12) and st[0, 1] == 1.0 + 49.0 * 12
