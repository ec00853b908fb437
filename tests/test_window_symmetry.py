"""Group-transformed windows (gs / gt / gr): `WindowRecipe.transformed` against the vectors the reference's own dataset classes produced with
`symmetry_operator` set (tools/gen_symmetry_window_golden.py -> tests/golden/windows_symmetry.npz), the group laws on the tables, and the refusals.
No GPU: a recipe is evaluated by the few lines of numpy below -- per run `sign * seq[series][start:start + T, col]`, labels likewise."""
import os

import numpy as np
import pytest

from oracle.gen_window_golden import synthetic_sequence, minicheetah_sequence, CASES
from morphsym_hgnn_amd.windows import GroupAction, WindowRecipe, quadsdk_a1_c2_recipe, minicheetah_k4_recipe, solo_com_recipe

FX = np.load(os.path.join(os.path.dirname(__file__), "golden", "windows_symmetry.npz"))
T, N = int(FX["T"]), int(FX["N"])
SEQ = synthetic_sequence(int(FX["seed_a1"]), N)
SEQ4 = minicheetah_sequence(int(FX["seed_k4"]), N)
JP, FP = FX["joint_perm"].astype(int), FX["foot_perm"].astype(int)
STARTS = [int(s) for s in FX["starts"]]
OPS, MODES = ("gs", "gt", "gr"), ("MorphSym", "Euclidean")
A1, K4 = GroupAction.load("a1-c2"), GroupAction.load("mini_cheetah-k4")


def evaluate(recipe: WindowRecipe, seq, start: int):
    """({type: [n, width]}, labels) of one window in fp64: the recipe's meaning, written out."""
    Tn, xs = recipe.history, {}
    col = lambda s, c: np.asarray(seq[s], dtype=np.float64).reshape(len(seq[s]), -1)[:, c]
    for t in recipe.node_types:
        rows = []
        for n in range(recipe.num_nodes[t]):
            runs = []
            for vi, (s, cols) in enumerate(recipe.variables.get(t, [])):
                for ai, c in enumerate(cols[n]):
                    r = (recipe.variable_signs[t][vi][n][ai] if recipe.variable_signs else 1) * col(s, c)[start:start + Tn]
                    if recipe.normalize:
                        with np.errstate(invalid="ignore", divide="ignore"):
                            r = np.nan_to_num((r - r.mean()) / r.std(ddof=1), nan=0.0, posinf=np.inf, neginf=-np.inf)
                    runs.append(r)
            rows.append(np.concatenate(runs) if runs else np.ones(1))
        xs[t] = np.stack(rows)
    row = start + Tn - 1
    y = np.array([col(recipe.label_series, c)[row] for c in recipe.label_cols])
    if recipe.label_rotate:      # world -> body with the closed-form matrix of the (x, y, z, w) quaternion of that row, per foot triple
        x, yq, z, s = np.asarray(seq[recipe.quat_series], dtype=np.float64)[row] / np.linalg.norm(np.asarray(seq[recipe.quat_series], dtype=np.float64)[row])
        R = np.array([[1 - 2 * (yq * yq + z * z), 2 * (x * yq - z * s), 2 * (x * z + yq * s)],
                      [2 * (x * yq + z * s), 1 - 2 * (x * x + z * z), 2 * (yq * z - x * s)],
                      [2 * (x * z - yq * s), 2 * (yq * z + x * s), 1 - 2 * (x * x + yq * yq)]])
        y = (y.reshape(-1, 3) @ R.T).reshape(-1)
    if recipe.label_signs is not None:
        y = y * np.asarray(recipe.label_signs, dtype=np.float64)
    return xs, y


def close(got, want, tol):
    return got.shape == want.shape and np.abs(got - want).max() <= tol * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_a1_transformed_recipe_reproduces_the_reference(case, op, mode):
    recipe = quadsdk_a1_c2_recipe(JP, FP, T, 3 if case["body"] else case["grf"], case["body"], case["norm"]).transformed(op, A1, mode)
    tol = 1e-12 if (case["body"] or case["norm"]) else 0.0      # exact, but for standardised values and the closed-form rotation (oracle/gen_window_golden.py)
    for st in STARTS:
        xs, y = evaluate(recipe, SEQ, st)
        key = f"a1:{case['name']}:{op}:{mode}:{st}"
        assert close(y, FX[key + ":y"], tol), key
        assert close(xs["base"][:, ::7], FX[key + ":base"], tol) and close(xs["joint"][:, ::11], FX[key + ":joint"], tol), key
        assert np.array_equal(xs["foot"], np.ones((4, 1)))
        if case["body"]:      # the quaternion by-product is not transformed
            assert np.array_equal(FX[key + ":r_o"], np.asarray(SEQ["r_o"])[st + T - 1])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("normalize", [False, True], ids=["plain", "norm"])
def test_k4_transformed_recipe_reproduces_the_reference(normalize, op, mode):
    recipe = minicheetah_k4_recipe(JP, FP, T, normalize).transformed(op, K4, mode)
    tol = 1e-12 if normalize else 0.0
    for st in STARTS:
        xs, y = evaluate(recipe, SEQ4, st)
        key = f"k4:{'norm' if normalize else 'plain'}:{op}:{mode}:{st}"
        assert close(y, FX[key + ":y"], 0.0), key
        for t, stride in (("base", 7), ("joint", 11), ("foot", 13)):
            assert close(xs[t][:, ::stride], FX[f"{key}:{t}"], tol), (key, t)


def test_the_fixture_is_not_the_identity():
    """(a transform that did nothing would not pass the tests above)"""
    plain, _ = evaluate(quadsdk_a1_c2_recipe(JP, FP, T), SEQ, 37)
    for op in OPS:
        assert not np.array_equal(plain["joint"][:, ::11], FX[f"a1:d3:{op}:MorphSym:37:joint"])
    assert not np.array_equal(FX["a1:d3:gs:MorphSym:37:base"], FX["a1:d3:gs:Euclidean:37:base"])


@pytest.mark.parametrize("group", [A1, K4], ids=["a1-c2", "mini_cheetah-k4"])
def test_group_laws_on_the_tables(group):
    for mode in MODES:
        for part in GroupAction.PARTS:
            (Ps, cs), (Pt, ct), (Pr, cr) = (group.table(part, op, mode) for op in OPS)
            n = len(Ps)
            compose = lambda A, B: ([B[0][A[0][k]] for k in range(n)], [A[1][k] * B[1][A[0][k]] for k in range(n)])      # first B, then A
            ident = (list(range(n)), [1] * n)
            assert compose((Ps, cs), (Ps, cs)) == ident and compose((Pt, ct), (Pt, ct)) == ident
            assert compose((Pt, ct), (Ps, cs)) == (Pr, cr) == compose((Ps, cs), (Pt, ct))
            if mode == "Euclidean":
                assert cs == ct == cr == [1] * n


@pytest.mark.parametrize("make,group", [(lambda: quadsdk_a1_c2_recipe(JP, FP, T, 3, True, True), A1), (lambda: quadsdk_a1_c2_recipe(JP, FP, T, 1), A1),
                                        (lambda: minicheetah_k4_recipe(JP, FP, T), K4)], ids=["a1-body-norm", "a1-d1", "k4"])
def test_transformed_composes(make, group):
    r = make()
    same = lambda a, b: (a.variables == b.variables and a.variable_signs == b.variable_signs and a.label_cols == b.label_cols and a.label_signs == b.label_signs)
    gs, gt, gr = (r.transformed(op, group) for op in OPS)
    assert same(gs.transformed("gt", group), gr) and same(gt.transformed("gs", group), gr)
    back = gs.transformed("gs", group)
    assert back.variables == r.variables and back.label_cols == r.label_cols
    assert all(x == 1 for t in back.variable_signs.values() for v in t for n in v for x in n) and all(x == 1 for x in back.label_signs)
    assert (gs.history, gs.normalize, gs.label_rotate, gs.quat_series, gs.symmetry_parts) == (r.history, r.normalize, r.label_rotate, r.quat_series, r.symmetry_parts)


def test_default_recipes_have_no_signs():
    for r in (quadsdk_a1_c2_recipe(JP, FP, T), minicheetah_k4_recipe(JP, FP, T), solo_com_recipe("k4_com", JP)):
        assert r.variable_signs is None and r.label_signs is None
    assert solo_com_recipe("c2_com", JP).symmetry_parts is None
    assert set(quadsdk_a1_c2_recipe(JP, FP, T).symmetry_parts) == {"imu_acc", "imu_omega", "q", "qd", "tau", "F"}
    assert quadsdk_a1_c2_recipe(JP, FP, T, 3).symmetry_parts["F"] == "fs" and quadsdk_a1_c2_recipe(JP, FP, T, 1).symmetry_parts["F"] == "ls"
    assert minicheetah_k4_recipe(JP, FP, T).symmetry_parts["contacts"] == "ls"


def test_group_action_load():
    assert GroupAction.load(os.path.join(os.path.dirname(__file__), "..", "morphsym_hgnn_amd", "cfg", "a1-c2.yaml")).permutation == A1.permutation
    assert len(A1.permutation["bs"][0]) == 6 and len(K4.permutation["bs"][0]) == 12
    with pytest.raises(ValueError):
        GroupAction.load("no-such-robot")


def test_refusals():
    r = quadsdk_a1_c2_recipe(JP, FP, T)
    with pytest.raises(ValueError, match="operator"):
        r.transformed("gx", A1)
    with pytest.raises(ValueError, match="mode"):
        r.transformed("gs", A1, mode="Affine")
    with pytest.raises(ValueError, match="Solo"):
        solo_com_recipe("k4_com", JP).transformed("gs", GroupAction.load("solo-k4"))
    import dataclasses
    with pytest.raises(ValueError, match="symmetry_parts"):
        dataclasses.replace(r, symmetry_parts=None).transformed("gs", A1)
    # body-frame labels rotate whole foot triples: a label permutation that tears one apart is refused
    bad = GroupAction({**A1.permutation, "fs": [[1, 0, 2] + list(range(3, 12)), A1.permutation["fs"][1]]}, A1.reflection)
    body = quadsdk_a1_c2_recipe(JP, FP, T, 3, body_frame_labels=True)
    with pytest.raises(ValueError, match="triples"):
        body.transformed("gs", bad)
    body.transformed("gs", A1)
    dataclasses.replace(body, label_rotate=False, variables={**body.variables}).transformed("gt", bad)      # (gt's row is intact)
    with pytest.raises(ValueError, match="tables have"):      # the K4 base tables are 12 wide, the C2 recipe's base has 6 columns
        r.transformed("gs", K4)
