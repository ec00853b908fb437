"""Host tests of the orbit-average mirror (tests/orbit_reference.py) and of `OutputAction`'s label-table rule.  No GPU.

1. The mirror obeys the contract's own statements (K = 1 keeps every bit, the backward is the exact transpose, an equivariant output has defect zero).
2. The case matrix of tests/test_orbit_average_gpu.py tells every damaged variant from the mirror: a kernel that uses perm where pinv belongs, drops a sign,
   adds in reverse element order or multiplies by 1 / K before the adds cannot pass the bit-for-bit comparison there.
3. `OutputAction.from_recipes` (the rule of `from_store`) reproduces `GroupAction.table("fs" | "ls", op)` for the A1 3-D, A1 1-D and MiniCheetah recipes
   and their MLP forms, and refuses what the contract says it refuses."""
import numpy as np
import pytest

from tests import orbit_reference as orb
from tests import test_window_symmetry as ws


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_one_element_reproduces_the_output_bit_for_bit():
    for (U, w) in orb.SHAPES:
        perm, sign, o, g = orb.case(17, 1, U, w)
        assert np.array_equal(_bits(orb.average(o, perm, sign, w, 17)), _bits(o))
        assert np.array_equal(_bits(orb.average_backward(g, perm, sign, w, 17)), _bits(g))
    assert bool((_bits(o) == 0x80000000).any()) and bool(((np.abs(o) < 1e-38) & (o != 0)).any())      # the data holds -0 and subnormals


@pytest.mark.parametrize("K", [1, 2, 4, 8])
def test_the_backward_is_the_exact_transpose_on_integer_data(K):
    """<avg(o), v> == <o, avg^T(v)> exactly in fp64: small integers and K a power of two make every operation exact."""
    rng = np.random.default_rng(K)
    for (U, w) in orb.SHAPES:
        B = 17
        perm, sign = orb.make_action(K, U)
        o = rng.integers(-64, 65, (K * B, U * w)).astype(np.float32)
        v = rng.integers(-64, 65, (B, U * w)).astype(np.float32)
        lhs = float((orb.average(o, perm, sign, w, B).astype(np.float64) * v).sum())
        rhs = float((o.astype(np.float64) * orb.average_backward(v, perm, sign, w, B)).sum())
        assert lhs == rhs and lhs != 0.0


def test_an_equivariant_output_has_defect_zero_and_is_its_own_average():
    perm, sign = orb.three_cycle_action()
    B, w = 17, 1
    o0 = orb.make_data(B, 6, 5)
    o = np.concatenate([orb.apply_action(o0, perm, sign, w, e) for e in range(3)])
    st = orb.defect(o, perm, sign, w, B)
    assert np.array_equal(st[:, 0], np.zeros(3)) and np.array_equal(st[:, 2], np.zeros(3)) and st[0, 1] > 0 and list(st[:, 3]) == [B * 6.0] * 3
    # every t_e is o_0 again: the average of integer-valued data is o_0 itself when 3 x divides exactly -- checked on a planted multiple of 3
    o0i = (3 * np.random.default_rng(2).integers(-20, 21, (B, 6))).astype(np.float32)
    oi = np.concatenate([orb.apply_action(o0i, perm, sign, w, e) for e in range(3)])
    assert np.abs(orb.average(oi, perm, sign, w, B) - o0i).max() <= 1e-5 * np.abs(o0i).max()


def test_a_planted_difference_gives_the_hand_computed_state():
    perm, sign = orb.three_cycle_action()
    B, w = 2, 1
    o0 = np.arange(1, 13, dtype=np.float32).reshape(B, 6)
    o = np.concatenate([orb.apply_action(o0, perm, sign, w, e) for e in range(3)])
    o[1 * B + 1, 2] += 0.5       # element 1, window 1, unit 2: comes back as unit perm[1][2] = 0 of window 1
    o[2 * B + 0, 4] -= 2.0       # element 2, window 0, unit 4
    st = orb.defect(o, perm, sign, w, B)
    s0 = float((o0.astype(np.float64) ** 2).sum())
    assert st.tolist() == [[0.0, s0, 0.0, 12.0], [0.25, s0, 0.5, 12.0], [4.0, s0, 2.0, 12.0]]
    st2 = orb.defect(o, perm, sign, w, B, st)      # a second call accumulates; the maximum stays
    assert st2.tolist() == [[0.0, 2 * s0, 0.0, 24.0], [0.5, 2 * s0, 0.5, 24.0], [8.0, 2 * s0, 2.0, 24.0]]


def test_the_gpu_cases_tell_every_damaged_variant_from_the_mirror():
    """Per variant: the cases of the GPU matrix in which its bits differ from the mirror's.  Every variant must be seen by some case; perm against pinv must be
    seen by the hand-built 3-cycle action (the real groups' involutions cannot see it)."""
    seen_fwd = {v: [] for v in orb.VARIANTS}
    seen_bwd = {v: [] for v in ("perm_for_pinv", "dropped_sign")}
    for (B, K, U, w) in orb.CASES:
        if B > 17:
            continue      # (the larger batches repeat the smaller ones' arithmetic on more rows)
        perm, sign, o, g = orb.case(B, K, U, w)
        ref, ref_b = orb.average(o, perm, sign, w, B), orb.average_backward(g, perm, sign, w, B)
        for v in seen_fwd:
            if not np.array_equal(_bits(orb.average(o, perm, sign, w, B, v)), _bits(ref)):
                seen_fwd[v].append((B, K, U, w))
        for v in seen_bwd:
            if not np.array_equal(_bits(orb.average_backward(g, perm, sign, w, B, v)), _bits(ref_b)):
                seen_bwd[v].append((B, K, U, w))
    for v, cases in list(seen_fwd.items()) + list(seen_bwd.items()):
        assert cases, v
    assert (17, 3, 6, 1) in seen_fwd["perm_for_pinv"] and (17, 3, 6, 1) in seen_bwd["perm_for_pinv"]
    for v in ("perm_for_pinv", "dropped_sign"):      # the quad-wide units (16-byte loads of a permuted unit on the device) are held to the same bits
        assert any(w == 4 for (_, _, _, w) in seen_fwd[v]) and any(w == 4 for (_, _, _, w) in seen_bwd[v]), v
    assert all(K > 2 for (_, K, _, _) in seen_fwd["reverse_order"])      # two terms commute: only K >= 3 can see the order
    # an involution cannot see perm against pinv: the A1 'fs' table under gs
    P, c = ws.A1.table("fs", "gs")
    perm, sign = [list(range(12)), list(P)], [[1] * 12, list(c)]
    o = orb.make_data(2 * 17, 12, 3)
    assert np.array_equal(_bits(orb.average(o, perm, sign, 1, 17, "perm_for_pinv")), _bits(orb.average(o, perm, sign, 1, 17)))


def _recipes():
    from morphsym_hgnn_amd.windows import (quadsdk_a1_c2_recipe, minicheetah_k4_recipe, quadsdk_a1_mlp_recipe, minicheetah_mlp_recipe)
    return [("a1-3d", quadsdk_a1_c2_recipe(ws.JP, ws.FP, ws.T, 3), ws.A1, "fs", True),
            ("a1-3d-body", quadsdk_a1_c2_recipe(ws.JP, ws.FP, ws.T, 3, body_frame_labels=True), ws.A1, "fs", True),
            ("a1-1d", quadsdk_a1_c2_recipe(ws.JP, ws.FP, ws.T, 1), ws.A1, "ls", True),
            ("mck4", minicheetah_k4_recipe(ws.JP, ws.FP, ws.T), ws.K4, "ls", False),
            ("a1-mlp", quadsdk_a1_mlp_recipe(ws.JP, ws.FP, ws.T, 3), ws.A1, "fs", True),
            ("mck4-mlp", minicheetah_mlp_recipe(ws.JP, ws.FP, ws.T), ws.K4, "ls", False)]


@pytest.mark.parametrize("mode", ws.MODES)
def test_the_label_table_rule_reproduces_the_groups_tables(mode):
    from morphsym_hgnn_amd.symmetrise import OutputAction
    for name, recipe, group, part, regression in _recipes():
        act = OutputAction.from_recipes(recipe.orbit(group, ws.OPS, mode), regression, [None] + list(ws.OPS))
        assert act.n_elements == 4 and act.width == (1 if regression else 2) and act.n_units == len(recipe.label_cols), name
        assert act.perm[0] == list(range(act.n_units)) and act.sign[0] == [1] * act.n_units
        for e, op in enumerate(ws.OPS, 1):
            P, c = group.table(part, op, mode)
            assert act.perm[e] == list(P) and act.sign[e] == [int(x) for x in c], (name, op)
            assert orb.inverse(act.perm[e]) == act.perm[e]      # (the real groups' label permutations are involutions)
        if part == "fs" and mode == "MorphSym":
            assert any(x < 0 for row in act.sign for x in row)


def test_what_the_rule_refuses():
    from morphsym_hgnn_amd.symmetrise import OutputAction
    from morphsym_hgnn_amd.windows import quadsdk_a1_c2_recipe, solo_com_recipe
    import dataclasses
    r = quadsdk_a1_c2_recipe(ws.JP, ws.FP, ws.T, 3)
    orbit = r.orbit(ws.A1)
    with pytest.raises(ValueError, match="one element"):
        OutputAction.from_recipes(orbit[:1], True)
    with pytest.raises(ValueError, match="identity=False"):
        OutputAction.from_recipes(r.orbit(ws.A1, identity=False), True, list(ws.OPS))
    with pytest.raises(ValueError, match="no labels"):
        OutputAction.from_recipes([dataclasses.replace(x, label_cols=[], label_signs=None) for x in orbit], True)
    with pytest.raises(ValueError, match="duplicate label columns"):
        solo = solo_com_recipe("k4_com", list(range(12)))
        OutputAction.from_recipes([solo, solo], True)
    with pytest.raises(ValueError, match="no sign to flip"):
        OutputAction.from_recipes(orbit, False)
    for perm, sign, width, msg in (([[0, 1], [1, 1]], [[1, 1], [1, 1]], 1, "not a permutation"), ([[0, 1], [1, 0]], [[1, 1], [1, 0]], 1, r"\+-1"),
                                   ([[1, 0], [0, 1]], [[1, 1], [1, 1]], 1, "identity"), ([[0, 1], [1, 0]], [[1, -1], [1, 1]], 1, "identity"),
                                   ([[0, 1]], [[1, 1]], 17, "width"), ([list(range(65))], [[1] * 65], 1, "n_units"),
                                   ([[0]] * 9, [[1]] * 9, 1, "elements")):
        with pytest.raises(ValueError, match=msg):
            OutputAction.from_tables(perm, sign, width)
