"""tests/window_reference.py on the host (no GPU): (1) the table-reading reference agrees with the two host evaluators the suite already has --
oracle/window_oracle.py (pinned to the reference's own dataset functions by tests/golden/windows_*.npz) and `evaluate` of tests/test_window_symmetry.py
(pinned by tests/golden/windows_symmetry.npz) -- at the tolerances those files use; (2) controls for every case family of
tests/test_windows_exact_gpu.py: an fp64 emulation of the kernels' arithmetic followed by one fp32 rounding passes the checker on both output dtypes,
and every mutation of the list in the issue is rejected on that family's own descriptors."""
import numpy as np
import pytest

from oracle import window_oracle as wo
from morphsym_hgnn_amd.windows import quadsdk_a1_c2_recipe, minicheetah_k4_recipe, solo_com_recipe, solo_com_arrays, stack_orbit_tables
from tests import window_reference as wr
from tests import test_windows as tw
from tests import test_window_symmetry as ts


def _reference_of(recipe, seq, starts, elements=None, orbit=None):
    names = recipe.series()
    tables = stack_orbit_tables([r.tables(names)[:3] for r in orbit]) if orbit else None
    tab = wr.recipe_tables(recipe, names, "f32", lambda t: recipe.width(t) + 3, tables)
    series = [wr.f32(seq[s]).reshape(len(seq[s]), -1) for s in names]
    st = list(starts) if elements is None else [(e << wr.ELEMENT_SHIFT) | s for s, e in zip(starts, elements)]
    exp = wr.reference(tab, series, st)
    for t, name in enumerate(recipe.node_types):      # every feature column is covered, every pad column is not
        assert exp.covered[t][:, :, :recipe.width(name)].all() and not exp.covered[t][:, :, recipe.width(name):].any()
    return exp


def _close(got, want, tol):
    return got.shape == want.shape and np.abs(got - want).max() <= tol * max(1.0, np.abs(want).max())


# ---- 1. the reference against the host evaluators -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", tw.CASES, ids=[c["name"] for c in tw.CASES])
def test_reference_agrees_with_the_a1_oracle(case):
    T = tw.T
    recipe = quadsdk_a1_c2_recipe(tw.JP, tw.FP, T, case["grf"], case["body"], case["norm"])
    starts = [0, 37, tw.N - T]
    exp = _reference_of(recipe, tw.SEQ, starts)
    tol = 1e-12 if (case["body"] or case["norm"]) else 0.0      # (tests/test_windows.py: the oracle against the fixture)
    for b, st in enumerate(starts):
        base, joint, foot, y, q = wo.a1_c2_window(tw.SEQ, st, T, tw.JP, tw.FP, case["grf"], case["body"], case["norm"])
        for t, want in enumerate((base, joint, foot)):
            assert _close(exp.x[t][b][:, :want.shape[1]], want, tol), (st, t)
        assert _close(exp.y[b], y, tol) and np.array_equal(exp.quat[b].astype(np.float64), q)
        if case["norm"]:
            assert max(e.max() for e in exp.bound) < 2.0 ** -40      # integer / 64 data: the derived bound is far below an fp32 ulp


@pytest.mark.parametrize("normalize", [False, True], ids=["plain", "norm"])
def test_reference_agrees_with_the_minicheetah_oracle(normalize):
    T = tw.T
    recipe = minicheetah_k4_recipe(tw.JP, tw.FP, T, normalize)
    starts = [0, 99, int(tw.FX4["N"]) - T]
    exp = _reference_of(recipe, tw.SEQ4, starts)
    for b, st in enumerate(starts):
        want = wo.minicheetah_k4_window(tw.SEQ4, st, T, tw.JP, tw.FP, normalize)
        for t in range(3):
            assert _close(exp.x[t][b][:, :want[t].shape[1]], want[t], 1e-12 if normalize else 0.0), (st, t)
        assert np.array_equal(exp.y[b], want[3]) and exp.quat is None


@pytest.mark.parametrize("history", [1, 5])
@pytest.mark.parametrize("kind", list(tw.SOLO_KINDS))
def test_reference_agrees_with_the_solo_oracle(kind, history):
    nb = tw.SOLO_KINDS[kind][1]
    starts = [0, 17, int(tw.FXS["N"]) - history]
    exp = _reference_of(solo_com_recipe(kind, tw.JP, history), solo_com_arrays(tw.SEQS["X"], tw.SEQS["Y"]), starts)
    for b, st in enumerate(starts):
        base, joint, y = wo.solo_com_window(tw.SEQS["X"], tw.SEQS["Y"], st, history, tw.JP, nb)
        assert np.array_equal(exp.x[0][b][:, :base.shape[1]], base) and np.array_equal(exp.x[1][b][:, :joint.shape[1]], joint) and np.array_equal(exp.y[b], y)


@pytest.mark.parametrize("normalize", [False, True], ids=["plain", "norm"])
def test_reference_agrees_with_the_recipe_evaluator_on_a_transformed_sibling(normalize):
    recipe = quadsdk_a1_c2_recipe(ts.JP, ts.FP, ts.T, 3, True, normalize).transformed("gr", ts.A1)
    exp = _reference_of(recipe, ts.SEQ, ts.STARTS)
    for b, st in enumerate(ts.STARTS):
        xs, y = ts.evaluate(recipe, ts.SEQ, st)
        for t, name in enumerate(recipe.node_types):
            assert _close(exp.x[t][b][:, :xs[name].shape[1]], xs[name], 1e-12), (st, name)
        assert _close(exp.y[b], y, 1e-12)


def test_reference_agrees_with_the_recipe_evaluator_on_an_orbit():
    recipe = minicheetah_k4_recipe(ts.JP, ts.FP, ts.T, True)
    orbit = recipe.orbit(ts.K4)
    elements = [(3 * i + 1) % len(orbit) for i in range(len(ts.STARTS))]
    exp = _reference_of(recipe, ts.SEQ4, ts.STARTS, elements, orbit)
    assert len(set(elements)) > 1
    for b, (st, e) in enumerate(zip(ts.STARTS, elements)):
        xs, y = ts.evaluate(orbit[e], ts.SEQ4, st)
        for t, name in enumerate(recipe.node_types):
            assert _close(exp.x[t][b][:, :xs[name].shape[1]], xs[name], 1e-12), (st, e, name)
        assert _close(exp.y[b], y, 0.0)


# ---- 2. controls: one per case family of tests/test_windows_exact_gpu.py ------------------------------------------------------------------------------
COPY = ["start+1", "drop-last", "swap-runs", "feature-late", "neighbour-column", "uncovered-overwritten"]


def _orbit_general():
    tab, series = wr.general_case([1, 7, 8, 9], 5, signed=True, K=2)
    return tab, series, wr.starts_for(tab, series, 5, elements=[0, 1, 2, 255, 1])


def _orbit_labels():
    tab, series = wr.label_case(12, True, K=2)
    return tab, series, wr.starts_for(tab, series, 12, elements=[0, 1, 2, 255])


def _plain(builder, B=5, chunk=0):
    def make():
        tab, series = builder()
        return tab, series, wr.starts_for(tab, series, B)
    make.chunk = chunk
    return make


FAMILIES = {
    # family: (case, chunk elements of the chunk kernel per dtype or None, the mutations this family must reject)
    "run-by-run/lengths": (_plain(lambda: wr.lengths_case(signed=True)), None, COPY[:2] + COPY[3:]),
    "run-by-run/rows-of-runs": (_plain(lambda: wr.general_case([1, 7, 8, 9, 16, 17], 3, signed=True)), None, COPY),
    "run-by-run/128-runs-65-rows": (_plain(lambda: wr.general_case([1] * 63 + [64, 1], 4), B=2), None, COPY),
    "run-by-run/orbit": (_orbit_general, None, COPY + ["element-not-clamped"]),
    "chunk/history-7": (None, {"f32": 4, "bf16": 8}, COPY[:3] + ["neighbour-column", "sign-dropped-in-chunk", "pad-outside-last-chunk", "uncovered-overwritten"]),
    "chunk/history-9": (None, {"f32": 4, "bf16": 8}, ["sign-dropped-in-chunk", "pad-outside-last-chunk"]),
    "standardise/all-kinds": (_plain(wr.standardise_case), None, COPY + ["sign-after-stats", "ddof0", "constant-nan", "ones-standardised"]),
    # the mutations below on exactly the runs that the issue names for them: a negated constant run (only the sign of the zero shows, see window_reference),
    # the offset-1e6 run (the bound itself must reject an fp32-formed mean: no exact element is in this descriptor)
    "standardise/negated-constant": (_plain(lambda: wr.standardise_case([wr.SIGN_FLAG | 1])), None, ["sign-after-stats", "constant-nan"]),
    "standardise/offset-1e6": (_plain(lambda: wr.standardise_case([2, wr.SIGN_FLAG | 2])), None, ["mean-fp32", "ddof0", "start+1"]),
    "standardise/random": (_plain(lambda: wr.standardise_case([0, 7])), None, ["ddof0", "neighbour-column", "swap-runs"]),
    "labels/unrotated": (_plain(lambda: wr.label_case(25, False, signed=True), B=12), None, ["label-first-row", "start+1"]),
    "labels/rotated": (_plain(lambda: wr.label_case(27, True, signed=True), B=12), None,
                       ["label-first-row", "R-transposed", "quat-not-normalised", "label-negated-before-rotation"]),
    "labels/orbit": (_orbit_labels, None, ["element-not-clamped", "R-transposed", "label-negated-before-rotation"]),
}


def _family(name, dtype):
    make, chunks, muts = FAMILIES[name]
    if make is None:      # the chunk kernel's descriptors depend on the elements of a 16-byte chunk
        chunk = chunks[dtype]
        hist = int(name.rsplit("-", 1)[1])
        tab, series = wr.general_case([9, 1, 8, 3], 6, n_types=3, signed=True, fast_layout=True, history=hist, chunk=chunk, const_rows=2)
        return tab, series, wr.starts_for(tab, series, 5), chunk, muts
    tab, series, starts = make()
    return tab, series, starts, 0, muts


CONTROLS = [(f, m) for f, (_, _, muts) in FAMILIES.items() for m in [None] + muts]


def test_every_mutation_of_the_list_is_exercised():
    assert {m for _, m in CONTROLS if m} == set(wr.MUTATIONS)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("family,mutation", CONTROLS, ids=[f"{f}:{m or 'emulation-passes'}" for f, m in CONTROLS])
def test_control(family, mutation, dtype):
    """family = the GPU case family guarded, mutation = what the kernel is imagined to get wrong (None: nothing -- the emulation must pass)."""
    tab, series, starts, chunk, _ = _family(family, dtype)
    exp = wr.reference(tab, series, starts, chunk)
    xs, y, q = wr.emulate(tab, series, starts, dtype, chunk, mutation)
    verdict = wr.check(tab, exp, xs, y, q, starts)
    if mutation is None:
        assert verdict is None, verdict
    else:
        assert verdict is not None, f"{family}: the checker accepts '{mutation}'"


def test_checkers_on_special_values():
    import torch
    want = np.array([0.0, -0.0, np.nan, 3.4028235e38, 1e-45, 1.0])
    ok = torch.tensor([0.0, -0.0, float("nan"), 3.4028235e38, 1e-45, 1.0])
    assert wr.first_mismatch(ok, want) is None and wr.first_mismatch(ok.to(torch.bfloat16), want) is None
    assert torch.isinf(ok.to(torch.bfloat16)[3])                                   # the largest fp32 is infinity on bf16: torch's cast is the expectation
    assert wr.first_mismatch(torch.tensor([-0.0, -0.0, float("nan"), 3.4028235e38, 1e-45, 1.0]), want) == (0,)      # the sign of a zero counts
    assert wr.first_mismatch(-ok, want) == (0,) and wr.first_mismatch(torch.flip(ok, [0]), want) is not None
    # fp64 -> bf16 in one step differs from fp64 -> fp32 -> bf16 where the fp32 rounding lands on a bf16 tie: the checker wants the two-step bits
    v = 1.0 + 2.0 ** -8 + 2.0 ** -30
    assert wr.first_mismatch(torch.tensor([1.0], dtype=torch.bfloat16), np.array([v])) is None
    assert wr.first_mismatch(torch.tensor([1.0 + 2.0 ** -7], dtype=torch.bfloat16), np.array([v])) == (0,)
    # the interval: outward-rounded fp32 ends, bf16 roundings of them
    w, e = np.array([1.0 + 2.0 ** -30]), np.array([2.0 ** -40])
    assert wr.within_bound(torch.tensor([1.0]), w, e) is None and wr.within_bound(torch.tensor([1.0 + 2.0 ** -23]), w, e) is None
    assert wr.within_bound(torch.tensor([1.0 - 2.0 ** -24]), w, e) == (0,) and wr.within_bound(torch.tensor([1.0 + 2.0 ** -22]), w, e) == (0,)
    assert wr.within_bound(torch.tensor([float("nan")]), w, e) == (0,)
    assert wr.within_bound(torch.tensor([1.0], dtype=torch.bfloat16), w, e) is None and wr.within_bound(torch.tensor([1.0078125], dtype=torch.bfloat16), w, e) == (0,)


def test_the_bound_refuses_data_it_cannot_judge():
    with pytest.raises(ValueError, match="infinities"):
        wr.standardise_exact(np.array([1.0, np.inf], dtype=np.float32))
    # (fp32 data cannot reach the other refusal: max |x| / sd <= 2^24 sqrt(n) there, rs stays below 1e-6)
    x = np.full(256, 1e20, dtype=np.float32); x[3] = np.nextafter(np.float32(1e20), np.float32(np.inf))
    assert wr.standardise_exact(x)[1].max() < 1e-4
