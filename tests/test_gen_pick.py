"""Which kernel a launch of the generic-width engine gets: pick_job_kernel / pick_gradw_kernel of mshgnn_gen_plan.hpp, driven on the CPU through
libmshgnn_hostplan.so (as tests/test_plan_property.py drives the plan compilers).  mshgnn_gen.hip launches row `kernel` of its table with the pick's grid,
tiles and (job, tile) pair count and nothing else, so what is asserted here is what runs: the cases the GPU tests' docstrings state (tests/test_widths_gpu.py,
tests/test_generic_gpu.py), the forced modes of MSHGNN_GEN_TILE, and invariants over the whole query space.

A kernel's name carries its template arguments: k_gstep<SPLIT, MB, NW> and k_gstep4<SPLIT, MB, NW> work on tiles of 16 MB windows with NW waves, a workgroup
covering NW / 4 column tiles of 128; k_gstep5<SPLIT, MB, MASKED, NW, RAW> the same with NW / 2 column tiles per workgroup (each wave owns two 32-column slices of
the 16 NW).  The grid invariant below uses those column tiles: n_jobs . tiles . NCT / column tiles, which for k_gstep and k_gstep4 is NCT / (nw / 4)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "morphsym_hgnn_amd", "csrc")
GS5_MAX_TERMS, GS5_MB_SPLIT = 16, 6
N_CU = 256      # MI355X
FIELDS = ("forced", "split", "NCT", "n_jobs", "all_raw", "all_plain", "any_mask", "max_terms", "B", "n_cu", "raw_ok")
# the query space (the one the pick was compared with the ladder it replaced on)
SPACE = dict(forced=(-1, 0, 1, 2, 3, 6, 8, 9), split=(0, 1), NCT=(1, 2, 3, 4, 5, 6, 7, 8, 12, 16), n_jobs=(1, 16, 32, 48, 300), all_raw=(0, 1), all_plain=(0, 1),
             any_mask=(0, 1), max_terms=(1, 16, 17), B=(1, 16, 63, 64, 65, 96, 97, 127, 128, 129, 255, 256, 257, 300, 1100, 8192), n_cu=(64, 256, 304), raw_ok=(0, 1))
# every kernel some query reaches with MSHGNN_GEN_TILE unset; the others (k_gstep on 128-window tiles, the split k_gstep at 16 waves) only run forced
UNFORCED = {"k_gstep<false,4,4>", "k_gstep<false,4,8>", "k_gstep<false,4,16>", "k_gstep<true,4,4>", "k_gstep<true,4,8>", "k_gstep4<false,8,16>", "k_gstep4<true,4,16>",
            "k_gstep5<false,8,false,8,false>", "k_gstep5<false,8,true,8,false>", "k_gstep5<false,8,false,4,false>", "k_gstep5<false,8,true,4,false>",
            "k_gstep5<true,GS5_MB_SPLIT,false,8,false>", "k_gstep5<true,GS5_MB_SPLIT,true,8,false>", "k_gstep5<false,8,false,8,true>", "k_gstep5<false,8,false,4,true>"}
FORCED_ONLY = {"k_gstep<false,8,8>", "k_gstep<true,8,8>", "k_gstep<true,4,16>"}


@pytest.fixture(scope="module")
def lib():
    path = os.path.join(ROOT, "morphsym_hgnn_amd", "libmshgnn_hostplan.so")
    subprocess.run(["make", "-C", CSRC, "../libmshgnn_hostplan.so"], check=True, capture_output=True)
    lib = C.CDLL(path)
    lib.mshgnn_hostplan_gen_pick.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    lib.mshgnn_hostplan_gen_pick.restype = None
    lib.mshgnn_hostplan_gen_kernel_name.restype = C.c_char_p
    lib.mshgnn_hostplan_gen_tile_mode.argtypes = [C.c_char_p]
    return lib


@pytest.fixture(scope="module")
def kernels(lib):
    """Per kernel index: (name, family, split, MB, NW, MASKED or None, RAW), read off the name."""
    out = []
    for k in range(lib.mshgnn_hostplan_gen_kernel_count()):
        name = lib.mshgnn_hostplan_gen_kernel_name(k).decode()
        fam, args = re.fullmatch(r"(k_gstep[45]?)<(.*)>", name).groups()
        a = [GS5_MB_SPLIT if x == "GS5_MB_SPLIT" else {"false": 0, "true": 1}.get(x, x) for x in args.split(",")]
        if fam == "k_gstep5": out.append((name, fam, a[0], int(a[1]), int(a[3]), a[2], a[4]))
        else: out.append((name, fam, a[0], int(a[1]), int(a[2]), None, 0))
    assert len({o[0] for o in out}) == len(out)
    return out


def _pick(lib, queries):
    q = np.ascontiguousarray(queries, dtype=np.int32).reshape(-1, len(FIELDS))
    p = np.zeros((q.shape[0], 6), dtype=np.int32)
    lib.mshgnn_hostplan_gen_pick(q.ctypes.data, p.ctypes.data, q.shape[0])
    return p


def _one(lib, kernels, **kw):
    """(kernel name, waves) of one query; unnamed fields: mode unset, bf16, one plain unmasked job, raw_ok, 256 CUs."""
    q = dict(forced=-1, split=0, NCT=4, n_jobs=1, all_raw=0, all_plain=0, any_mask=0, max_terms=1, B=300, n_cu=N_CU, raw_ok=1)
    assert set(kw) <= set(q)
    q.update(kw)
    p = _pick(lib, [[q[f] for f in FIELDS]])[0]
    return kernels[p[0]][0], int(p[1])


def test_the_wave_switch_of_the_pipelined_kernel(lib, kernels):
    """hidden 512 (NCT 4) on the 16-limb robot, bf16: a 48-job raw-input launch, a 32-job first layer, a 16-job last layer (forward unmasked, backward masked).
    256 windows (2 tiles of 128): at most 96 (job, tile) pairs on 256 CUs, every launch k_gstep5 at 8 waves.  1100 windows (9 tiles): 432 and 288 pairs switch
    to 4 waves, 144 stay at 8."""
    for B, raw48, l32, l16 in ((256, 8, 8, 8), (1100, 4, 4, 8)):
        assert _one(lib, kernels, B=B, n_jobs=48, all_raw=1) == (f"k_gstep5<false,8,false,{raw48},true>", raw48)
        for mask in (0, 1):
            m = "true" if mask else "false"
            assert _one(lib, kernels, B=B, n_jobs=32, all_plain=1, any_mask=mask) == (f"k_gstep5<false,8,{m},{l32},false>", l32)
            assert _one(lib, kernels, B=B, n_jobs=16, all_plain=1, any_mask=mask) == (f"k_gstep5<false,8,{m},{l16},false>", l16)
            # the split plan has the 8-wave form only, at both batches
            for n_jobs in (32, 16):
                assert _one(lib, kernels, split=1, B=B, n_jobs=n_jobs, all_plain=1, any_mask=mask) == (f"k_gstep5<true,GS5_MB_SPLIT,{m},8,false>", 8)


def test_launches_the_pipelined_kernel_does_not_take(lib, kernels):
    # hidden 768 (NCT 6) with input tensors k_gstep5<RAW> cannot read (the dense-input fallback): the raw launch goes to k_gstep at 8 waves, at NCT 4 to k_gstep4
    assert _one(lib, kernels, NCT=6, B=1100, n_jobs=48, all_raw=1, raw_ok=0) == ("k_gstep<false,4,8>", 8)
    assert _one(lib, kernels, NCT=6, B=1100, n_jobs=48, all_raw=1, raw_ok=1) == ("k_gstep5<false,8,false,4,true>", 4)      # (a multiple of 256, not of 512: 4 waves only)
    assert _one(lib, kernels, NCT=4, B=1100, n_jobs=48, all_raw=1, raw_ok=0) == ("k_gstep4<false,8,16>", 16)
    # bf16 under 256 windows: the widest k_gstep the NCT allows, whatever the launch holds
    for nct, nw in ((1, 4), (2, 8), (3, 4), (4, 16), (6, 8), (8, 16)):
        for kw in (dict(all_plain=1), dict(all_raw=1), dict()):
            assert _one(lib, kernels, NCT=nct, B=255, n_jobs=32, **kw) == (f"k_gstep<false,4,{nw}>", nw)
    # split arithmetic at hidden % 512 != 0: k_gstep at 8 or 4 waves, at every batch
    for nct, nw in ((1, 4), (2, 8), (3, 4), (6, 8)):
        for B in (70, 300, 1100):
            assert _one(lib, kernels, split=1, NCT=nct, B=B, n_jobs=32, all_plain=1) == (f"k_gstep<true,4,{nw}>", nw)
    # more terms than k_gstep5's table holds, or terms that are not one plain row: k_gstep4 (NCT % 4 == 0)
    assert _one(lib, kernels, B=300, all_plain=1, max_terms=GS5_MAX_TERMS + 1) == ("k_gstep4<false,8,16>", 16)
    assert _one(lib, kernels, B=300, all_plain=1, max_terms=GS5_MAX_TERMS) == ("k_gstep5<false,8,false,8,false>", 8)
    assert _one(lib, kernels, split=1, B=300) == ("k_gstep4<true,4,16>", 16)


@pytest.mark.parametrize("split", [0, 1])
def test_forced_modes(lib, kernels, split):
    """MSHGNN_GEN_TILE at an odd (3, hidden 384) and an even (4, hidden 512) NCT on 300 windows, the table of tests/test_widths_gpu.py
    (test_forced_tile_modes_match_the_oracle) and of tests/test_exact_generic_gpu.py (test_forced_mode_is_the_oracle_bit_for_bit): plain launches, masked or not, and
    the raw-input launch."""
    s = "true" if split else "false"
    for kw in (dict(all_plain=1), dict(all_plain=1, any_mask=1), dict(all_raw=1)):
        plain, m = "all_plain" in kw, "true" if kw.get("any_mask") else "false"
        for mode in (0, 1, 2, 3, 6, 8, 9):      # NCT 3: one column tile per workgroup is all that divides it
            assert _one(lib, kernels, forced=mode, split=split, NCT=3, **kw) == (f"k_gstep<{s},4,4>", 4)
        assert _one(lib, kernels, forced=0, split=split, **kw) == (f"k_gstep<{s},4,4>", 4)
        assert _one(lib, kernels, forced=1, split=split, **kw) == (f"k_gstep<{s},8,8>", 8)
        assert _one(lib, kernels, forced=2, split=split, **kw) == (f"k_gstep<{s},4,8>", 8)
        assert _one(lib, kernels, forced=3, split=split, **kw) == (f"k_gstep<{s},4,16>", 16)
        k4 = ("k_gstep4<true,4,16>", 16) if split else ("k_gstep4<false,8,16>", 16)
        assert _one(lib, kernels, forced=6, split=split, **kw) == k4
        if split:      # one k_gstep5 form, plain launches only
            for mode in (8, 9):
                assert _one(lib, kernels, forced=mode, split=1, **kw) == ((f"k_gstep5<true,GS5_MB_SPLIT,{m},8,false>", 8) if plain else k4)
        else:
            assert _one(lib, kernels, forced=8, **kw) == ((f"k_gstep5<false,8,{m},8,false>", 8) if plain else ("k_gstep5<false,8,false,8,true>", 8))
            assert _one(lib, kernels, forced=9, **kw) == ((f"k_gstep5<false,8,{m},4,false>", 4) if plain else ("k_gstep5<false,8,false,4,true>", 4))
            # forced, the (job, tile) pair count does not switch the wave count
            assert _one(lib, kernels, forced=8, B=8192, n_jobs=300, **kw)[1] == 8 and _one(lib, kernels, forced=9, B=1, **kw)[1] == 4


def test_only_the_documented_values_of_the_variable_force_a_mode(lib):
    for v in (0, 1, 2, 3, 6, 8, 9):
        assert lib.mshgnn_hostplan_gen_tile_mode(str(v).encode()) == v
    for text in (None, b"", b"4", b"5", b"7", b"10", b"-1", b"08", b" 8", b"8 ", b"8x", b"x", b"3.5"):
        assert lib.mshgnn_hostplan_gen_tile_mode(text) == -1, text


def test_invariants_over_the_query_space(lib, kernels):
    """Every pick of the space is launchable and is what its kernel decodes.  On the k_gstep5 rule: the plain forms need all_plain and at most GS5_MAX_TERMS terms;
    the RAW forms need all_raw, which the plan compiler only sets on launches whose jobs have at most 16 terms (compile_gen_plan) -- max_terms is the plain
    launches' figure and the raw rule never read it."""
    grids = np.meshgrid(*[np.array(SPACE[f], dtype=np.int32) for f in FIELDS], indexing="ij")
    q = np.stack([g.reshape(-1) for g in grids], axis=1)
    assert q.shape[0] == 1843200
    p = _pick(lib, q)
    Q = {f: q[:, i].astype(np.int64) for i, f in enumerate(FIELDS)}
    k, nw, tw, tiles, njt = (p[:, i].astype(np.int64) for i in range(5))
    grid = p[:, 5].astype(np.int64) & 0xffffffff
    assert k.min() >= 0 and k.max() < len(kernels)
    col = lambda i: np.array([kr[i] for kr in kernels], dtype=object)[k]
    fam = col(1)
    k_split, k_mb, k_nw, k_raw = (col(i).astype(np.int64) for i in (2, 3, 4, 6))
    gs5 = fam == "k_gstep5"
    has_mask = np.array([kr[5] is not None and not kr[6] for kr in kernels])[k]
    k_masked = np.array([int(kr[5] or 0) for kr in kernels])[k]
    # the pick's numbers are its kernel's template arguments
    assert np.array_equal(nw, k_nw) and np.array_equal(tw, 16 * k_mb) and np.array_equal(k_split, Q["split"])
    assert np.all(nw % 4 == 0) and np.all(Q["NCT"] % (nw // 4) == 0)
    assert np.all(64 * nw <= 1024)
    assert np.all((tiles - 1) * tw < Q["B"]) and np.all(Q["B"] <= tiles * tw)
    col_tiles = np.where(gs5, nw // 2, nw // 4)
    assert np.all(Q["NCT"] % col_tiles == 0)
    pairs = Q["n_jobs"] * tiles
    by_pairs = gs5 & (nw == 4)      # decoded from (job, tile) pairs in groups of 8
    assert np.array_equal(grid, np.where(by_pairs, (pairs + 7) // 8 * 8, pairs) * (Q["NCT"] // col_tiles))
    assert np.array_equal(njt[by_pairs], pairs[by_pairs]) and np.all((njt == 0) | (njt == pairs))
    assert np.all(~(k_raw == 1) | ((Q["all_raw"] == 1) & (Q["raw_ok"] == 1) & (Q["split"] == 0)))
    plain5 = gs5 & (k_raw == 0)
    assert np.all(~plain5 | ((Q["all_plain"] == 1) & (Q["max_terms"] <= GS5_MAX_TERMS)))
    assert np.all(~gs5 | (Q["all_plain"] == 1) | (Q["all_raw"] == 1))
    assert np.array_equal(k_masked[has_mask], Q["any_mask"][has_mask]) and has_mask.sum() == plain5.sum()
    # reachability
    names = np.array([kr[0] for kr in kernels])
    assert set(names[np.unique(k)]) == set(names) == UNFORCED | FORCED_ONLY
    assert set(names[np.unique(k[Q["forced"] < 0])]) == UNFORCED


def test_the_bit_exact_matrix_reaches_every_kernel_the_library_dispatches(lib, kernels):
    """tests/test_exact_generic_gpu.py meets the oracle bit for bit on the (arithmetic, NCT, batch, MSHGNN_GEN_TILE) of its matrix; here: the kernels those
    queries pick.  A launch's job count and plain / raw flags are the plan's (not visible from Python), so each query is asked for the launch classes this
    model class has -- the raw-input launch (the encoder, padded rows: raw_ok), launches of plain rows, launches with a term of several sources -- at 1, 16
    and 32 jobs (the 8-limb model has 33 nodes) and up to 16 terms, and the union is asserted.  Reached: every kernel of UNFORCED | FORCED_ONLY except
      * the three MASKED k_gstep5 forms: a launch takes one only when a source of its jobs carries relu bits (any_mask), which no plan of the product
        library has -- the producer of dX writes the masked row (GenPlan::dhm; MSHGNN_GEN_DHM=0 exists only under -DMSHGNN_TUNING).
    k_gstep4<false,8,16> is reached by MSHGNN_GEN_TILE=6, not by a launch of more than GS5_MAX_TERMS terms: a job has one term for its root weights and one
    per relation into its node (two where a sum of two rows is split), 7 at most on the MI graph, whatever the in-degree -- many rows are ONE term of many
    sources or one aggregate row.  That fallback stays on this file's own query (test_launches_the_pipelined_kernel_does_not_take)."""
    from tests import test_exact_gpu as gx
    from tests import test_exact_generic_gpu as gen
    points = {(m, B, -1) for m, B in gen.DEFAULT_CASES + gen.RANDOM_CASES + gen.MEAN_CASES} | {(gen.THRESHOLD_MODEL, B, -1) for B in gen.THRESHOLD_BATCHES}
    points |= {(m, B, int(mode)) for m, B, mode in gen.FORCED_CASES} | {(m, B, -1) for m, B, _, _ in gen.AGGREGATE_CASES + gen.MANY_ROW_CASES}
    nct = {m: gx._spec(m).hidden // 128 for m in {p[0] for p in points}}
    seen, by_point = set(), {}
    for m, B, forced in sorted(points):
        for split in (0, 1):
            for kw in (dict(all_raw=1), dict(all_plain=1), dict()):
                for n_jobs in (1, 16, 32):
                    for max_terms in (1, 16):
                        name, _ = _one(lib, kernels, forced=forced, split=split, NCT=nct[m], B=B, n_jobs=n_jobs, max_terms=max_terms, **kw)
                        seen.add(name)
                        by_point.setdefault(name, (m, B, forced, split, kw))
    masked = {k for k in UNFORCED if re.fullmatch(r"k_gstep5<[^,]+,[^,]+,true,.*", k)}
    assert len(masked) == 3
    assert seen == (UNFORCED | FORCED_ONLY) - masked, ((UNFORCED | FORCED_ONLY) - masked - seen, seen & masked)
    print("\n" + "\n".join(f"{k}: first reached by {v}" for k, v in sorted(by_point.items())))


def test_weight_gradient_pick(lib):
    # GGradwKernel: BF16_OS1, BF16_OS2, X3_OS1, X3_OS2, then the four NOMASK forms (plans with dhm: no P operand carries relu bits)
    seen = {(split, os_, dhm): lib.mshgnn_hostplan_gen_gradw_pick(split, os_, dhm) for split in (0, 1) for os_ in (1, 2) for dhm in (0, 1)}
    assert sorted(seen.values()) == list(range(8))
    assert seen[(0, 1, 0)] == 0 and seen[(0, 2, 0)] == 1 and seen[(1, 1, 0)] == 2 and seen[(1, 2, 0)] == 3
    assert all(seen[(s, o, 1)] == seen[(s, o, 0)] + 4 for s in (0, 1) for o in (1, 2))
