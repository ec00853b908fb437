"""Which kernel a stack or encoder launch of the LDS-resident engine gets: pick_stack / pick_enc / spec_form of mshgnn_pick.hpp, driven on the CPU through
libmshgnn_hostplan.so (as tests/test_gen_pick.py drives the generic engine's pick).  mshgnn.hip and mshgnn_x3.hip launch row `k` of the picked family's table with the
pick's grid, block and LDS, copy the pick's program table, scratch offset, store policy and stagger into the kernel arguments and decide nothing else, so what is
asserted here is what runs: the cases DESIGN.md and the docstrings of tests/test_spec_gpu.py state, invariants over the whole query space, and reachability of every
table row.

A query's `use_spec` means: the plan has a compile-time program (built in, or attached) and MSHGNN_SPEC is not 0.  `op`: forward in evaluation, forward in training,
backward, forward with a fused loss (the first launch of a one-call step)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "morphsym_hgnn_amd", "csrc")
F32, BF16, X3P = 0, 1, 2
EVAL, TRAIN, BWD_OP, LOSS = 0, 1, 2, 3
PER_LAYER, STACK8, SLAB, SLAB_SPEC, X3, X3_SPEC = range(6)
FWD, BWD, STEP = 0, 1, 2
EOK, EINVAL, EUNSUPPORTED = 0, -1, -2
FIELDS = ("plan", "op", "B", "n_cu", "use_fused", "use_slab", "slab_force", "use_spec", "use_step", "stash_nt", "gw_phase", "n_mlp", "sl_hb", "sl_blk", "fs_blk",
          "x3_alias", "node0", "n_out", "blk", "stagger", "extra_blk")
PICK = ("family", "what", "NM", "HB", "NT", "TR", "FULL", "ALIAS", "k", "threads", "lds", "tiles", "slab_prog", "red_off", "stash_nt", "stagger")
BLK = {F32: 8192, BF16: 4096, X3P: 4096}      # bytes of one LDS node block
SL_HB, SL_HB_MAX = 6, 8
DEC_SLAB_BYTES = (8 * 128 + 16) * 4            # one decoder slab per wave: the reduction scratch of a one-launch step
# (node0, n_out, fs_blk, sl_blk): where the reduction scratch of a one-launch step can go beside the out type's blocks
FRONT = (12, 4, 20, 18)         # in front of them, on every family (A1-C2: the out type comes last)
BEHIND = (0, 1, 17, 14)         # the out type comes first (the centroidal-momentum models): not in front, behind
NOWHERE = (2, 14, 18, 17)       # neither: no one-launch step
SLAB_ONLY = (5, 13, 19, 19)     # 4 waves' scratch fits in front, 8 waves' fits nowhere
# the query space (the one the pick was compared on with the ladders it replaced)
SPACE = dict(plan=(F32, BF16, X3P), op=(EVAL, TRAIN, BWD_OP, LOSS), B=(1, 15, 16, 17, 30, 32, 4096, 4097, 4112, 8190, 8192), n_cu=(64, 256, 304), use_fused=(0, 1),
             use_slab=(0, 1), slab_force=(0, 1), use_spec=(0, 1), use_step=(0, 1), stash_nt=(0, 1), gw_phase=(-1, 0), mlp=((1, SL_HB), (2, SL_HB_MAX), (3, SL_HB), (4, SL_HB_MAX)),
             layout=(FRONT, BEHIND, NOWHERE, SLAB_ONLY), x3_alias=(0, 1))
STAGGER = 2048
# rows only a switch reaches (MSHGNN_SLAB=2, MSHGNN_STEP_KERNEL=0): none -- a plan whose tables do not allow the slab or fused kernels has use_slab / use_fused off as well
FORCED_ONLY = set()


@pytest.fixture(scope="module")
def lib():
    path = os.path.join(ROOT, "morphsym_hgnn_amd", "libmshgnn_hostplan.so")
    subprocess.run(["make", "-C", CSRC, "../libmshgnn_hostplan.so"], check=True, capture_output=True)
    lib = C.CDLL(path)
    lib.mshgnn_hostplan_stack_pick.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    lib.mshgnn_hostplan_stack_pick.restype = None
    lib.mshgnn_hostplan_enc_pick.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    lib.mshgnn_hostplan_enc_pick.restype = None
    lib.mshgnn_hostplan_stack_kernel_name.restype = C.c_char_p
    lib.mshgnn_hostplan_enc_form_name.restype = C.c_char_p
    lib.mshgnn_hostplan_red_need.restype = C.c_int64
    return lib


@pytest.fixture(scope="module")
def names(lib):
    """names[family][k]; every row of every family has a name of its own."""
    out = [[lib.mshgnn_hostplan_stack_kernel_name(f, k).decode() for k in range(lib.mshgnn_hostplan_stack_kernel_count(f))] for f in range(6)]
    assert [len(n) for n in out] == [2, 3, 12, 9, 5, 3]
    flat = [n for fam in out for n in fam]
    assert all(flat) and len(set(flat)) == len(flat)
    assert lib.mshgnn_hostplan_stack_kernel_name(SLAB, 12) == b"" and lib.mshgnn_hostplan_stack_kernel_count(6) == 0
    return out


def _pick(lib, queries):
    q = np.ascontiguousarray(queries, dtype=np.int32).reshape(-1, len(FIELDS))
    p = np.zeros((q.shape[0], len(PICK)), dtype=np.int32)
    lib.mshgnn_hostplan_stack_pick(q.ctypes.data, p.ctypes.data, q.shape[0])
    return p


def _one(lib, names, **kw):
    """The pick of one query as a dict, `name` added; unnamed fields: the bf16 plan of A1-C2 on 256 CUs, every switch at its default, no program."""
    q = dict(plan=BF16, op=LOSS, B=32, n_cu=256, use_fused=1, use_slab=1, slab_force=0, use_spec=0, use_step=1, stash_nt=0, gw_phase=-1, n_mlp=2, sl_hb=SL_HB,
             x3_alias=0, stagger=STAGGER, extra_blk=0)
    q["node0"], q["n_out"], q["fs_blk"], q["sl_blk"] = kw.pop("layout", FRONT)
    assert set(kw) <= set(q)
    q.update(kw)
    q["blk"] = BLK[q["plan"]]
    if q["plan"] == X3P: q.update(use_slab=0, stagger=0)
    p = dict(zip(PICK, (int(v) for v in _pick(lib, [[q[f] for f in FIELDS]])[0])))
    p["name"] = names[p["family"]][p["k"]]
    return p


def _name(lib, names, **kw):
    return _one(lib, names, **kw)["name"]


def test_a_plan_with_a_program_runs_it_at_every_batch_size(lib, names):
    """DESIGN.md, "Which stack kernel a launch takes", and tests/test_spec_gpu.py: the one-call step at 16, 32, 64 and 4 096 windows on the unpredicated program, at 30 and
    50 on the predicated form, which exists with plain stash stores only."""
    for nt in (0, 1):
        for B in (16, 32, 64, 4096, 8192):
            p = _one(lib, names, use_spec=1, B=B, stash_nt=nt)
            assert (p["name"], p["what"], p["FULL"], p["NT"], p["threads"], p["slab_prog"]) == (f"k_slab_step<SP,NT={nt},FULL>", STEP, 1, nt, 256, 1)
    for B in (30, 50, 8190):
        assert _name(lib, names, use_spec=1, B=B, stash_nt=0) == "k_slab_step<SP,NT=0,RAGGED>"
    # a ragged step whose stash wants non-temporal stores keeps the interpreter: 8-wave up to one tile per CU, slab beyond
    assert _name(lib, names, use_spec=1, B=30, stash_nt=1) == "k_stack_step<bf16>"
    assert _name(lib, names, use_spec=1, B=4090, stash_nt=1) == "k_stack_step<bf16>"      # 256 tiles on 256 CUs
    assert _name(lib, names, use_spec=1, B=4097, stash_nt=1) == "k_slab_step<bf16,2,SL_HB>"
    assert _name(lib, names, use_spec=1, B=8190, stash_nt=1) == "k_slab_step<bf16,2,SL_HB>"


def test_forward_and_backward_alone(lib, names):
    for nt in (0, 1):
        # forward evaluation, whole tiles or ragged: the program; an evaluation stashes nothing, so no store policy reaches the kernel
        for B, form in ((16, "FULL"), (4096, "FULL"), (8192, "FULL"), (30, "RAGGED"), (8190, "RAGGED")):
            p = _one(lib, names, use_spec=1, op=EVAL, B=B, stash_nt=nt)
            assert (p["name"], p["stash_nt"], p["what"]) == (f"k_slab_fwd_spec<SP,TR=0,NT=0,{form}>", 0, FWD)
        # the two-call training route: whole tiles on the program, with the launch's store policy
        for B in (16, 32, 4096, 8192):
            assert _name(lib, names, use_spec=1, op=TRAIN, B=B, stash_nt=nt) == f"k_slab_fwd_spec<SP,TR=1,NT={nt},FULL>"
            assert _name(lib, names, use_spec=1, op=BWD_OP, B=B, stash_nt=nt) == f"k_slab_bwd_spec<SP,NT={nt}>"
        # ... ragged: the interpreters, forward and backward alike
        for B, fwd, bwd in ((30, "k_stack_fwd<bf16>", "k_stack_bwd<bf16>"), (4090, "k_stack_fwd<bf16>", "k_stack_bwd<bf16>"),
                            (4097, "k_slab_fwd<bf16,2,SL_HB>", "k_slab_bwd<bf16,2,SL_HB>"), (8190, "k_slab_fwd<bf16,2,SL_HB>", "k_slab_bwd<bf16,2,SL_HB>")):
            p = _one(lib, names, use_spec=1, op=TRAIN, B=B, stash_nt=nt)
            assert (p["name"], p["stash_nt"]) == (fwd, nt)
            assert _name(lib, names, use_spec=1, op=BWD_OP, B=B, stash_nt=nt) == bwd


def test_plans_without_a_program_and_the_switches(lib, names):
    # no program: 8-wave up to one tile per CU, slab from n_cu + 1 tiles (tools/slab_threshold_sweep.py); MSHGNN_SPEC=0 is the same query
    for n_cu in (64, 256, 304):
        for op, what in ((EVAL, "fwd"), (TRAIN, "fwd"), (BWD_OP, "bwd"), (LOSS, "step")):
            for B in (1, 16, 30, 16 * n_cu - 1, 16 * n_cu):
                p = _one(lib, names, op=op, B=B, n_cu=n_cu)
                assert (p["name"], p["threads"], p["lds"], p["slab_prog"], p["stagger"]) == (f"k_stack_{what}<bf16>", 512, 20 * 4096, 0, 0)
            for B in (16 * n_cu + 1, 16 * n_cu + 16, 8 * 16 * n_cu):
                p = _one(lib, names, op=op, B=B, n_cu=n_cu)
                assert (p["name"], p["threads"], p["lds"], p["slab_prog"], p["stagger"]) == (f"k_slab_{what}<bf16,2,SL_HB>", 256, 18 * 4096, 1, STAGGER)
    # the slab instantiation follows the plan: NM = bound on the base_transform nodes, HB = group-B slots
    for n_mlp, sl_hb, inst in ((0, 6, "2,SL_HB"), (2, 8, "2,SL_HB_MAX"), (3, 6, "4,SL_HB"), (4, 8, "4,SL_HB_MAX"), (4, 7, "4,SL_HB_MAX")):
        for op, what in ((EVAL, "fwd"), (BWD_OP, "bwd"), (LOSS, "step")):
            assert _name(lib, names, op=op, B=8192, n_mlp=n_mlp, sl_hb=sl_hb) == f"k_slab_{what}<bf16,{inst}>"
    for spec in (0, 1):
        for B in (16, 30, 4097, 8192):
            # MSHGNN_SLAB=0: 8-wave everywhere and never a program
            for op, what in ((EVAL, "fwd"), (TRAIN, "fwd"), (BWD_OP, "bwd"), (LOSS, "step")):
                assert _name(lib, names, use_slab=0, use_spec=spec, op=op, B=B) == f"k_stack_{what}<bf16>"
            # MSHGNN_STEP_KERNEL=0: never a step; the forward of the two-launch sequence as the two-call route takes it
            p = _one(lib, names, use_step=0, use_spec=spec, B=B)
            assert p["what"] == FWD and p["name"] == _name(lib, names, use_spec=spec, op=TRAIN, B=B) and p["red_off"] == 0
    # MSHGNN_SLAB=2: the slab kernels at one tile, and nothing to stagger below one tile per CU
    for op, what in ((EVAL, "fwd"), (TRAIN, "fwd"), (BWD_OP, "bwd"), (LOSS, "step")):
        p = _one(lib, names, slab_force=1, op=op, B=16)
        assert (p["name"], p["stagger"]) == (f"k_slab_{what}<bf16,2,SL_HB>", 0)
        assert _one(lib, names, slab_force=1, op=op, B=4112)["stagger"] == STAGGER
    # MSHGNN_FUSED=0 and the fp32 plan: one kernel per layer, whatever else is set
    for kw in (dict(use_fused=0), dict(plan=F32), dict(plan=F32, use_fused=0)):
        for spec in (0, 1):
            for B in (16, 30, 8192):
                assert _name(lib, names, op=LOSS, B=B, use_spec=spec, **kw) == "k_layer_fwd<T>" and _name(lib, names, op=BWD_OP, B=B, use_spec=spec, **kw) == "k_layer_bwd<T>"


def test_a_step_needs_room_for_its_reduction_scratch(lib, names):
    need4, need8 = 4 * DEC_SLAB_BYTES, 8 * DEC_SLAB_BYTES
    assert (lib.mshgnn_hostplan_red_need(256), lib.mshgnn_hostplan_red_need(512)) == (need4, need8)
    for spec in (0, 1):
        for B in (32, 8192):
            assert _one(lib, names, use_spec=spec, B=B, layout=FRONT)["red_off"] == 0
            # the centroidal-momentum layout: not in front (the out type is node 0), behind the out-type block
            p = _one(lib, names, use_spec=spec, B=B, layout=BEHIND)
            assert (p["what"], p["red_off"]) == (STEP, 1 * 4096)
            # nowhere: the forward alone (the two-launch sequence), its scratch offset unset
            p = _one(lib, names, use_spec=spec, B=B, layout=NOWHERE)
            assert (p["what"], p["red_off"]) == (FWD, 0) and p["name"] == _name(lib, names, use_spec=spec, op=TRAIN, B=B, layout=NOWHERE)
    # 4 waves' scratch fits, 8 waves' does not: a step only where the slab kernels run
    assert _one(lib, names, B=32, layout=SLAB_ONLY)["name"] == "k_stack_fwd<bf16>"
    assert _one(lib, names, B=8192, layout=SLAB_ONLY)["name"] == "k_slab_step<bf16,2,SL_HB>"
    assert _one(lib, names, B=32, use_spec=1, layout=SLAB_ONLY)["name"] == "k_slab_step<SP,NT=0,FULL>"
    # the split plan: 8 waves, inside the hi plane
    assert _one(lib, names, plan=X3P, layout=BEHIND)["red_off"] == 4096 and _one(lib, names, plan=X3P, layout=FRONT)["red_off"] == 0
    for lay in (NOWHERE, SLAB_ONLY):
        assert _one(lib, names, plan=X3P, layout=lay)["what"] == FWD


def test_the_split_plan(lib, names):
    for B in (1, 16, 30, 4096, 8190, 8192):
        for alias in (0, 1):
            a = "true" if alias else "false"
            for nt in (0, 1):
                kw = dict(plan=X3P, B=B, x3_alias=alias, stash_nt=nt)
                # its program on every batch, ragged included (predicated stores)
                for op, name, what in ((LOSS, "k_stack_step_x3<ALIAS,SP>", STEP), (EVAL, "k_stack_fwd_x3_spec<ALIAS,SP>", FWD), (TRAIN, "k_stack_fwd_x3_spec<ALIAS,SP>", FWD),
                                       (BWD_OP, "k_stack_bwd_x3_spec<SP>", BWD)):
                    p = _one(lib, names, use_spec=1, op=op, **kw)
                    assert (p["name"], p["what"], p["threads"], p["lds"], p["slab_prog"], p["stagger"]) == (name, what, 512, 2 * 20 * 4096, 0, 0)
                    assert p["ALIAS"] == (alias if what != BWD else 0)
                    assert p["stash_nt"] == nt      # (an evaluation leaves the policy set on this plan)
                for op, name in ((LOSS, f"k_stack_step_x3<{a}>"), (EVAL, f"k_stack_fwd_x3<{a}>"), (TRAIN, f"k_stack_fwd_x3<{a}>"), (BWD_OP, "k_stack_bwd_x3")):
                    assert _name(lib, names, op=op, **kw) == name
                # a two-phase step keeps the backward sweep a launch of its own on this plan; the bf16 plan has no such condition
                for spec in (0, 1):
                    assert _one(lib, names, gw_phase=0, use_spec=spec, **kw)["what"] == FWD and _one(lib, names, use_step=0, use_spec=spec, **kw)["what"] == FWD
                    assert _one(lib, names, plan=BF16, gw_phase=0, use_spec=spec, B=B)["what"] == STEP


def test_spec_form(lib):
    """The specialised forms that exist: on whole tiles everything, both store policies; on a ragged batch the step with plain stores and the evaluation forward."""
    sf = lambda *a: lib.mshgnn_hostplan_spec_form(BF16, *a)
    assert [sf(0, 1, nt, full) for full in (1, 0) for nt in (0, 1)] == [0, 1, 2, -1]
    assert [sf(1, 0, nt, full) for full in (1, 0) for nt in (0, 1)] == [3, 3, 4, 4]
    assert [sf(1, 1, nt, full) for full in (1, 0) for nt in (0, 1)] == [5, 6, -1, -1]
    assert [sf(2, 1, nt, full) for full in (1, 0) for nt in (0, 1)] == [7, 8, -1, -1]
    assert [lib.mshgnn_hostplan_spec_form(X3P, kind, tr, nt, full) for kind in (0, 1, 2) for tr in (0, 1) for nt in (0, 1) for full in (0, 1)] == [0] * 8 + [1] * 8 + [2] * 8
    assert sf(3, 1, 0, 1) == -1 and sf(-1, 1, 0, 1) == -1 and lib.mshgnn_hostplan_spec_form(F32, 0, 1, 0, 1) == -1 and lib.mshgnn_hostplan_spec_form(X3P, 3, 1, 0, 1) == -1


def test_invariants_over_the_query_space(lib, names):
    axes = list(SPACE)
    grids = np.meshgrid(*[np.arange(len(SPACE[f])) for f in axes], indexing="ij")
    shape = grids[0].shape
    ix = {f: g.reshape(-1) for f, g in zip(axes, grids)}
    val = {f: np.array(SPACE[f], dtype=np.int64)[ix[f]] for f in axes}
    Q = {f: val[f] for f in axes if f not in ("mlp", "layout")}
    Q["n_mlp"], Q["sl_hb"] = val["mlp"][:, 0], val["mlp"][:, 1]
    Q["node0"], Q["n_out"], Q["fs_blk"], Q["sl_blk"] = (val["layout"][:, i] for i in range(4))
    n = ix["plan"].size
    assert n == 1622016
    Q["blk"] = np.array([BLK[F32], BLK[BF16], BLK[X3P]])[Q["plan"]]
    Q["stagger"], Q["extra_blk"] = np.full(n, STAGGER), np.zeros(n, dtype=np.int64)
    p = _pick(lib, np.stack([Q[f] for f in FIELDS], axis=1))
    P = {f: p[:, i].astype(np.int64) for i, f in enumerate(PICK)}
    fam, what, k = P["family"], P["what"], P["k"]
    tiles = (Q["B"] + 15) // 16
    full = Q["B"] % 16 == 0
    # every pick names a row of its family's table; the fp32 plan and MSHGNN_FUSED=0 have the per-layer kernels, the fused plans their own families
    rows = np.array([len(f) for f in names])
    assert fam.min() >= 0 and fam.max() < 6 and np.all(k >= 0) and np.all(k < rows[fam])
    per_layer = (Q["plan"] == F32) | (Q["use_fused"] == 0)
    assert np.array_equal(fam == PER_LAYER, per_layer)
    assert np.all(np.isin(fam[~per_layer & (Q["plan"] == BF16)], (STACK8, SLAB, SLAB_SPEC))) and np.all(np.isin(fam[~per_layer & (Q["plan"] == X3P)], (X3, X3_SPEC)))
    assert np.array_equal(P["tiles"], tiles)
    # threads and LDS are the family's
    slabf, x3f = np.isin(fam, (SLAB, SLAB_SPEC)), np.isin(fam, (X3, X3_SPEC))
    assert np.array_equal(P["threads"], np.where(slabf, 256, 512))
    lds = np.select([fam == PER_LAYER, fam == STACK8, slabf, x3f], [0, Q["fs_blk"] * Q["blk"], Q["sl_blk"] * Q["blk"], 2 * Q["fs_blk"] * Q["blk"]])
    assert np.array_equal(P["lds"], lds)
    assert np.array_equal(P["slab_prog"] == 1, slabf)
    # the template coordinates: the slab instantiation is the plan's; FULL only on whole tiles; a program's form exists and is the row
    assert np.array_equal(P["NM"][slabf], np.where(Q["n_mlp"] <= 2, 2, 4)[slabf]) and np.array_equal(P["HB"][slabf], np.where(Q["sl_hb"] <= SL_HB, SL_HB, SL_HB_MAX)[slabf])
    assert np.array_equal(k[fam == SLAB], (what * 4 + (P["NM"] == 4) * 2 + (P["HB"] == SL_HB_MAX))[fam == SLAB])
    assert np.all(full[P["FULL"] == 1]) and np.all(P["FULL"][fam != SLAB_SPEC] == 0)
    spec = np.nonzero(fam == SLAB_SPEC)[0]
    kind = np.array([1, 2, 0])[what]      # FWD, BWD, STEP -> the selector's kind
    forms = {key: lib.mshgnn_hostplan_spec_form(BF16, *key) for key in {(int(kind[i]), int(P["TR"][i]), int(P["NT"][i]), int(P["FULL"][i])) for i in spec}}
    form_of = np.array([forms[(int(kind[i]), int(P["TR"][i]), int(P["NT"][i]), int(P["FULL"][i]))] for i in spec])
    assert np.all(form_of >= 0) and np.array_equal(form_of, k[spec])
    assert np.all(Q["use_spec"][np.isin(fam, (SLAB_SPEC, X3_SPEC))] == 1) and np.all(Q["use_slab"][slabf] == 1)
    assert np.array_equal(P["NT"][spec], (P["stash_nt"] * (P["TR"] == 1))[spec]) and np.all(full[spec] == (P["FULL"][spec] == 1))
    assert np.array_equal(k[fam == STACK8], what[fam == STACK8])
    assert np.array_equal(P["ALIAS"][x3f], (Q["x3_alias"] * (what != BWD))[x3f]) and np.all(P["ALIAS"][~x3f] == 0)
    # the store policy: the bf16 evaluation forward zeroes it, the split plan does not
    fused16 = ~per_layer & (Q["plan"] == BF16)
    assert np.array_equal(P["stash_nt"], np.where(fused16 & (Q["op"] == EVAL), 0, Q["stash_nt"]))
    # stagger: only above n_cu tiles on a slab-for-tiles launch
    assert np.array_equal(P["stagger"], np.where(fused16 & (Q["use_slab"] == 1) & (tiles > Q["n_cu"]), STAGGER, 0))
    assert np.all(slabf[P["stagger"] > 0])
    # STEP implies a fused loss and the step switch; its reduction scratch lies inside the launch's LDS (split plan: the hi plane) beside the out-type blocks
    step = what == STEP
    assert np.array_equal(what == BWD, Q["op"] == BWD_OP)
    assert np.all(Q["op"][step] == LOSS) and np.all(Q["use_step"][step] == 1) and np.all(fam[step] != PER_LAYER)
    assert np.all((Q["gw_phase"] < 0)[step & x3f])
    need = (P["threads"] // 64) * DEC_SLAB_BYTES
    extent = np.where(x3f, P["lds"] // 2, P["lds"])
    lo, hi = Q["node0"] * Q["blk"], (Q["node0"] + Q["n_out"]) * Q["blk"]
    assert np.all(P["red_off"][~step] == 0) and np.all(P["red_off"] >= 0)
    assert np.all((P["red_off"] + need <= extent)[step]) and np.all(((P["red_off"] + need <= lo) | (P["red_off"] >= hi))[step])
    # ... and a step is taken wherever it is asked for and the scratch fits the family that then runs
    fits = lambda n_, ext: (lo >= n_) | (hi + n_ <= ext)
    want = ~per_layer & (Q["op"] == LOSS) & (Q["use_step"] == 1) & ((Q["plan"] == BF16) | (Q["gw_phase"] < 0))
    fits_fam = np.where(slabf, fits(4 * DEC_SLAB_BYTES, Q["sl_blk"] * Q["blk"]), fits(8 * DEC_SLAB_BYTES, Q["fs_blk"] * Q["blk"]))
    assert np.all(step[want & fits(4 * DEC_SLAB_BYTES, Q["sl_blk"] * Q["blk"]) & fits(8 * DEC_SLAB_BYTES, Q["fs_blk"] * Q["blk"])]) and np.all(fits_fam[step])
    # forward and backward of the two-call training route agree on the program table (the backward reads the forward's stashes through it), store policy and instantiation
    by_op = lambda f: np.moveaxis(P[f].reshape(shape), axes.index("op"), 0)
    for f in ("family", "slab_prog", "NM", "HB", "NT", "FULL", "stash_nt", "threads", "lds", "stagger"):
        assert np.array_equal(by_op(f)[TRAIN], by_op(f)[BWD_OP]), f
        no_step = by_op("what")[LOSS] != STEP      # MSHGNN_STEP_KERNEL=0, or no room for the scratch: the two-launch sequence
        assert np.array_equal(by_op(f)[LOSS][no_step], by_op(f)[BWD_OP][no_step]), f
    # reachability: the union of the picked rows is every table's every row, with the switches at their defaults already
    reached = lambda m: {names[f][r] for f, r in set(zip(fam[m].tolist(), k[m].tolist()))}
    everything = {n_ for f in names for n_ in f}
    assert reached(np.ones(n, dtype=bool)) == everything
    assert reached((Q["slab_force"] == 0) & (Q["use_step"] == 1)) == everything - FORCED_ONLY


ENC_FORMS = ("ELEMENTWISE", "ALIGNED", "WIDE4", "WIDE8", "SERIES", "SERIES_STD", "SERIES_SIGNED", "SERIES_SIGNED_STD", "SERIES_ORBIT", "SERIES_ORBIT_STD")


def test_the_encoder_pick(lib):
    """Every set of route facts maps to the form the encoder ladders of the two plans launched: series before wide sources, a group element per window (K > 1 in the sign
    word) before one element's signs before none, standardised or raw; wide rows by their element size; else the aligned or element-wise encoder of the caller's rows.
    The fp32 plan (no source routes) refuses wide sources and ignores a series; unaligned rows where rows are written are refused."""
    assert [lib.mshgnn_hostplan_enc_form_name(i).decode() for i in range(lib.mshgnn_hostplan_enc_form_count())] == list(ENC_FORMS)
    facts, want = [], []
    for src_routes in (0, 1):
        for wide_needs_rows in (0, 1):
            for series, stats, sign, lab in [(0, 0, 0, 0)] + [(1, st, sg, lb) for st in (0, 1) for sg in (0, 1, 1 | (4 << 8), 2 << 8) for lb in (0, 1, 256, 257, 8192)]:
                for wide in (0, 4, 8):
                    if series and wide: continue      # (refused before any launch)
                    for x in (0, 1):
                        for aligned in (0, 1):
                            facts.append((series, stats, sign, lab, wide, x, aligned, src_routes, wide_needs_rows, 0))
                            plain = "ALIGNED" if aligned else "ELEMENTWISE"
                            if not src_routes: want.append((plain, 0, EUNSUPPORTED if wide else EOK))
                            elif series:
                                form = ("SERIES_ORBIT" if sign >> 8 else "SERIES_SIGNED" if sign else "SERIES") + ("_STD" if stats else "")
                                want.append((plain, 0, EINVAL) if x and not aligned else (form, (lab + 255) // 256, EOK))
                            elif wide: want.append((plain, 0, EINVAL) if (x or wide_needs_rows) and not aligned else (f"WIDE{wide}", 0, EOK))
                            else: want.append((plain, 0, EOK))
    f = np.ascontiguousarray(facts, dtype=np.int32)
    out = np.zeros((f.shape[0], 3), dtype=np.int32)
    lib.mshgnn_hostplan_enc_pick(f.ctypes.data, out.ctypes.data, f.shape[0])
    got = [(ENC_FORMS[o[0]], int(o[1]), int(o[2])) for o in out]
    assert len(got) == 688 and got == want
    ok = [g[0] for g in got if g[2] == EOK]
    assert set(ok) == set(ENC_FORMS)
    # the fp32 plan's table has the two forms of the caller's rows: no fact set names another row there
    assert {g[0] for g, fa in zip(got, facts) if not fa[7]} == {"ELEMENTWISE", "ALIGNED"}
