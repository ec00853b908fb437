"""Every kernel form of the generic-width engine (csrc/mshgnn_gen.hip, planned by csrc/mshgnn_gen_plan.hpp) against the fp64 oracle BIT FOR BIT: the
rounding-free data, the comparisons, the routes and the cached cases are those of tests/test_exact_gpu.py; this file adds its models to that table, as
tests/test_exact_families_gpu.py does.  Every run is compared with the oracle, never with another run.  Asserted everywhere: the output, every hidden state
the plan computes and every parameter gradient (exact zeros included) are the oracle's bits; the loss within 2e-7.  tests/test_exact_data.py proves on the
host that every (model, batch, seed) used here is rounding-free and covering, that the sums the engine stages as one bf16 operand row (a relation's
aggregate, forward and backward) are bf16 values, that the base is the live destination the model's name claims, and -- through libmshgnn_hostplan.so, the
pick tests/test_gen_pick.py drives -- which kernels the matrix below reaches.

Models: MI-HGNN at 5 layers on the synthetic robot of N three-joint limbs (helpers.make_limbs_spec: 1 base, 3 N joints, N feet; the base is live as a
destination of N hip-joint rows in layer 0 and the source of N gradient rows in its backward), hidden 128 under MSHGNN_ENGINE=generic; the random
topologies of tests/test_generic_gpu.py (helpers.make_random_topology_spec); MiniCheetah-K4 regression at 5 layers with a 'mean' relation of
in-degrees 1, 2 and 4 (helpers.make_mean_degree_spec).

Matrix (bf16 and x3 arithmetic everywhere; one-call step and two-call route -- training forward, evaluation forward, backward -- unless said otherwise):
  * Default pick, 8 limbs: hidden 128 (17, 300 windows), 256 (17, 300), 384 (300), 512 (17, 300), 768 (300), 1024 (70).  bf16 under 256 windows: k_gstep<false,4,NW>
    at 4 (NCT 1, 3), 8 (NCT 2) and 16 waves (NCT 4, 8); from 256 windows the pipelined k_gstep5 -- 8 waves and <RAW> at 8 waves at hidden 512, the 4-wave plain and
    <RAW> forms at hidden 256 and 768 -- and k_gstep<false,4,4> at the odd NCT 3.  x3: k_gstep<true,4,4> (NCT 1, 3), <true,4,8> (NCT 2, 6), k_gstep5<true,GS5_MB_SPLIT,...>
    at hidden 512 and 1024 (plain launches), k_gstep4<true,4,16> for their raw-input launch.  Sums of 8 rows: one term of 8 sources at hidden 128 and 384 and
    in x3 at 256 and 768; through the aggregate launch k_gagg (from three rows on) at hidden 512 and 1024 and in bf16 at 256 and 768, sums of two rows as two terms there.
  * Tile and pick thresholds, hidden 512: 127, 128, 129 windows (k_gstep on 64-window tiles: two tiles, the second ragged / full / a third of one window;
    x3: k_gstep5 on 96-window tiles) and 255, 256, 257 (bf16 changes from k_gstep<false,4,16> to k_gstep5 on 128-window tiles: two full tiles at 256, a third
    of one window at 257).
  * Every forced mode: MSHGNN_GEN_TILE in {0, 1, 2, 3, 6, 8, 9} at hidden 384 (NCT 3) and 512 (NCT 4), 300 windows -- the table of test_forced_modes in
    tests/test_gen_pick.py, raw-input launch (the encoder) included: the forced-only k_gstep<false,8,8>, k_gstep<true,8,8>, k_gstep<true,4,16>; k_gstep4 in both
    arithmetics; k_gstep5 at 8 and at 4 waves, plain and <RAW>.
  * Aggregate launch and its alternatives, 8 limbs, the `aggregate` row of the engine's profile asserted to have launched or not: hidden 128 and 384 under
    MSHGNN_GEN_MANY=4 (k_gagg runs, its forward sums feed the weight-gradient item of their relation) and with the variable unset (threshold 32: one term of 8
    sources, no launch); hidden 512 unset (k_gagg from three rows on) and under MSHGNN_GEN_MANY=64 (no launch: the 8 rows are gathered inside the job kernel).
  * Many rows, 17 windows: 20 limbs at hidden 512 under MSHGNN_GEN_MANY=64 (no aggregate launch: the 20 rows are ONE term of 20 sources, gathered by k_gstep<false,4,16> /
    k_gstep4<true,4,16>) and with the variable unset (k_gagg over 20 rows); 40 limbs at hidden 128 with the variable unset (more rows than the default threshold of 32: k_gagg).
    The stock generator closes neither (a sum of that many full rows, fed back through the hip joints, leaves bf16 in X2.base / X3.base); exact_case's `thin` knob -- a row density of 0.03 / 0.06 for the relation
    weights into the base -- does, at seeds 3 and 5 (of 1..4 at densities 0.03, 0.1, 0.25 for 20 limbs; of 5..20 at 0.06, 0.1, 0.15 for 40).
  * Topologies no robot has, 21 windows: the random topologies of test_random_topologies_match_the_oracle with seed 7 (hidden 1024) and seed 2 (hidden 128), and topology seed 9
    (2 base, 9 joint, 3 foot nodes, 2 layers) at hidden 256 and 512.  Between them a repeated edge into a live node, an empty relation and a live node without in-edges
    (asserted on the host).
  * 'mean' over in-degrees 2, 4 (one edge repeated), 1 and 2 (1 / in-degree is exact), MiniCheetah-K4 regression at 5 layers, 17 windows: the engine's per-source scale while
    it stages the aggregate.  The relation's weights carry a gain of 4 (exact_case's `gain`), so that W . mean is a whole number: with quarters, none of seeds 1..12 closes
    (two of bf16's 8 bits are gone in every later layer); with the gain seeds 6 and 10 do.  tests/bf16_emulation.py and exact_data._kernel_algebra apply 1 / in-degree where a
    'mean' destination has more than one in-edge, and nothing where it has one (every other case of the three files).
The masked k_gstep5 forms, k_gstep5 behind MSHGNN_GEN_RAW5 and plans without split sums are built only under -DMSHGNN_TUNING; the product library's plans carry
no relu bits in a job's sources, so no launch of it picks a masked form.
Not covered, and why:
  * A launch of more than GS5_MAX_TERMS = 16 terms (k_gstep5's fallback to k_gstep4): no model of this family has one.  A job has one term for its root weights and one
    per relation into its node -- two where a sum of two rows is split -- so at most 7 on the five relations of the MI graph, whatever the in-degree: many rows are one term
    of many sources (the 20-limb case above) or one aggregate row, never many terms.  The pick's rule stays on tests/test_gen_pick.py's own query; k_gstep4 itself runs
    here under MSHGNN_GEN_TILE=6, and in x3 on every raw-input launch at hidden 512 and 1024.
  * Random topology seeds 3 (hidden 256, 3 layers) and 5 (hidden 512): check_exact refuses case seeds 1..8 at 21 windows, on coverage (c) (gradients that are live on random
    data are zero) and once on closure (X3.foot leaves bf16, seed 3 / case seed 1).  Topology seed 9 stands in at both widths.
  * The items of tests/test_exact_gpu.py's list (8-layer models, the cross-entropy step, the series step).
"""
import pytest

from tests import helpers
from tests import test_exact_gpu as gx

pytestmark = pytest.mark.gpu

_K1 = dict(rel_scales=(1.0,))


def _limbs(n, hidden, seeds, **knobs):
    return dict(build=(helpers.make_limbs_spec, n, hidden, 5), knobs=dict(_K1, **knobs), seeds=seeds, program=None)


GENERIC = {      # spec builder and arguments, generator knobs, the seed the host search found per batch size (gx.MODELS' layout)
    "limbs8_h128_L5": _limbs(8, 128, {17: 4, 300: 4}),
    "limbs8_h256_L5": _limbs(8, 256, {17: 5, 300: 5}),
    "limbs8_h384_L5": _limbs(8, 384, {300: 2}),
    "limbs8_h512_L5": _limbs(8, 512, {17: 5, 127: 5, 128: 5, 129: 5, 255: 5, 256: 5, 257: 5, 300: 5}),
    "limbs8_h768_L5": _limbs(8, 768, {300: 2}),
    "limbs8_h1024_L5": _limbs(8, 1024, {70: 1}),
    # many rows into the base: its relation weights thinned (exact_data.exact_case, `thin`), or no seed closes -- a sum of that many full rows outgrows bf16
    "limbs20_h512_L5": _limbs(20, 512, {17: 3}, thin={"base": 0.03}),
    "limbs40_h128_L5": _limbs(40, 128, {17: 5}, thin={"base": 0.06}),
    "random7_h1024_L2": dict(build=(helpers.make_random_topology_spec, 7, 1, 4, 2, 1024, 2), knobs=_K1, seeds={21: 1}, program=None),
    "random2_h128_L2": dict(build=(helpers.make_random_topology_spec, 2, 2, 15, 5, 128, 2), knobs=_K1, seeds={21: 7}, program=None),
    "random9_h256_L2": dict(build=(helpers.make_random_topology_spec, 9, 2, 9, 3, 256, 2), knobs=_K1, seeds={21: 3}, program=None),
    "random9_h512_L2": dict(build=(helpers.make_random_topology_spec, 9, 2, 9, 3, 512, 2), knobs=_K1, seeds={21: 1}, program=None),
    # 'mean' over in-degrees 2, 4, 1, 2: the relation's weights times 4 (`gain`), so that W . mean is a whole number
    "mck4_mean_reg_L5": dict(build=(helpers.make_mean_degree_spec, 5, True), knobs=dict(_K1, gain={"gt": 4.0}), seeds={17: 6}, program=None),
}
gx.MODELS.update(GENERIC)

LIMBS = {m: v["build"][1] for m, v in GENERIC.items() if m.startswith("limbs")}      # model -> in-degree of its base node
DEFAULT_CASES = [(m, B) for m in ("limbs8_h128_L5", "limbs8_h256_L5", "limbs8_h384_L5", "limbs8_h512_L5", "limbs8_h768_L5", "limbs8_h1024_L5")
                 for B in sorted(GENERIC[m]["seeds"]) if B in (17, 70, 300)]
THRESHOLD_MODEL, THRESHOLD_BATCHES = "limbs8_h512_L5", [127, 128, 129, 255, 256, 257]
FORCED_MODES = ["0", "1", "2", "3", "6", "8", "9"]
FORCED_CASES = [(m, 300, mode) for m in ("limbs8_h384_L5", "limbs8_h512_L5") for mode in FORCED_MODES]
AGGREGATE_CASES = [      # (model, batch, MSHGNN_GEN_MANY or None, the aggregate launch runs)
    ("limbs8_h128_L5", 17, "4", True), ("limbs8_h128_L5", 17, None, False),
    ("limbs8_h384_L5", 300, "4", True), ("limbs8_h384_L5", 300, None, False),
    ("limbs8_h512_L5", 17, None, True), ("limbs8_h512_L5", 17, "64", False),
]
MANY_ROW_CASES = [      # 20 rows as one term of 20 sources, and through k_gagg (from three rows on at hidden 512); 40 rows: past the default threshold of 32
    ("limbs20_h512_L5", 17, "64", False), ("limbs20_h512_L5", 17, None, True), ("limbs40_h128_L5", 17, None, True),
]
RANDOM_CASES = [(m, B) for m in GENERIC if m.startswith("random") for B in sorted(GENERIC[m]["seeds"])]
MEAN_CASES = [("mck4_mean_reg_L5", 17)]
CASES = sorted({(m, B) for m in GENERIC for B in GENERIC[m]["seeds"]})      # what tests/test_exact_data.py proves on the host
GEN_SWITCHES = ("MSHGNN_GEN_TILE", "MSHGNN_GEN_MANY")


def _engine(monkeypatch, spec, model, dtype, env=None):
    """An engine on the generic-width kernels with exactly the switches of `env` (MSHGNN_GEN_MANY is read when the plan is compiled, MSHGNN_GEN_TILE per
    launch: both stay set until the next engine is made)."""
    for k in GEN_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    env = dict(env or {}, **({"MSHGNN_ENGINE": "generic"} if spec.hidden == 128 else {}))
    e = gx._engine(monkeypatch, spec, model, dtype, env, False)
    assert e.generic and e.info.kernel_sets == 4, f"{model} {dtype}: not the generic engine"
    return e


def _run(monkeypatch, model, B, env=None, aggregate=None):
    """Both arithmetics under `env`: the one-call step (regression models) and the two-call route against the oracle; aggregate: True / False -- the
    aggregate launch (k_gagg) must / must not have run in the step or the route's training forward and backward."""
    spec, case, ref, _ = gx._reference(model, B)
    bad = []
    for dtype in ("bf16", "x3"):
        e = _engine(monkeypatch, spec, model, dtype, env)
        name = f"{model} B={B} {dtype} {env or ''}"
        if aggregate is not None:
            e.profile(True)
        if spec.regression:
            gx._step(bad, name, e, spec, case, ref, B)
        gx._two_call(bad, name, e, spec, case, ref, B)
        if aggregate is not None:
            n = sum(r["launches"] for r in e.profile_read() if r["name"] == "aggregate")
            assert (n > 0) == aggregate, f"{name}: {n} aggregate launches"
        del e
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("model,B", DEFAULT_CASES)
def test_default_pick_is_the_oracle_bit_for_bit(monkeypatch, model, B):
    """The 8-limb model at every width class on the kernels the pick gives with no switch set (module docstring: which ones)."""
    _run(monkeypatch, model, B)


@pytest.mark.parametrize("B", THRESHOLD_BATCHES)
def test_tile_and_pick_thresholds_are_the_oracle_bit_for_bit(monkeypatch, B):
    """Hidden 512 on either side of a full 128-window tile and of two: a ragged tile's masked rows, a tile of one window, and at 256 windows the bf16
    plan's change from k_gstep<false,4,16> to the pipelined k_gstep5."""
    _run(monkeypatch, THRESHOLD_MODEL, B)


@pytest.mark.parametrize("model,B,mode", FORCED_CASES)
def test_forced_mode_is_the_oracle_bit_for_bit(monkeypatch, model, B, mode):
    """MSHGNN_GEN_TILE: the table of test_forced_modes in tests/test_gen_pick.py at NCT 3 and 4 on 300 windows, each kernel against the oracle."""
    _run(monkeypatch, model, B, {"MSHGNN_GEN_TILE": mode})


@pytest.mark.parametrize("model,B,many,runs", AGGREGATE_CASES + MANY_ROW_CASES)
def test_aggregate_launch_and_its_alternatives_are_the_oracle_bit_for_bit(monkeypatch, model, B, many, runs):
    """The sums into and out of the base node through k_gagg's buffers (which the weight-gradient item of the relation reads too), or gathered by the job
    kernel as one term of many sources -- whichever the threshold gives, asserted from the engine's profile."""
    _run(monkeypatch, model, B, {"MSHGNN_GEN_MANY": many} if many else None, aggregate=runs)


@pytest.mark.parametrize("model,B", RANDOM_CASES + MEAN_CASES)
def test_topology_no_robot_has_is_the_oracle_bit_for_bit(monkeypatch, model, B):
    """Random edge lists (repeated edges, an empty relation, nodes without in-edges, in-degrees up to the node count) and a 'mean' relation over
    in-degrees 1, 2 and 4."""
    _run(monkeypatch, model, B)
