"""Every model family the library ships against the fp64 oracle BIT FOR BIT, at depths where the base nodes are live: the rounding-free data, the
comparisons and the routes are those of tests/test_exact_gpu.py (whose matrix is A1-C2 and MiniCheetah-K4 at 3 layers, base nodes dead); this file adds
the families to its table and runs them.  tests/test_exact_data.py proves closure and coverage on the host for every (family, batch, seed) used here, and
that each case really has the live base its name claims.

Families (hidden 128, the LDS-resident kernels, no compile-time program: `specialised == ""` is asserted on every kernel set):
  * A1-C2 at 4 layers: the base encoder (F = 900) and the base -> joint relations are live, the base is never a destination.  Also under type-level
    liveness (MSHGNN_PRUNE=0, bf16 and split).
  * A1-C2 at 5 layers: every node of every type is live, the base is a destination in layer 0 (relations into base, base_transform, the base rows of a
    stack layer).  Also through the programs compiled on demand (morphsym_hgnn_amd/jit.py), bf16 and split, against the oracle.
  * MiniCheetah-C2 contact classification at 4 layers; MiniCheetah-K4 contact classification at 5 layers (four base nodes, the gt / gs mean relations).
  * MiniCheetah-K4 regression at 3 layers (one output per foot).
  * MI-HGNN (no symmetry group, no base_transform, no residual) at 5 layers, at 17 windows and at 1000 (seed 5 closes both: no fall-back to 4 or 3 layers
    was needed).
  * Solo K4, C2 (4 layers) and S4 (5 layers) centroidal momentum: the decoder sits on the base nodes (6 outputs each), there is no foot type, the base is
    a destination in every layer, S4 has a single base node.
Batches: every family at 17 windows (one whole tile plus one window) and at 1000 (many tiles, a ragged last one); A1-C2 L4 also at 16 and, with Solo K4
COM L4, at 8193 (past the slab threshold; the stash store policy and the tile staircase change the launch there).
Routes: regression families run the one-call step on the bf16 plan's default kernels, MSHGNN_SLAB=0, MSHGNN_FUSED=0, MSHGNN_STASH_NT=1, the split plan and
the fp32 plan, then the two-call route, the two-phase step and the fp64-source step on the bf16 and split defaults.  Classification families run logits,
hidden states and backward(gout) (their one-call cross-entropy step: tests/test_exact_ce_gpu.py, on cases where the softmax gradient is exact).  Every family also runs at 17 windows through the
generic-width engine forced with MSHGNN_ENGINE=generic (bf16 and split), A1-C2 L4 and Solo K4 COM L4 at hidden 256 as well.
Not covered, and why:
  * MiniCheetah-C2 classification at 5 layers: none of seeds 1..12 closes it at 17 windows (X4.joint leaves bf16), so its base-destination path is
    carried by MiniCheetah-K4 L5 and A1-C2 L5, which share its kernels.
  * 8-layer models and the series step: see tests/test_exact_gpu.py.
No case of the required matrix had to be left out: a seed closes every (family, batch) above.
"""
import pytest

from morphsym_hgnn_amd import jit
from tests import test_exact_gpu as gx

pytestmark = pytest.mark.gpu

_K1 = dict(rel_scales=(1.0,))
_CLS = dict(rel_scales=(1.0,), bias_range=(0, 1))
FAMILIES = {      # spec arguments, generator knobs, the seed the host search found per batch size (gx.MODELS' layout; no compile-time program at these depths)
    "a1c2_L4": dict(spec=("c2", "a1-c2", "a1-c2", 128, 4, True), knobs=_K1, seeds={16: 3, 17: 3, 1000: 3, 8193: 3}),
    "a1c2_L5": dict(spec=("c2", "a1-c2", "a1-c2", 128, 5, True), knobs=_K1, seeds={17: 5, 1000: 5}),
    "mcc2_cls_L4": dict(spec=("c2", "mini_cheetah-c2", "mini_cheetah-c2", 128, 4, False), knobs=_CLS, seeds={17: 4, 1000: 4}),
    "mck4_cls_L5": dict(spec=("k4", "mini_cheetah-k4", "mini_cheetah-k4", 128, 5, False), knobs=_CLS, seeds={17: 2, 1000: 2}),
    "mck4_reg_L3": dict(spec=("k4", "mini_cheetah-k4", "mini_cheetah-k4", 128, 3, True, 1), knobs=_K1, seeds={17: 4, 1000: 4}),
    "mi_L5": dict(spec=("mi", "quadruped-mi", "", 128, 5, True, 1), knobs=_K1, seeds={17: 5, 1000: 5}),
    "solok4_com_L4": dict(spec=("k4_com", "solo-k4-com", "solo-k4", 128, 4, True, 1), knobs=_K1, seeds={17: 3, 1000: 3, 8193: 3}),
    "soloc2_com_L4": dict(spec=("c2_com", "solo-c2-com", "solo-c2", 128, 4, True, 1), knobs=_K1, seeds={17: 3, 1000: 3}),
    "solos4_com_L5": dict(spec=("s4_com", "solo-s4-com", "", 128, 5, True, 1), knobs=_K1, seeds={17: 3, 1000: 3}),
    # the generic-width engine's own width
    "a1c2_h256_L4": dict(spec=("c2", "a1-c2", "a1-c2", 256, 4, True), knobs=_K1, seeds={17: 3}),
    "solok4_com_h256_L4": dict(spec=("k4_com", "solo-k4-com", "solo-k4", 256, 4, True, 1), knobs=_K1, seeds={17: 3}),
}
for _m in FAMILIES.values():
    _m["program"] = None
gx.MODELS.update(FAMILIES)

H128 = [m for m in FAMILIES if "_h256_" not in m]
REGRESSION = [m for m in H128 if FAMILIES[m]["spec"][5]]
CLASSIFICATION = [m for m in H128 if not FAMILIES[m]["spec"][5]]
BASE_IS_A_DESTINATION = ["a1c2_L5", "mck4_cls_L5", "mi_L5", "solok4_com_L4", "soloc2_com_L4", "solos4_com_L5"]      # (asserted on the host, tests/test_exact_data.py)
REG_CASES = [(m, B) for m in REGRESSION for B in sorted(FAMILIES[m]["seeds"])]
CLS_CASES = [(m, B) for m in CLASSIFICATION for B in sorted(FAMILIES[m]["seeds"])]
GENERIC_CASES = [(m, 17) for m in FAMILIES]
JIT_MODEL, JIT_BATCHES = "a1c2_L5", [17, 1000]
CASES = REG_CASES + CLS_CASES + [c for c in GENERIC_CASES if c[0] not in H128]

ONE_CALL_SETS = [      # (name, plan dtype, switches, compile-time program: False = none, asserted)
    ("bf16", "bf16", {}, False),
    ("bf16 MSHGNN_SLAB=0", "bf16", {"MSHGNN_SLAB": "0"}, False),
    ("bf16 MSHGNN_FUSED=0", "bf16", {"MSHGNN_FUSED": "0"}, False),
    ("bf16 MSHGNN_STASH_NT=1", "bf16", {"MSHGNN_STASH_NT": "1"}, False),
    ("x3", "x3", {}, False),
    ("f32", "f32", {}, False),
]
ROUTE_SETS = [ONE_CALL_SETS[0], ONE_CALL_SETS[4]]
TYPE_LEVEL_SETS = {"a1c2_L4": [s for s in gx.KERNEL_SETS if "MSHGNN_PRUNE" in s[2]]}


def _all_routes(bad, name, e, spec, case, ref, B):
    gx._two_call(bad, name, e, spec, case, ref, B)
    gx._two_phase(bad, name, e, spec, case, ref, B)      # (asserts that the plan has a two-phase step: every family's LDS-resident plan has)
    gx._src_step(bad, name, e, spec, case, ref, B)


@pytest.mark.parametrize("model,B", REG_CASES)
def test_regression_family_is_the_oracle_bit_for_bit_on_every_kernel_set_and_route(monkeypatch, model, B):
    spec, case, ref, stats = gx._reference(model, B)
    bad = []
    for name, dtype, env, program in ONE_CALL_SETS + TYPE_LEVEL_SETS.get(model, []):
        e = gx._engine(monkeypatch, spec, model, dtype, env, program)
        assert not e.generic, f"{model} {name}: not the LDS-resident kernels"
        gx._step(bad, f"{model} B={B} {name}", e, spec, case, ref, B)
        if (name, dtype, env, program) in ROUTE_SETS:
            _all_routes(bad, f"{model} B={B} {name}", e, spec, case, ref, B)
        del e
    print(f"\n{model} B={B}: {stats['zero_decisions']} exact-zero relu pre-activations, {stats['nonzero_grads']} of {stats['grads']} gradient tensors non-zero")
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("model,B", CLS_CASES)
def test_classification_family_is_the_oracle_bit_for_bit(monkeypatch, model, B):
    gx._classification(monkeypatch, model, B, program=False)


@pytest.mark.parametrize("model,B", GENERIC_CASES)
def test_family_through_the_generic_engine_is_the_oracle_bit_for_bit(monkeypatch, model, B):
    """mshgnn_gen.hip on topologies the LDS-resident kernels also take (MSHGNN_ENGINE=generic at hidden 128) and at its own width 256: base sums over
    several rows, mean relations, a decoder on the base nodes."""
    spec, case, ref, _ = gx._reference(model, B)
    bad = []
    for dtype in ("bf16", "x3"):
        e = gx._engine(monkeypatch, spec, model, dtype, {"MSHGNN_ENGINE": "generic"} if spec.hidden == 128 else {}, False)
        assert e.generic, f"{model} {dtype}: not the generic engine"
        if spec.regression:
            gx._step(bad, f"{model} B={B} generic {dtype}", e, spec, case, ref, B)
        gx._two_call(bad, f"{model} B={B} generic {dtype}", e, spec, case, ref, B)
        del e
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("B", JIT_BATCHES)
@pytest.mark.parametrize("dtype", ["bf16", "x3"])
def test_program_compiled_on_demand_is_the_oracle_bit_for_bit(monkeypatch, dtype, B):
    """A1-C2 at 5 layers over the program jit.py compiles for its plan (tests/test_jit_gpu.py pins such a program to the interpreting kernels on random
    data; here it meets the oracle): one-call step, training and evaluation forward, backward."""
    monkeypatch.delenv("MSHGNN_JIT", raising=False)
    spec, case, ref, _ = gx._reference(JIT_MODEL, B)
    e = gx._engine(monkeypatch, spec, JIT_MODEL, dtype, {}, False)
    name = jit.attach_program(e)
    assert name.startswith("JIT_X3_" if dtype == "x3" else "JIT_") and e.specialised == name and (dtype == "x3" or not name.startswith("JIT_X3_"))
    bad = []
    gx._step(bad, f"{JIT_MODEL} B={B} {name}", e, spec, case, ref, B)
    gx._two_call(bad, f"{JIT_MODEL} B={B} {name}", e, spec, case, ref, B)
    assert not bad, "\n".join(bad[:20])
