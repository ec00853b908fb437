"""The fused cross-entropy steps against the fp64 oracle BIT FOR BIT: step_ce and backward_ce of every engine on cases whose softmax gradient is itself exact.

tests/test_exact_gpu.py pins the classification models' logits and backward(gout) with a hand-made gout.  The softmax arithmetic in front of that gout exists in
five copies -- the `ce` branch of decoder_tail_impl (csrc/mshgnn_device.hpp: the bf16 one-call step on the slab and the 8-wave step kernels, the split plan's step
tail), k_dec_bwd (csrc/mshgnn.hip: backward_ce on the bf16 and fp32 plans, MSHGNN_FUSED=0), the split plan's decoder backward (csrc/mshgnn_x3.hip), k_gdec_bwd
(csrc/mshgnn_gen.hip) and the loss tail of k_mlp_stack (csrc/mshgnn_mlp.hip) -- each with its own label indexing, inv_n, masks and loss partials, and the tolerance
tests scale their bound by the largest gradient.  All five evaluate m = fmaxf(l0, l1); e_i = expf(l_i - m); se = e0 + e1; g_i = (e_i / se - onehot_i) * inv_n, which
rounds nothing on a tie (e = 1, 1; se = 2) and on a saturated pair (|l0 - l1| >= 128: the smaller exponential is exactly 0).  exact_data.ce_case multiplies the
decoder of a rounding-free case by 2^7, so that every (window, foot) is one or the other, draws labels, and evaluates that formula on the host; with B * n_out a power
of two the gradient is 0, +-1 or +-2 units of 0.5 * inv_n and check_exact_ce proves closure and coverage for it (tests/test_exact_data.py, for every case of this
file).  The reference gradients are the oracle's backward of that gout (an fp64 cross entropy keeps e^-128 / N where fp32 has 0: at most 6.5e-57 away).

Asserted per case: the logits, every hidden state the plan computes, every gradient (exact zeros included) are the oracle's bits; the loss equals the fp64 mean cross
entropy exactly where the case has no ties (every term is 0 or a multiple of 128), and within (gamma_{n+4} + 2^-23) of it where it has (an fp32 sum of n non-negative
terms in any fixed order, logf(2) rounded once per tie; the measured ratio is printed).  Every step runs twice into a gradient buffer pre-filled with a sentinel: a
parameter the step never writes shows, and both runs give the same bits, the loss included (its partials are summed in a fixed order, without atomics).

Matrix (seed, wrong share, label seed and ties per case: CE_CASES; counts and sums of |terms| are printed by tests/test_exact_data.py):
  * MiniCheetah-K4 classification at 3 layers, hidden 128 (no compile-time program), at B in {2, 8, 16, 32, 1024}; launch-table rows as tests/test_resident_pick.py
    names them (test_plans_without_a_program_and_the_switches, test_the_split_plan), every B being at most one tile per CU:
      bf16, MSHGNN_STASH_NT=1, MSHGNN_PRUNE=0   k_stack_step<bf16> (8 waves; decoder_tail_impl)
      MSHGNN_SLAB=0                             k_stack_step<bf16>
      MSHGNN_SLAB=2                             k_slab_step<bf16,NM,HB> of the plan at every batch (the slab tail, which is otherwise reached past 4096 windows)
      MSHGNN_FUSED=0, f32                       k_layer_fwd<T>, k_dec_bwd, k_layer_bwd<T>
      x3, x3 MSHGNN_PRUNE=0                     k_stack_step_x3<ALIAS> (decoder_tail_impl, SPLIT)
    4 windows: LEFT_OUT.  At 8 and 1024 windows on the bf16 and x3 defaults also forward + backward_ce (k_stack_fwd + k_dec_bwd / the split plan's decoder backward) and the fp64-source
    step (engine.WideInputs).  Classification has no two-phase step (the engine has step_mse_phase only).
  * MSHGNN_STEP_CHUNK=64 at 1024 windows, bf16 and x3: sixteen sub-steps, each with the whole batch's inv_n.
  * MiniCheetah-C2 classification at 4 layers and MiniCheetah-K4 classification at 5 layers (live base nodes) at 16 and 1024 windows, on the kernel sets of
    tests/test_exact_families_gpu.py.
  * The generic engine (k_gdec_bwd), bf16 and split arithmetic, step_ce and forward + backward_ce: hidden 256 and 384 at 16 and 1024 windows, hidden 128 forced with
    MSHGNN_ENGINE=generic at 16.
  * The MLP baselines: tests/test_mlp_exact_gpu.py's engines on mlp_reference.ce_case (test_mlp_step_ce_is_the_reference_bit_for_bit).
LEFT_OUT lists what no seed of 1..12 closes, with the failing condition.
Not possible: a batch size that is not a power of two -- inv_n = fl32(1 / (4 B)) then has 24 significant bits and the first bf16 store of dX_L rounds it; ragged last
tiles after full ones (17, 8193) stay with the tolerance tests.  Partially filled tiles are covered (2, 8).  An 8192-window case would cost 17-29 s of host reference:
MSHGNN_SLAB=2 reaches its kernel.
"""
from functools import lru_cache

import pytest
import torch

from morphsym_hgnn_amd import engine as eng
from tests import exact_data as xd
from tests import test_exact_families_gpu as fam
from tests import test_exact_gpu as gx

pytestmark = pytest.mark.gpu

_CLS = dict(rel_scales=(1.0,), bias_range=(0, 1))
gx.MODELS.update({      # the generic engine's own widths
    "mck4_cls_h256_L3": dict(spec=("k4", "mini_cheetah-k4", "mini_cheetah-k4", 256, 3, False), knobs=_CLS, program=None),
    "mck4_cls_h384_L3": dict(spec=("k4", "mini_cheetah-k4", "mini_cheetah-k4", 384, 3, False), knobs=_CLS, program=None),
})
# (model, B): seed, wrong share, label seed, ties, the decoder row ce_case negates -- what the host search over seeds 1..12 found (tests/test_exact_data.py proves each)
CE_CASES = {
    ("mck4_cls_L3", 2): dict(seed=11, wrong_share=0.6, label_seed=24, ties=False),
    ("mck4_cls_L3", 8): dict(seed=3, wrong_share=0.5, label_seed=2, ties=True),
    ("mck4_cls_L3", 16): dict(seed=3, wrong_share=0.5, label_seed=0, ties=True),
    ("mck4_cls_L3", 32): dict(seed=3, wrong_share=0.5, label_seed=0, ties=True),
    ("mck4_cls_L3", 1024): dict(seed=3, wrong_share=0.5, label_seed=0, ties=True),
    # the families: at the seeds that close check_exact the decoder's two rows have opposite signs and l0 - l1 one sign in every row of the batch, which (ii)
    # refuses; with row 1 negated (flip_row: no magnitude changes) both signs occur, and ties with them.  At 1024 windows the weight-gradient sums of |terms| pass
    # 2^24 units above a wrong share of about 1/5 (the factor 128 costs 7 of the 24 bits).
    ("mcc2_cls_L4", 16): dict(seed=7, wrong_share=0.5, label_seed=0, ties=True, flip_row=1),
    ("mcc2_cls_L4", 1024): dict(seed=7, wrong_share=0.125, label_seed=0, ties=True, flip_row=1),
    ("mck4_cls_L5", 16): dict(seed=11, wrong_share=0.5, label_seed=0, ties=False),
    ("mck4_cls_L5", 1024): dict(seed=2, wrong_share=0.125, label_seed=0, ties=True, flip_row=1),
    ("mck4_cls_h256_L3", 16): dict(seed=7, wrong_share=0.5, label_seed=0, ties=True),
    ("mck4_cls_h256_L3", 1024): dict(seed=7, wrong_share=0.5, label_seed=0, ties=True),
    ("mck4_cls_h384_L3", 16): dict(seed=5, wrong_share=0.5, label_seed=0, ties=True),
    ("mck4_cls_h384_L3", 1024): dict(seed=5, wrong_share=0.5, label_seed=0, ties=True),
}
# What no seed of 1..12 closes.  It is the coverage this file asks of a case, not the kernels, that excludes 16-row cases: 4 windows x 4 feet have to hold, at once, both
# labels on every foot, right and wrong rows with both signs of l0 - l1, and enough non-zero output gradients for every live parameter gradient to be non-zero (c).
# Searched: wrong shares 1/2 and 3/4 with label seeds 0..99 (3/4: 0..399), 1/2 with flip_row=1 and label seeds 0..40.  Partially filled tiles run at 2 and 8 windows.
LEFT_OUT = {
    ("mck4_cls_L3", 4): "16 rows: coverage (c) (the gradients of the layer-1 base -> joint relation are zero) or (ii) (a foot with one label, a regime with one sign)",
}
LDS_MODEL = "mck4_cls_L3"
LDS_BATCHES = [2, 8, 16, 32, 1024]
ROUTE_BATCHES = [8, 1024]
LDS_SETS = [s for s in gx.KERNEL_SETS if s[0] in ("bf16", "bf16 MSHGNN_SLAB=0", "bf16 MSHGNN_FUSED=0", "bf16 MSHGNN_STASH_NT=1", "x3 MSHGNN_SPEC=1", "f32",
                                                  "bf16 MSHGNN_PRUNE=0", "x3 MSHGNN_PRUNE=0")] + [("bf16 MSHGNN_SLAB=2", "bf16", {"MSHGNN_SLAB": "2"}, False)]
LDS_SETS = [(n, d, env, None if p is None else False) for n, d, env, p in LDS_SETS]      # (the model has no compile-time program: asserted, but under MSHGNN_PRUNE=0)
ROUTE_SETS = [s for s in LDS_SETS if s[0] in ("bf16", "x3 MSHGNN_SPEC=1")]
FAMILY_CASES = [c for c in CE_CASES if c[0] in fam.CLASSIFICATION]
GENERIC_CASES = [c for c in CE_CASES if "_h256_" in c[0] or "_h384_" in c[0]] + [(LDS_MODEL, 16)]
SENTINEL = 12345.0


@lru_cache(maxsize=3)
def _reference(model, B):
    spec = gx._spec(model)
    c = CE_CASES[(model, B)]
    case = xd.ce_case(spec, B, c["seed"], c["wrong_share"], c["label_seed"], flip_row=c.get("flip_row"), **gx.MODELS[model]["knobs"])
    stats = {}
    ref = xd.check_exact_ce(spec, case, c["ties"], stats=stats)
    ref["hidden"] = [h.float() for h in ref["hidden"]]
    return spec, case, ref, stats


def _compare_loss(bad, what, loss, case, ref):
    bound = xd.ce_loss_bound(case)
    err = abs(float(loss) - ref["loss"]) / ref["loss"]
    if bound > 0:
        print(f"\n{what}: loss rel err {err:.3e} = {err / bound:.3e} of the bound {bound:.3e}")
    if not err <= bound:
        bad.append(f"{what}: loss {float(loss)!r}, reference {ref['loss']!r}: rel err {err:.3e} > {bound:.3e}")


def _twice(bad, what, run):
    """`run()` -> (out, loss, grads), twice, each into a gradient buffer full of the sentinel: the first run's results, after requiring the second's bits to be
    the same -- the loss included: every kernel run here sums its loss partials in a fixed order (k_finalize, k_gfinalize, k_mlp_reduce)."""
    res = []
    for _ in range(2):
        out, loss, g = run()
        torch.cuda.synchronize()
        res.append((out.clone(), loss.clone(), g.clone()))
    for name, a, b in zip(("out", "loss", "grads"), res[0], res[1]):
        if not torch.equal(a, b):
            bad.append(f"{what}: a second run gives other bits in {name}")
    return res[0]


def _grad_buffer(e, spec):
    return torch.full((spec.flat_size(),), SENTINEL, dtype=torch.float32, device=e.device)


def _labels(e, case):
    return case["labels"].to(e.device).contiguous()


def _step(bad, name, e, spec, case, ref, B, hidden=True, wide=False):
    flat = eng.flatten_params(spec, case["params"], e.device)
    xs = e.cast_inputs({t: v.to(e.device) for t, v in case["x"].items()} if wide else case["x"])
    assert isinstance(xs, eng.WideInputs) == wide
    what = f"{name} step_ce" + (" (fp64 source)" if wide else "")
    out, loss, g = _twice(bad, what, lambda: e.step_ce(xs, flat, _labels(e, case), B, grad_flat=_grad_buffer(e, spec)))
    gx._compare(bad, f"{what} out", out, ref["out"])
    if hidden:      # (a one-call step does not stash X_L: the logits and the decoder's gradients cover it)
        gx._compare_hidden(bad, what, e, spec, ref, B, range(spec.num_layers))
    gx._compare_grads(bad, what, spec, g, ref)
    _compare_loss(bad, what, loss, case, ref)


def _two_call(bad, name, e, spec, case, ref, B):
    flat = eng.flatten_params(spec, case["params"], e.device)
    xs = e.cast_inputs(case["x"])
    what = f"{name} forward + backward_ce"

    def run():
        out = e.forward(xs, flat, B, training=True).clone()
        loss, g = e.backward_ce(xs, flat, out, _labels(e, case), B, grad_flat=_grad_buffer(e, spec))
        return out, loss, g
    out, loss, g = _twice(bad, what, run)
    gx._compare(bad, f"{what} out", out, ref["out"])
    gx._compare_hidden(bad, what, e, spec, ref, B, range(spec.num_layers + 1))
    gx._compare_grads(bad, what, spec, g, ref)
    _compare_loss(bad, what, loss, case, ref)


@pytest.mark.parametrize("B", LDS_BATCHES)
def test_one_call_cross_entropy_step_is_the_oracle_bit_for_bit_on_every_kernel_set(monkeypatch, B):
    spec, case, ref, stats = _reference(LDS_MODEL, B)
    bad = []
    for name, dtype, env, program in LDS_SETS:
        e = gx._engine(monkeypatch, spec, LDS_MODEL, dtype, env, program)
        assert not e.generic
        _step(bad, f"{LDS_MODEL} B={B} {name}", e, spec, case, ref, B)
        if B in ROUTE_BATCHES and (name, dtype, env, program) in ROUTE_SETS:
            _two_call(bad, f"{LDS_MODEL} B={B} {name}", e, spec, case, ref, B)
            _step(bad, f"{LDS_MODEL} B={B} {name}", e, spec, case, ref, B, wide=True)
        del e
    print(f"\n{LDS_MODEL} B={B}: ties / right / wrong = {stats['ties']} / {stats['right']} / {stats['wrong']}, backward sums of |terms| <= {stats['bwd_sum_bound']:.2e}")
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("dtype", ["bf16", "x3"])
def test_chunked_cross_entropy_step_is_the_oracle_bit_for_bit(monkeypatch, dtype):
    """MSHGNN_STEP_CHUNK=64 at 1024 windows: sixteen sub-steps accumulating into one gradient and one loss, each dividing by the whole batch's row count."""
    B = 1024
    spec, case, ref, _ = _reference(LDS_MODEL, B)
    e = gx._engine(monkeypatch, spec, LDS_MODEL, dtype, {"MSHGNN_STEP_CHUNK": "64"}, None)
    bad = []
    _step(bad, f"{dtype} chunked", e, spec, case, ref, B, hidden=False)      # (the workspace holds the last sub-step only)
    assert not bad, "\n".join(bad[:20])
    # it really ran as sub-steps: the engine refuses to read the stash, and what sits where a whole-batch step would have left X_0 is not X_0
    with pytest.raises(RuntimeError, match="sub-steps"):
        e.hidden_state(B, 0)

    class WholeLayout:
        def hidden_state(self, B, l):
            return e._act_tensor(e.layout(B, True).x[l], B)
    stale = []
    gx._compare_hidden(stale, "whole-batch layout", WholeLayout(), spec, ref, B, [0])
    assert stale, "X_0 of the whole batch is in the workspace: the step did not run as sub-steps"


@pytest.mark.parametrize("model,B", FAMILY_CASES)
def test_family_cross_entropy_step_is_the_oracle_bit_for_bit(monkeypatch, model, B):
    spec, case, ref, _ = _reference(model, B)
    bad = []
    for name, dtype, env, program in fam.ONE_CALL_SETS:
        e = gx._engine(monkeypatch, spec, model, dtype, env, program)
        assert not e.generic
        _step(bad, f"{model} B={B} {name}", e, spec, case, ref, B)
        del e
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("model,B", GENERIC_CASES)
def test_generic_engine_cross_entropy_is_the_oracle_bit_for_bit(monkeypatch, model, B):
    """k_gdec_bwd's cross-entropy branch in bf16 and split arithmetic: step_ce, then forward + backward_ce."""
    spec, case, ref, stats = _reference(model, B)
    assert stats["aggregates_not_bf16"] == []
    bad = []
    for dtype in ("bf16", "x3"):
        e = gx._engine(monkeypatch, spec, model, dtype, {"MSHGNN_ENGINE": "generic"} if spec.hidden == 128 else {}, False)
        assert e.generic, f"{model} {dtype}: not the generic engine"
        _step(bad, f"{model} B={B} generic {dtype}", e, spec, case, ref, B)
        _two_call(bad, f"{model} B={B} generic {dtype}", e, spec, case, ref, B)
        del e
    assert not bad, "\n".join(bad[:20])


# ---------------------------------------------------------------------------------------------------
# the MLP baselines (the loss tail of k_mlp_stack)
# ---------------------------------------------------------------------------------------------------
from tests import mlp_reference as mr      # noqa: E402

MLP_CASES = [c[:2] for c in mr.CE_MATRIX]


@lru_cache(maxsize=2)
def _mlp_reference(shape, B):
    _, _, seed, share, ties = next(c for c in mr.CE_MATRIX if c[:2] == (shape, B))
    case = mr.ce_case(shape, B, seed, share)
    return case, mr.check_exact_ce(case, ties)


@pytest.mark.parametrize("shape,B", MLP_CASES, ids=[f"in{s[0]}_T{s[1]}_h{s[2]}_L{s[3]}_o{s[4]}_B{B}" for s, B in MLP_CASES])
def test_mlp_step_ce_is_the_reference_bit_for_bit(shape, B):
    """MLPEngine.step_ce in bf16 and x3 (every operand of the case is a bf16 value: the split plan's lo halves are zero and its sums the same exact ones),
    dense and (bf16) from the resident series with the same labels: logits, the input-layer stash and every dW / db are fp64's bits, the loss as for the graph models."""
    from morphsym_hgnn_amd import engine, windows
    in_channels, T, hidden, L, out_channels = shape
    dev = torch.device("cuda:0")
    case, ref = _mlp_reference(shape, B)
    dims = (in_channels, hidden, out_channels, L)
    labels = case["labels"].to(dev).contiguous()
    bad = []
    for dtype in ("bf16", "x3"):
        e = engine.MLPEngine(in_channels, hidden, out_channels, L, dtype, "cuda:0")
        flat = mr.flatten(case["params"]).float().to(dev)
        x = e.cast_input(case["x"])
        ws = torch.full((e.workspace_bytes(B, True),), 0xFF, dtype=torch.uint8, device=dev)
        starts = case["starts"].to(dev)
        routes = [(f"{dtype} step_ce", lambda: e.step_ce(x, flat, labels, grad_flat=grad(), workspace=ws))]
        if dtype == "bf16":      # (the split plan has no series form: tests/test_mlp_x3_gpu.py)
            store = windows.SequenceStore({"s": case["series"].numpy()}, windows.mlp_recipe([("s", list(range(in_channels // T)))], T), dtype="bf16", device=dev)
            assert e._series_ok(store)
            routes.append(("bf16 step_ce_series", lambda: e.step_ce_series(store, starts, flat, grad_flat=grad(), workspace=ws, targets=labels)[1:]))

        def grad():
            return torch.full((e.n_flat,), SENTINEL, dtype=torch.float32, device=dev)
        for what, run in routes:
            out, loss, g = _twice(bad, what, run)
            bad += mr.compare(ref, out.view(B, out_channels), e.stash(B, 1, ws), mr.unflatten(g, mr.layer_dims(*dims)), what + ": ")
            _compare_loss(bad, what, loss, case, ref)
        del e
    assert not bad, "\n".join(bad[:20])
