"""Gradients with respect to the inputs (mshgnn_input_grad, Engine.input_grad, models._EngineFn) against the fp64 oracle BIT FOR BIT, on rounding-free
data (tests/exact_data.py with enc_cover=True: on it dx = m . (dY_enc @ W_enc) is a short sum of exact products in every plan's operand form, and every
input type's dx is non-zero in every 16-column tile -- tests/test_exact_data.py proves that, (a)-(d), on the host for every (model, batch) used here).
A wrong column chunk, a dropped K block, a mis-indexed node row or a missing sign flip is then a failure, where a tolerance could miss it.  On this
data dY_enc and W_enc are bf16 values, so every lo half is zero: the split plan's hi.lo and lo.hi products are pinned bit for bit by
tests/test_x3_exact_gpu.py (wide_gout / wide_dec: dY_enc carries lo halves; wide_enc: W_enc does; split and fp32 plans, the generic engine at hidden 256),
and on random data by the own-operand tests of tests/test_input_grad_gpu.py (helpers.check_input_grad_against_own_operands).

Matrix:
  * A1-C2 at 4 layers (the shallowest depth whose base rows -- 2 nodes, F = 900, 15 column chunks, signed masks -- are live) and at 3 layers (base dead:
    under MSHGNN_POISON_WS=1 its rows must still come out exactly zero), fp32, bf16 and split plans, B in {1, 15, 16, 17, 1000, 8192, 8208} (8192 / 8208:
    36 row tiles per workgroup, runs that start in the middle of a node), after backward(gout), backward_mse and backward(weights=False), fp32 and fp64.
  * The generic engine at hidden 256, 1024 and 2048 (bf16 and split: at 2048 the workgroup's LDS is 65 792 / 131 584 bytes), the padded engine at
    hidden 200 and 1000 (served at 256 and 1024).
  * MiniCheetah-K4 classification at 3 layers through backward(gout) (live joint F = 300 and foot F = 900: 5- and 15-chunk types); after backward_ce
    (softmax: not exact) the same launch against its own operands (helpers.check_input_grad_against_own_operands).
  * One module through _EngineFn, with fp32 and fp64 leaves mixed across types.
The references are the oracle alone: the host proofs live in tests/test_exact_data.py, which runs check_exact on exactly these cases.
"""
from functools import lru_cache

import pytest
import torch

from morphsym_hgnn_amd import engine as eng
from tests import exact_data as xd
from tests import helpers
from tests import test_exact_gpu as gx

pytestmark = pytest.mark.gpu

MODELS = {      # spec arguments (helpers.make_spec) and generator knobs (exact_data.exact_case)
    "a1c2_L4": dict(spec=("c2", "a1-c2", "a1-c2", 128, 4, True), knobs=dict(rel_scales=(1.0,), enc_cover=True)),
    "a1c2_L3": dict(spec=gx.MODELS["a1c2_L3"]["spec"], knobs=dict(gx.MODELS["a1c2_L3"]["knobs"], enc_cover=True)),
    "a1c2_h256_L3": dict(spec=gx.MODELS["a1c2_h256_L3"]["spec"], knobs=dict(gx.MODELS["a1c2_h256_L3"]["knobs"], enc_cover=True)),
    "a1c2_h1024_L3": dict(spec=gx.MODELS["a1c2_h1024_L3"]["spec"], knobs=dict(gx.MODELS["a1c2_h1024_L3"]["knobs"], enc_cover=True)),
    "a1c2_h2048_L3": dict(spec=("c2", "a1-c2", "a1-c2", 2048, 3, True), knobs=dict(rel_scales=(1.0,), enc_cover=True)),
    "a1c2_h200_L3": dict(spec=gx.MODELS["a1c2_h200_L3"]["spec"], knobs=dict(gx.MODELS["a1c2_h200_L3"]["knobs"], enc_cover=True)),
    "a1c2_h1000_L3": dict(spec=("c2", "a1-c2", "a1-c2", 1000, 3, True), knobs=dict(rel_scales=(1.0,), enc_cover=True)),
    "mck4_cls_L3": dict(spec=gx.MODELS["mck4_cls_L3"]["spec"], knobs=dict(gx.MODELS["mck4_cls_L3"]["knobs"], enc_cover=True)),
}
SEED = 3
SEEDS = {("a1c2_L3", 1): 7, ("a1c2_h1024_L3", 70): 5}      # (seeds 3-6 / 3-4 there: no negative symmetry sign meets a non-zero dx)
HETERO_MODELS = ["a1c2_L4", "a1c2_L3"]
BATCHES = [1, 15, 16, 17, 1000, 8192, 8208]
WIDE_CASES = [("a1c2_h256_L3", 300), ("a1c2_h1024_L3", 70), ("a1c2_h2048_L3", 70)]
PADDED_CASES = [("a1c2_h200_L3", 50), ("a1c2_h1000_L3", 50)]
CLS_CASES = [("mck4_cls_L3", 17), ("mck4_cls_L3", 1000)]
MODULE_CASE = ("a1c2_L4", 17)
CASES = ([(m, B) for m in HETERO_MODELS for B in BATCHES] + WIDE_CASES + PADDED_CASES + CLS_CASES + [MODULE_CASE])


def exact_case(model, B):
    spec = helpers.make_spec(*MODELS[model]["spec"])
    return spec, xd.exact_case(spec, B, SEEDS.get((model, B), SEED), **MODELS[model]["knobs"])


@lru_cache(maxsize=2)
def _reference(model, B):
    spec, case = exact_case(model, B)
    gout = case["gout_mse"] if case.get("gout_mse") is not None else case["gout"]
    ref = xd.reference(spec, case, gout, input_grads=True)
    ref["gout"] = gout
    return spec, case, ref


def _engine(monkeypatch, spec, dtype, poison=False):
    for k in gx.SWITCHES + ("MSHGNN_POISON_WS",):
        monkeypatch.delenv(k, raising=False)
    if poison:
        monkeypatch.setenv("MSHGNN_POISON_WS", "1")
    return eng.make_engine(spec, dtype)


def _compare_dx(bad, what, e, flat, ref, B, dtypes):
    for dt in dtypes:
        got = e.input_grad(B, flat, dtype=dt)
        torch.cuda.synchronize()
        for t, g in got.items():
            assert g.dtype == dt and g.shape == ref["xgrads"][t].shape
            d = xd.first_difference(g, ref["xgrads"][t])
            if d is not None:
                bad.append(f"{what} {str(dt)[6:]} dx[{t}]: {d}")


def _routes(bad, what, e, spec, case, ref, B):
    """backward(gout) (fp32 and fp64 dx), backward_mse (fp32) and backward(weights=False) (fp64), each after a fresh training forward."""
    flat = eng.flatten_params(spec, case["params"], e.device)
    xs = e.cast_inputs(case["x"])
    gout = ref["gout"].to(e.device, torch.float32).contiguous()
    e.forward(xs, flat, B, training=True)
    e.backward(xs, flat, gout, B)
    _compare_dx(bad, f"{what} backward", e, flat, ref, B, (torch.float32, torch.float64))
    if case.get("y") is not None:
        out = e.forward(xs, flat, B, training=True)
        e.backward_mse(xs, flat, out, case["y"].to(e.device, torch.float32).contiguous(), B)
        _compare_dx(bad, f"{what} backward_mse", e, flat, ref, B, (torch.float32,))
    e.forward(xs, flat, B, training=True)
    assert e.backward(xs, flat, gout, B, weights=False) is None
    _compare_dx(bad, f"{what} backward(weights=False)", e, flat, ref, B, (torch.float64,))


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("model", HETERO_MODELS)
def test_hetero_plans_input_grad_is_the_oracle_bit_for_bit(monkeypatch, model, B):
    spec, case, ref = _reference(model, B)
    live_base = bool(spec.node_liveness()[1][0]["base"])
    assert live_base == (model == "a1c2_L4") and (float(ref["xgrads"]["base"].abs().max()) > 0) == live_base
    bad = []
    for dtype in ("f32", "bf16", "x3"):
        e = _engine(monkeypatch, spec, dtype, poison=not live_base)
        assert not e.generic
        _routes(bad, f"{model} B={B} {dtype}", e, spec, case, ref, B)
        del e
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("model,B", WIDE_CASES + PADDED_CASES)
def test_generic_and_padded_engines_input_grad_is_the_oracle_bit_for_bit(monkeypatch, model, B):
    spec, case, ref = _reference(model, B)
    bad = []
    for dtype in ("bf16", "x3"):
        e = _engine(monkeypatch, spec, dtype)
        assert e.generic and getattr(e, "padded", False) == (spec.hidden % 128 != 0)
        _routes(bad, f"{model} B={B} {dtype}", e, spec, case, ref, B)
        del e
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("model,B", CLS_CASES)
def test_classification_input_grad_is_the_oracle_bit_for_bit(monkeypatch, model, B):
    spec, case, ref = _reference(model, B)
    assert [t for t in spec.node_types if float(ref["xgrads"][t].abs().max()) > 0] == ["joint", "foot"]
    bad = []
    for dtype in ("bf16", "x3"):
        e = _engine(monkeypatch, spec, dtype)
        assert not e.generic
        _routes(bad, f"{model} B={B} {dtype}", e, spec, case, ref, B)
        # backward_ce: its softmax gradient is not exact, so the same launch is held to the product of the engine's own operands
        flat = eng.flatten_params(spec, case["params"], e.device)
        xs = e.cast_inputs(case["x"])
        out = e.forward(xs, flat, B, training=True)
        labels = torch.randint(0, 2, (B, e.n_out), generator=torch.Generator().manual_seed(B)).to(e.device, torch.int32)
        e.backward_ce(xs, flat, out, labels, B)
        for dt in (torch.float32, torch.float64):
            helpers.check_input_grad_against_own_operands(e, spec, case["params"], B, e.input_grad(B, flat, dtype=dt))
        del e
    assert not bad, "\n".join(bad[:20])


def test_module_input_grad_with_mixed_leaf_dtypes_is_the_oracle_bit_for_bit(monkeypatch):
    """models._EngineFn: fp64 base and foot leaves, an fp32 joint leaf (one launch per dtype), each given its gradient in its own dtype."""
    from tests.test_models import _build
    model, B = MODULE_CASE
    spec, case, ref = _reference(model, B)
    for k in gx.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("MSHGNN_DTYPE", "bf16")
    args = MODELS[model]["spec"]
    m = _build({"kind": args[0], "cfg": args[2], "hidden": args[3], "layers": args[4], "regression": args[5], "grf": 3}, spec).cuda()
    ei = {k: v.cuda() for k, v in spec.topology.edge_index_dict(B).items()}
    with torch.no_grad():
        m(x_dict={k: v.cuda().clone() for k, v in case["x"].items()}, edge_index_dict=ei)
    m.load_state_dict(case["params"])
    dts = {"base": torch.float64, "joint": torch.float32, "foot": torch.float64}
    xl = {t: case["x"][t].to("cuda", dts[t]).clone().requires_grad_(True) for t in spec.node_types}
    out = m(x_dict=xl, edge_index_dict=ei)
    out.backward(ref["gout"].to(out.device, out.dtype).reshape(out.shape))
    bad = []
    for t in spec.node_types:
        g = xl[t].grad
        assert g is not None and g.dtype == dts[t] and g.shape == xl[t].shape, t
        d = xd.first_difference(g, ref["xgrads"][t])
        if d is not None:
            bad.append(f"module dx[{t}]: {d}")
    assert not bad, "\n".join(bad)
