"""Host tests of the robust-loss references (tests/loss_reference.py) and of the argument checks that return before a device is touched.

  * the fp64 references against torch.nn.functional.l1_loss / huber_loss (fp64, mean) at 1e-12, values and gradients, with d == 0, |d| == delta and both signs;
  * the fp32 mirror against the fp64 references (a few fp32 ulps of the gradient's scale), and its special values: sign(0) = 0, NaN in -> NaN out;
  * the exact-case generator: delta exists for every batch size the issue names, the cases the GPU tests use pass exact_data.check_exact with their coverage;
  * the damaged variants are refused by `check_loss`, the undamaged values accepted;
  * the C-ABI: null plans, unknown kinds and bad deltas are MSHGNN_EINVAL with the function's own name.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from morphsym_hgnn_amd import engine as eng
from tests import helpers
from tests import loss_reference as lr

F32 = np.float32


def _data(n=257, seed=0, delta=0.75):
    g = torch.Generator().manual_seed(seed)
    out = torch.randn(n, generator=g, dtype=torch.float64)
    y = torch.randn(n, generator=g, dtype=torch.float64)
    y[0] = out[0]                         # d == 0
    y[1], y[2] = out[1] - delta, out[2] + delta      # |d| == delta (up to the rounding of the subtraction), both signs
    out[3], y[3] = 0.0, -delta            # d == delta exactly
    out[4], y[4] = 0.0, delta             # d == -delta exactly
    y[5], y[6] = out[5] - 3 * delta, out[6] + 3 * delta
    return out, y


@pytest.mark.parametrize("kind,delta", [("l1", 1.0), ("huber", 0.75), ("huber", 0.0249)])
def test_fp64_references_are_torchs_losses(kind, delta):
    out, y = _data(delta=delta)
    leaf = out.clone().requires_grad_(True)
    want = torch.nn.functional.l1_loss(leaf, y) if kind == "l1" else torch.nn.functional.huber_loss(leaf, y, delta=delta)
    want.backward()
    want = want.detach()
    loss, g = lr.ref64(kind, out, y, delta)
    assert abs(loss - float(want)) <= 1e-12 * abs(float(want))
    assert float((g - leaf.grad).abs().max()) <= 1e-12 * float(leaf.grad.abs().max())
    assert float(g[0]) == 0.0
    assert abs(float(lr.terms64(kind, out, y, delta).sum()) / out.numel() - loss) <= 1e-12 * abs(loss)


@pytest.mark.parametrize("kind,delta", [("mse", 1.0), ("l1", 1.0), ("huber", 0.75)])
def test_fp32_mirror_follows_the_fp64_reference(kind, delta):
    out, y = _data(n=1000, seed=1, delta=delta)
    o32, y32 = out.numpy().astype(F32), y.numpy().astype(F32)
    g, term = lr.mirror32(kind, o32, y32, delta=delta)
    loss64, g64 = lr.ref64(kind, torch.from_numpy(o32.astype(np.float64)), torch.from_numpy(y32.astype(np.float64)), float(F32(delta)))
    # gradient: one rounding of d (exact here or 1/2 ulp), one or two multiplications: 3 units of 2^-24 relative to the largest gradient
    assert float(np.abs(g.astype(np.float64) - g64.numpy()).max()) <= 3 * 2.0 ** -24 * float(g64.abs().max())
    assert abs(float(term.astype(np.float64).sum()) / o32.size - loss64) <= 4 * 2.0 ** -24 * loss64
    assert g.dtype == F32 and term.dtype == F32


def test_mirror_special_values():
    o = np.array([1.0, 1.0, np.nan, 0.0], dtype=F32)
    t = np.array([1.0, 3.0, 0.0, -0.0], dtype=F32)
    for kind in ("l1", "huber"):
        g, term = lr.mirror32(kind, o, t, delta=0.5)
        assert g[0] == 0 and term[0] == 0 and g[3] == 0
        assert np.isnan(g[2]) and np.isnan(term[2])
        assert not np.isnan(g[[0, 1, 3]]).any()
    assert lr.mirror32("l1", o, t)[0][1] == -F32(0.25)
    assert lr.mirror32("huber", o, t, delta=0.5)[0][1] == F32(-0.5) * F32(0.25)


@pytest.mark.parametrize("B", [1, 2, 3, 16, 17, 100, 127, 1000, 1024, 8193])
def test_huber_delta_exists_at_every_batch_size(B):
    n = 12 * B
    d = lr.huber_delta(n)
    assert F32(F32(d) * lr.inv_n32(n)) == F32(2.0 ** -13)
    assert abs(d - 2.0 ** -13 * n) <= 2.0 ** -22 * d


CASES = [      # (name, spec arguments, batch, kind, seed): the cases of tests/test_loss_exact_gpu.py are these and their neighbours
    ("a1c2 huber", ("c2", "a1-c2", "a1-c2", 128, 3, True, 3), 17, "huber", 3),
    ("a1c2 grf1 l1", ("c2", "a1-c2", "a1-c2", 128, 3, True, 1), 16, "l1", 4),
]


@pytest.mark.parametrize("name,spec_args,B,kind,seed", CASES)
def test_exact_cases_close_and_cover_every_class(name, spec_args, B, kind, seed):
    spec = helpers.make_spec(*spec_args)
    case = lr.robust_case(spec, B, seed, kind, rel_scales=(1.0,))
    stats = {}
    ref = lr.check_robust(spec, case, stats=stats)
    names = lr.HUBER_CLASSES if kind == "huber" else lr.L1_CLASSES
    counts = np.bincount(case["classes"], minlength=len(names))
    assert (counts > 0).all(), dict(zip(names, counts))
    # the gradient handed to the oracle is the mirror's, on the grid the closure proofs assume
    g = case["gout_reg"].numpy()
    unit = 2.0 ** -13 if kind == "huber" else float(lr.inv_n32(g.size))
    assert set(np.unique(g / unit)) <= {-1.0, -0.5, 0.0, 0.5, 1.0}
    bad = lr.check_loss(kind, ref["out"].numpy(), case["y"].numpy(), lr.mirror32(kind, ref["out"].numpy(), case["y"].numpy(), delta=case["delta"])[0],
                        ref["loss"], delta=case["delta"])
    assert not bad, bad
    print(f"\n{name} B={B}: classes {dict(zip(names, counts))}, delta {case['delta']!r}, loss {ref['loss']!r}, {stats['nonzero_grads']} of {stats['grads']} gradients non-zero")


@pytest.mark.parametrize("kind,delta", [("l1", 1.0), ("huber", 0.4)])
def test_checker_refuses_every_damaged_variant(kind, delta):
    out, y = _data(n=96, seed=2, delta=delta)
    o32, y32 = out.numpy().astype(F32), y.numpy().astype(F32)
    g, term = lr.mirror32(kind, o32, y32, delta=delta)
    loss = float(term.astype(np.float64).sum()) / o32.size
    assert lr.check_loss(kind, o32, y32, g, loss, delta=delta) == []
    variants = lr.damaged_variants(kind, o32, y32, delta=delta, chunk=32)
    want = {"the factor 2 of MSE left in", "inv_n of the chunk", "loss term of the wrong branch"}
    want |= {"gradient not clamped", "clamp at delta / 2"} if kind == "huber" else {"sign(0) = 1"}
    assert set(variants) == want
    for name, (gv, lv) in variants.items():
        assert lr.check_loss(kind, o32, y32, gv, lv, delta=delta), f"{kind}: the checker accepts '{name}'"


def test_python_side_checks_of_kind_and_delta():
    assert eng.reg_loss_code("mse", 5.0) == (0, 1.0) and eng.reg_loss_code("l1") == (1, 1.0) and eng.reg_loss_code("huber", 0.25) == (2, 0.25)
    for kind, delta in (("smooth_l1", 1.0), ("huber", 0.0), ("huber", -1.0), ("huber", float("inf")), ("huber", float("nan"))):
        with pytest.raises(ValueError):
            eng.reg_loss_code(kind, delta)


def test_cabi_argument_checks_return_before_a_device_is_touched():
    lib = eng.load_library()
    kind, delta = C.c_int32(7), C.c_float(7.0)
    for name, args in (("mshgnn_plan_set_regression_loss", (None, 0, 1.0)), ("mshgnn_mlp_set_regression_loss", (None, 2, 1.0)),
                       ("mshgnn_plan_get_regression_loss", (None, C.byref(kind), C.byref(delta))),
                       ("mshgnn_mlp_get_regression_loss", (None, C.byref(kind), C.byref(delta)))):
        assert getattr(lib, name)(*args) == -1, name      # MSHGNN_EINVAL
        assert name in lib.mshgnn_last_error().decode()
    assert (kind.value, delta.value) == (7, 7.0)      # nothing written
    fake = 4096      # never dereferenced: every refusal below comes before the launch
    for args, word in (((None, fake, 8, 0, 1.0, fake, None, fake, None), "mshgnn_regression_loss"),
                       ((fake, fake, 0, 0, 1.0, fake, None, fake, None), "mshgnn_regression_loss"),
                       ((fake, fake, 8, 3, 1.0, fake, None, fake, None), "kind"),
                       ((fake, fake, 8, -1, 1.0, fake, None, fake, None), "kind"),
                       ((fake, fake, 8, 2, 0.0, fake, None, fake, None), "delta"),
                       ((fake, fake, 8, 2, -2.0, fake, None, fake, None), "delta"),
                       ((fake, fake, 8, 2, float("inf"), fake, None, fake, None), "delta"),
                       ((fake, fake, 8, 2, float("nan"), fake, None, fake, None), "delta"),
                       ((fake, fake, 8, 1, 1.0, fake, None, fake + 8, None), "aligned")):
        assert lib.mshgnn_regression_loss(*args) != 0, args
        msg = lib.mshgnn_last_error().decode()
        assert "mshgnn_regression_loss" in msg and word in msg, (args, msg)
    assert lib.mshgnn_regression_loss_scratch_bytes(0) == 0
    assert 0 < lib.mshgnn_regression_loss_scratch_bytes(1) == lib.mshgnn_regression_loss_scratch_bytes(1 << 30) <= 1040


def test_models_and_wrappers_refuse_a_classification_model_on_the_host():
    from morphsym_hgnn_amd import models
    m = models.MLP(24, 128, 8, 3, regression=False)
    with pytest.raises(ValueError):
        m.set_regression_loss("huber", 1.0)
    r = models.MLP(24, 128, 4, 3, regression=True)
    assert r.regression_loss == ("mse", 1.0)
    assert r.set_regression_loss("huber", 0.5).regression_loss == ("huber", 0.5)
    assert r.set_regression_loss("l1", 9.0).regression_loss == ("l1", 1.0)
    with pytest.raises(ValueError):
        r.set_regression_loss("huber", 0.0)
    assert r.regression_loss == ("l1", 1.0)
