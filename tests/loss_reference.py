"""References for the robust regression losses (L1, Huber) of the fused steps and of mshgnn_regression_loss (test infrastructure, host only).

  * fp64 references of both losses and their gradients (`l1_ref64`, `huber_ref64`): torch.nn.functional.l1_loss / huber_loss, mean reduction, pinned to them
    at 1e-12 by tests/test_loss_reference.py.
  * `mirror32`: the kernels' expressions (csrc/mshgnn_device.hpp reg_loss_terms, include/mshgnn.h) in numpy float32, every operation rounded on its own, left
    to right -- the gradient a kernel stores must be these bits on ANY data.
  * `robust_case`: rounding-free step data.  It builds on exact_data.exact_case(..., mse=False) and hands the loss gradient to exact_data.check_exact(spec,
    case, gout=...), so the closure and coverage proofs there apply; the targets are chosen so that the fp32 loss gradient is a short dyadic number:
      Huber, any n: delta is the fp32 value next to 2 * 2^-14 * n with fl32(delta * inv_n) == 2 * 2^-14.  Quadratic elements get their target by the search of
        exact_data._mse_targets with the formula (o - y) * inv_n and wanted values k 2^-14, k in {-1, 0, 1}; saturated elements y = o -/+ m delta, m in
        {2, 3, 5}, rounded to fp32 and checked to saturate in fp32 (gradient +/- 2 * 2^-14); boundary elements |d| == delta exactly, which needs o - delta to
        be an fp32 value: only where the output is 0 (delta has 24 significant bits).
      L1, n a power of two: sign(d) * inv_n is exact; y == out elements have gradient exactly 0.
    The generator asserts that every class it means to produce is there: in every output channel, and among the windows of the last (ragged) tile -- the
    boundary class, tied to zero outputs, over the whole batch.
  * `damaged_variants`: gradients / losses with one defect each, which `check_loss` must refuse (the pattern of tests/train_ops_reference.py).
"""
import numpy as np
import torch

from tests import exact_data as xd

F32 = np.float32
KINDS = {"mse": 0, "l1": 1, "huber": 2}
G_UNIT = 2.0 ** xd.GOUT_EXP


# ---------------------------------------------------------------------------------------------------
# fp64 references
# ---------------------------------------------------------------------------------------------------
def l1_ref64(out, y):
    """(loss, d loss / d out) of mean |out - y| in fp64; sign(0) = 0."""
    d = out.double().reshape(-1) - y.double().reshape(-1)
    return float(d.abs().mean()), torch.sign(d) / d.numel()


def huber_ref64(out, y, delta):
    """(loss, gradient) of the mean Huber loss in fp64: d^2 / 2 where |d| <= delta, delta (|d| - delta / 2) beyond; gradient clamp(d, -delta, delta) / n."""
    d = out.double().reshape(-1) - y.double().reshape(-1)
    a = d.abs()
    terms = torch.where(a <= delta, 0.5 * d * d, delta * (a - 0.5 * delta))
    return float(terms.mean()), d.clamp(-delta, delta) / d.numel()


def ref64(kind, out, y, delta=1.0):
    if kind == "l1":
        return l1_ref64(out, y)
    if kind == "huber":
        return huber_ref64(out, y, delta)
    d = out.double().reshape(-1) - y.double().reshape(-1)
    return float((d * d).mean()), 2.0 * d / d.numel()


def terms64(kind, out, y, delta=1.0):
    """The per-element loss terms in fp64 (their sum / n is the loss; sum |terms| is the scale of the fp32 summation bound)."""
    d = out.double().reshape(-1) - y.double().reshape(-1)
    a = d.abs()
    if kind == "l1":
        return a
    if kind == "huber":
        return torch.where(a <= delta, 0.5 * d * d, delta * (a - 0.5 * delta))
    return d * d


# ---------------------------------------------------------------------------------------------------
# fp32 host mirror of the kernel expressions
# ---------------------------------------------------------------------------------------------------
def inv_n32(n_total):
    return F32(1.0) / F32(n_total)


def mirror32(kind, out, y, n_total=None, delta=1.0):
    """(g, term) as float32 arrays: the expressions of reg_loss_terms (kinds l1 / huber) and of the MSE sites, each operation rounded to fp32 on its own.
    n_total: the element count of the WHOLE batch (default: this array's)."""
    o, t = np.asarray(out, dtype=F32).reshape(-1), np.asarray(y, dtype=F32).reshape(-1)
    inv = inv_n32(o.size if n_total is None else n_total)
    with np.errstate(invalid="ignore"):
        d = (o - t).astype(F32)
        ad = np.abs(d)
        if kind == "mse":
            return ((F32(2.0) * d).astype(F32) * inv).astype(F32), (d * d).astype(F32)
        if kind == "l1":
            g = np.where(d > 0, inv, np.where(d < 0, -inv, (d * inv).astype(F32))).astype(F32)
            return g, ad
        dl = F32(delta)
        quad = ((F32(0.5) * d).astype(F32) * d).astype(F32)
        lin = (dl * (ad - (F32(0.5) * dl).astype(F32)).astype(F32)).astype(F32)
        term = np.where(ad <= dl, quad, lin).astype(F32)
        c = np.where(d < -dl, -dl, np.where(d > dl, dl, d)).astype(F32)
        return (c * inv).astype(F32), term


# ---------------------------------------------------------------------------------------------------
# exact-case generator
# ---------------------------------------------------------------------------------------------------
def huber_delta(n_total):
    """The fp32 delta next to 2 * 2^-14 * n with fl32(delta * fl32(1 / n)) == 2 * 2^-14 (searched within a few ulps; asserted to exist)."""
    inv = inv_n32(n_total)
    want = F32(2.0 * G_UNIT)
    base = F32(2.0 * G_UNIT * n_total)
    for m in (0, 1, -1, 2, -2, 3, -3):
        d = base
        for _ in range(abs(m)):
            d = np.nextafter(d, F32(np.inf) if m > 0 else F32(-np.inf))
        if F32(d * inv) == want:
            return float(d)
    raise AssertionError(f"no fp32 delta with fl32(delta / {n_total}) == 2^-13 within 3 ulps of {base}")


HUBER_CLASSES = ("zero", "quad+", "quad-", "sat+", "sat-", "boundary")
L1_CLASSES = ("zero", "pos", "neg")


def _search(o32, base, inv, want, ok_extra):
    """exact_data._mse_targets' neighbour search for the formula (o - y) * inv_n: the first fp32 y near `base` whose fp32 gradient is exactly `want`."""
    y, done = o32.copy(), np.zeros(o32.size, dtype=bool)
    for m in (0, 1, -1, 2, -2, 3, -3, 4, -4, 5, -5, 6, -6, 7, -7, 8, -8):
        ym = base.copy()
        for _ in range(abs(m)):
            ym = np.nextafter(ym, F32(np.inf) if m > 0 else F32(-np.inf))
        d = (o32 - ym).astype(F32)
        ok = ~done & ((d * inv).astype(F32).astype(np.float64) == want) & ok_extra(d)
        y[ok] = ym[ok]
        done |= ok
    return y, done


def robust_targets(kind, out, n_per_window, channels, n_total=None, tile=16, mask=None, seed=0):
    """Targets for the flat fp64 output `out` ([windows * n_per_window], channel = index % channels) such that the fp32 loss gradient is a short dyadic number.
    Returns (y fp64 tensor of fp32 values, classes: int array of indices into HUBER_CLASSES / L1_CLASSES, delta).  Asserts the coverage of the module
    docstring.  mask: the flat output mask of one window (elements with mask 0 never carry a class of their own: their gradient is 0 whatever the target)."""
    o = out.reshape(-1).numpy()
    N = o.size
    n_total = N if n_total is None else n_total
    o32 = o.astype(F32)
    assert np.array_equal(o32.astype(np.float64), o), "the output is not an fp32 value"
    inv = inv_n32(n_total)
    w = np.arange(N) // n_per_window
    e = np.arange(N) % n_per_window
    names = HUBER_CLASSES if kind == "huber" else L1_CLASSES
    n_main = len(names) - (1 if kind == "huber" else 0)       # (the boundary class is placed where it can be, below)
    cls = (e + w + seed) % n_main
    y = o32.copy()
    if kind == "l1":
        assert n_total & (n_total - 1) == 0, "L1 is exact only where the element count is a power of two"
        rng = np.random.Generator(np.random.PCG64(seed + 313))
        u = rng.integers(1, 9, size=N).astype(F32) * F32(0.25)
        y = np.where(cls == 1, o32 - u, np.where(cls == 2, o32 + u, o32)).astype(F32)
        delta = 1.0
    else:
        delta = huber_delta(n_total)
        dl = F32(delta)
        for k, c in ((1.0, 1), (-1.0, 2)):
            yq, found = _search(o32, (o - k * G_UNIT * n_total).astype(F32), inv, k * G_UNIT, lambda d: np.abs(d) <= dl)
            sel = (cls == c) & found
            y[sel] = yq[sel]
            cls[(cls == c) & ~found] = 0
        m = np.array([2.0, 3.0, 5.0])[(e + 2 * w) % 3]
        for sgn, c in ((1.0, 3), (-1.0, 4)):
            ys = (o - sgn * m * delta).astype(F32)
            d = (o32 - ys).astype(F32)
            sat = (d > dl) if sgn > 0 else (d < -dl)
            sel = (cls == c) & sat
            y[sel] = ys[sel]
            cls[(cls == c) & ~sat] = 0
        live = np.ones(N, dtype=bool) if mask is None else (np.asarray(mask).reshape(-1)[e] != 0)
        yb = (o32 - dl).astype(F32)
        at = ((o32 - yb).astype(F32) == dl) & (yb.astype(np.float64) == o - float(dl)) & live & (cls == 0)
        pick = np.zeros(N, dtype=bool)
        for k in range(channels):      # per channel every fourth candidate from the second on: zero-gradient elements stay in every channel
            pick[np.nonzero(at & (e % channels == k))[0][1::4]] = True
        at = pick
        y[at] = yb[at]
        cls[at] = 5
    y[cls == 0] = o32[cls == 0]
    # coverage: every class in every output channel and in the last tile
    ch = e % channels
    last = w >= ((w.max() // tile) * tile)
    for c in range(n_main):
        for k in range(channels):
            assert bool(((cls == c) & (ch == k)).any()), f"class {names[c]} is missing in output channel {k}"
        assert bool(((cls == c) & last).any()), f"class {names[c]} is missing among the windows of the last tile"
    if kind == "huber":
        assert bool((cls == 5).any()), "no element sits at |d| == delta exactly (no live zero output)"
    return torch.from_numpy(y.astype(np.float64)), cls, delta


def robust_case(spec, B, seed, kind, tile=16, **knobs):
    """exact_data.exact_case(..., mse=False) with targets for the fused L1 / Huber step: case["y"], case["gout_reg"] (the fp32 mirror's gradient with respect to the model's output, what check_exact
    is handed), case["kind"], case["delta"], case["classes"], case["loss"] (fp64)."""
    case = xd.exact_case(spec, B, seed, mse=False, **knobs)
    out = xd.reference(spec, case)["out"]
    n_per = spec.num_nodes[spec.out_type] * spec.out_channels
    mask = spec.output_mask().reshape(-1).numpy()
    y, cls, delta = robust_targets(kind, out, n_per, spec.out_channels, tile=tile, mask=mask, seed=seed)
    g, _ = mirror32(kind, out.numpy(), y.numpy(), delta=delta)
    gout = torch.from_numpy(g.astype(np.float64))      # d loss / d out of the MASKED output, as gout_mse is: the oracle's backward applies the mask (0, +-1) itself
    case.update(y=y, gout_reg=gout, kind=kind, delta=delta, classes=cls, loss=ref64(kind, out, y, delta)[0])
    return case


def check_robust(spec, case, stats=None):
    """exact_data.check_exact with the robust loss gradient; the reference's `loss` is the fp64 L1 / Huber loss."""
    ref = xd.check_exact(spec, case, gout=case["gout_reg"], stats=stats)
    ref["loss"] = case["loss"]
    # the mirror's gradient is the fp64 gradient exactly (short dyadic numbers): the oracle was handed what torch's loss would hand it
    g64 = ref64(case["kind"], ref["out"], case["y"], case["delta"])[1]
    live = case["gout_reg"] != 0
    err = float((case["gout_reg"][live] - g64[live]).abs().max() / G_UNIT) if bool(live.any()) else 0.0
    assert err < 2.0 ** -10, f"the fp32 gradient is not the fp64 gradient to 2^-10 of its unit: {err}"
    return ref


# ---------------------------------------------------------------------------------------------------
# checkers and the damaged variants they must catch
# ---------------------------------------------------------------------------------------------------
def check_loss(kind, out, y, g, loss, n_total=None, delta=1.0, loss_rtol=2e-7):
    """A gradient `g` (fp32) and a loss for (out, y): the gradient must be the mirror's bits, the loss the fp64 value within loss_rtol.  Returns a list of
    complaints (empty: accepted)."""
    bad = []
    gm, _ = mirror32(kind, out, y, n_total, delta)
    got = np.asarray(g, dtype=F32).reshape(-1)
    if not np.array_equal(got.view(np.uint32), gm.view(np.uint32)):
        i = int(np.nonzero(got.view(np.uint32) != gm.view(np.uint32))[0][0])
        bad.append(f"gradient[{i}] = {got[i]!r}, the mirror has {gm[i]!r}")
    n = gm.size if n_total is None else n_total
    want = float(terms64(kind, torch.from_numpy(np.asarray(out, dtype=np.float64)), torch.from_numpy(np.asarray(y, dtype=np.float64)), delta).sum()) / n
    if not abs(float(loss) - want) <= loss_rtol * abs(want):
        bad.append(f"loss {float(loss)!r}, fp64 has {want!r}")
    return bad


def damaged_variants(kind, out, y, n_total=None, delta=1.0, chunk=None):
    """{name: (g fp32, loss)} with one defect each.  chunk: the element count of a sub-step (for the `inv_n of the chunk` defect)."""
    o, t = np.asarray(out, dtype=F32).reshape(-1), np.asarray(y, dtype=F32).reshape(-1)
    n = o.size if n_total is None else n_total
    inv = inv_n32(n)
    d = (o - t).astype(F32)
    g, term = mirror32(kind, o, t, n, delta)
    loss = float(term.astype(np.float64).sum()) / n
    v = {}
    if kind == "huber":
        dl = F32(delta)
        v["gradient not clamped"] = ((d * inv).astype(F32), loss)
        h = F32(0.5) * dl
        v["clamp at delta / 2"] = ((np.clip(d, -h, h) * inv).astype(F32), loss)
        wrong = np.where(np.abs(d) <= dl, dl * (np.abs(d) - F32(0.5) * dl), F32(0.5) * d * d)
        v["loss term of the wrong branch"] = (g, float(wrong.astype(np.float64).sum()) / n)
    else:
        v["sign(0) = 1"] = (np.where(d >= 0, inv, -inv).astype(F32), loss)
        v["loss term of the wrong branch"] = (g, float((F32(0.5) * d * d).astype(np.float64).sum()) / n)
    v["the factor 2 of MSE left in"] = ((F32(2.0) * g).astype(F32), loss)
    inv_c = inv_n32(chunk if chunk is not None else max(n // 2, 1))
    v["inv_n of the chunk"] = (mirror32(kind, o, t, chunk if chunk is not None else max(n // 2, 1), delta)[0], loss)
    return v
