"""Host-side references, data, checkers and damaged variants for what a training loop runs AROUND the engine's step (csrc/mshgnn_train_ops.hip: k_adam,
k_adam_counted, k_mse, k_ce behind mshgnn_adam_step / _adam_step_counted / _mse_loss / _ce_loss): test infrastructure, no GPU.  The companion of
tests/ops_reference.py, with the same rule: exact data where a bound cannot see one wrong element, a derived bound -- counted rounding by rounding -- on
random data, and deliberately damaged results that every checker of every table case has to reject (tests/test_train_ops_reference.py).

Adam.  Hyperparameters are the fp32 values the C ABI receives (`hp32`); everything else of the reference is fp64, the bias corrections 1 - beta^t included.
Per element, no normalisation by a maximum (u = 2^-24, gamma_k = k u / (1 - k u)):
    m':  |got - ref| <= gamma_5 (|b1 m| + |(1 - b1) g s|)       roundings: g s, b1 m, 1 - b1, (1 - b1)(g s), the sum                               = 5
    v':  |got - ref| <= gamma_8 (|b2 v| + |(1 - b2)(g s)^2|)    roundings: g s (it enters twice), 1 - b2, two products, b2 v, the sum                = 7 <= 8
    p':  |got - (p - U)| <= gamma_8 |U| + u |got|,  U = lr / bc1 * m' / (sqrt(v') / sqrt(bc2) + eps) in fp64 FROM THE DEVICE'S OWN m', v' (errors do not stack)
         roundings of U: bc1 to fp32, lr / bc1, . m', sqrtf, sqrt(bc2) to fp32, the quotient, + eps, the last quotient                                 = 8
         (three sit in the numerator and five in the denominator, all terms of which are positive: (1 + u)^3 / (1 - u)^5 = 1 + 8 u + 33 u^2 + ... is
         below 1 + gamma_8 = 1 + 8 u + 64 u^2 + ...); u |got| is the final subtraction.  sqrtf and the fp32 division are correctly rounded in this build.
An FMA contraction only removes roundings from these paths, so the bounds hold with or without it.  An element whose bound is 0 (m = g = 0; v = g = 0; m' = 0)
must be exactly 0 in m' / v' and must keep p' == p BITWISE.  `adam_emulation` restates the kernel in fp32 torch operations (one rounding each, bias
corrections formed in fp64 and rounded once): the positive control; its errors reach 1.9 u, 3.4 u and 3.5 u of the three bounded quantities.

`adam_exact_case`: t = 1, m = v = 0, beta1 = 1/2, beta2 = 3/4, eps = lr = 2^-10, g = +-(2^k - 2^-10), p a multiple of 1/64 -- every intermediate of the
kernel is an fp32 value (proven on the host, DoesNotClose otherwise), so p', m', v' are compared bit for bit.

Losses.  MSE: gradient within gamma_3 |ref| (out - y, 1 / n, the product; the factor 2 is exact), loss within the any-order bound gamma_(n+3) sum |terms|.
gamma_n cannot see one dropped term at large n, so the large sizes are exact data (integer differences, n a power of two: every partial sum and every
product with 1 / n is an fp32 value -> bit for bit) or SPARSE data (16 non-zero terms of equal size, each 1/16 of the sum, far above gamma_n).
Contact CE ([rows, 2] logits, sum / rows, gradient (softmax - onehot) / rows; any non-zero label counts as 1): the plain arithmetic is counted as above, expf and
logf enter with an ULP figure K (`ce_bounds`); exact rows (equal logits: gradient +-0.5 / rows; gaps of +-1e4: loss term 0 or 1e4, gradient 0 or -+1 / rows)
are compared bit for bit with rows a power of two.

The tables at the end are the cases of tests/test_train_ops_exact_gpu.py; the host tests iterate over the same objects.
"""
import math
from functools import lru_cache

import numpy as np
import torch

from tests.ops_reference import U, DoesNotClose, first_mismatch, gamma, within_bound

SWEEP = 2048 * 256 * 4          # elements of one full sweep of the Adam launch (its block cap x threads x 4)
LOSS_SWEEP = 1024 * 256         # elements / rows of one full sweep of the loss launches


def f32(x):
    """The fp32 value a C float argument receives, as a Python float."""
    return float(np.float32(x))


def hp32(hp):
    return tuple(f32(v) for v in hp)


# ---------------------------------------------------------------------------------------------------
# Adam
# ---------------------------------------------------------------------------------------------------
def bias_corrections(b1, b2, t):
    """(1 - beta1^t, 1 - beta2^t) in fp64 from the fp32-valued betas."""
    return 1.0 - b1 ** t, 1.0 - b2 ** t


def adam_reference(p, g, m, v, t, hp):
    """One Adam step in fp64 from fp32 tensors (torch.optim.Adam: no weight decay, no amsgrad; the gradient is g * grad_scale).  hp: fp32-valued
    (beta1, beta2, eps, grad_scale, lr).  Returns (p', m', v') as fp64 tensors."""
    b1, b2, eps, s, lr = hp
    p, g, m, v = (x.double() for x in (p, g, m, v))
    gs = g * s
    m1 = b1 * m + (1.0 - b1) * gs
    v1 = b2 * v + (1.0 - b2) * gs * gs
    bc1, bc2 = bias_corrections(b1, b2, t)
    return p - lr / bc1 * m1 / (v1.sqrt() / math.sqrt(bc2) + eps), m1, v1


def _factors(b1, b2, t, how):
    """(bc1, sqrt(bc2)) as the fp32 values the kernel divides by: 'fp64' formed in double and rounded once; 'fp32': 1 - powf(beta, t) and sqrtf of it, all in
    fp32 (the defect); 'none': 1, 1."""
    if how == "fp64":
        bc1, bc2 = bias_corrections(b1, b2, t)
        return f32(bc1), f32(math.sqrt(bc2))
    if how == "fp32":
        one = np.float32(1.0)
        with np.errstate(under="ignore"):
            c1, c2 = one - np.power(np.float32(b1), np.float32(t)), one - np.power(np.float32(b2), np.float32(t))
        return float(c1), float(np.sqrt(c2))
    return 1.0, 1.0


def adam_emulation(p, g, m, v, t, hp, bc="fp64", eps_inside=False, use_scale=True):
    """k_adam in fp32 torch operations, one rounding per operation (no contraction).  Returns fp32 (p', m', v')."""
    b1, b2, eps, s, lr = hp
    assert p.dtype == g.dtype == m.dtype == v.dtype == torch.float32
    gs = g * s if use_scale else g.clone()
    om1, om2 = float(np.float32(1.0) - np.float32(b1)), float(np.float32(1.0) - np.float32(b2))
    m1 = m * b1 + gs * om1
    v1 = v * b2 + (gs * om2) * gs
    bc1, bc2s = _factors(b1, b2, t, bc)
    step = float(np.float32(lr) / np.float32(bc1))
    if eps_inside:
        den = (v1 / float(np.float32(bc2s) * np.float32(bc2s)) + eps).sqrt()
    else:
        den = v1.sqrt() / bc2s + eps
    return p - (m1 * step) / den, m1, v1


def adam_bounds(case):
    """(bound of m', bound of v') per element, fp64."""
    b1, b2, eps, s, lr = case["hp"]
    g, m, v = (case[k].double() for k in ("g", "m", "v"))
    gs = g * s
    return gamma(5) * ((b1 * m).abs() + ((1.0 - b1) * gs).abs()), gamma(8) * ((b2 * v).abs() + (1.0 - b2) * gs * gs)


def _bits(x):
    return x.detach().cpu().contiguous().view(torch.int32)


def adam_check(case, p_got, m_got, v_got):
    """None when (p', m', v') (fp32) pass the case's checker, else a description of the first offenders.  Exact cases: bit for bit against the proven
    values.  Random data: the three bounds of the module docstring, the parameter's from the returned m', v'."""
    p_got, m_got, v_got = (x.detach().cpu().reshape(-1) for x in (p_got, m_got, v_got))
    if case["exact"]:
        for name, got, ref in (("m'", m_got, case["ref_m"]), ("v'", v_got, case["ref_v"]), ("p'", p_got, case["ref_p"])):
            d = first_mismatch(got, ref)
            if d:
                return f"{name}: {d}"
        return None
    b1, b2, eps, s, lr = case["hp"]
    ref_p, ref_m, ref_v = adam_reference(case["p"], case["g"], case["m"], case["v"], case["t"], case["hp"])
    bm, bv = adam_bounds(case)
    d = within_bound(m_got, ref_m, bm)
    if d:
        return f"m': {d}"
    d = within_bound(v_got, ref_v, bv)
    if d:
        return f"v': {d}"
    bc1, bc2 = bias_corrections(b1, b2, case["t"])
    m1, v1 = m_got.double(), v_got.double()
    upd = lr / bc1 * m1 / (v1.sqrt() / math.sqrt(bc2) + eps)
    still = upd == 0
    bound = torch.where(still, torch.zeros_like(upd), gamma(8) * upd.abs() + U * p_got.double().abs())
    d = within_bound(p_got, case["p"].double() - upd, bound)
    if d:
        return f"p': {d}"
    moved = still & (_bits(p_got) != _bits(case["p"]))
    if bool(moved.any()):
        i = int(moved.nonzero()[0])
        return f"p'[{i}]: an element without update changed its bits ({float(case['p'][i])!r} -> {float(p_got[i])!r})"
    return None


def adam_error_units(case, p_got, m_got, v_got):
    """The worst errors in u of the bounded quantity ((|b1 m| + |(1 - b1) g s|), the same for v, |U|; the p' figure after taking u |p'| off): what the
    bounds 5, 8 and 8 are compared with.  For reports only."""
    b1, b2, eps, s, lr = case["hp"]
    ref_p, ref_m, ref_v = adam_reference(case["p"], case["g"], case["m"], case["v"], case["t"], case["hp"])
    bm, bv = adam_bounds(case)
    p_got, m_got, v_got = (x.detach().cpu().reshape(-1).double() for x in (p_got, m_got, v_got))
    bc1, bc2 = bias_corrections(b1, b2, case["t"])
    upd = lr / bc1 * m_got / (v_got.sqrt() / math.sqrt(bc2) + eps)

    def worst(err, scale):
        ok = scale > 0
        return float((err[ok] / scale[ok]).max() / U) if bool(ok.any()) else 0.0
    ep = ((p_got - (case["p"].double() - upd)).abs() - U * p_got.abs()).clamp(min=0)
    return worst((m_got - ref_m).abs(), bm / gamma(5)), worst((v_got - ref_v).abs(), bv / gamma(8)), worst(ep, upd.abs())


ADAM_HP = [(0.9, 0.999, 1e-8, 1.0, 1e-3), (0.5, 0.9, 1e-3, 1.0 / 3.0, 1e-2), (0.0, 0.99, 1e-8, 1.0 / 8.0, 1e-3)]      # (beta1, beta2, eps, grad_scale, lr)


@lru_cache(maxsize=2)
def _adam_data(n, hp_i):
    """|g s|, |m| and sqrt(v) are exactly 0 or log-uniform in [1e-12, 1e3] (no term underflows).  Every element 1 (mod 4) has g = m = v = 0 (the normal
    case of this project: most parameter tensors of a model have exact-zero gradients), 3 (mod 8) has g = 0 alone, 7 (mod 8) has m = v = 0 alone.  The
    PROBES -- elements 0, 2, n - 2, n - 1 -- have all three magnitudes within [0.5, 2] x 1000 eps and p = 0: there eps is 1e-3 of the denominator (a wrong
    bias correction shows undiluted, a misplaced eps too) and the update is not hidden behind the rounding of a large p.  A third of the other parameters are
    0, a third of size 1e-4, a third of size 1."""
    b1, b2, eps, s, lr = hp32(ADAM_HP[hp_i])
    gen = torch.Generator().manual_seed(7919 * n + hp_i)

    def mag():
        return (10.0 ** (torch.rand(n, generator=gen, dtype=torch.float64) * 14.9 - 11.95))

    def sign():
        return torch.randint(0, 2, (n,), generator=gen).double() * 2 - 1
    gs, mm, sv = mag() * sign(), mag() * sign(), mag()
    p = torch.randn(n, generator=gen, dtype=torch.float64)
    i = torch.arange(n)
    p[i % 3 == 0] = 0.0
    p[i % 3 == 1] *= 1e-4
    probes = sorted({k for k in (0, 2, n - 2, n - 1) if 0 <= k < n})
    zero = (i % 4 == 1) & (i < n - 2)
    g0 = (i % 8 == 3)
    s0 = (i % 8 == 7)
    for k in probes:
        zero[k] = g0[k] = s0[k] = False
    gs[zero | g0] = 0.0
    mm[zero | s0] = 0.0
    sv[zero | s0] = 0.0
    r = torch.rand(3, len(probes), generator=gen, dtype=torch.float64) * 1.5 + 0.5
    sg = torch.randint(0, 2, (2, len(probes)), generator=gen).double() * 2 - 1
    for j, k in enumerate(probes):
        gs[k], mm[k], sv[k], p[k] = 1000 * eps * r[0, j] * sg[0, j], 1000 * eps * r[1, j] * sg[1, j], 1000 * eps * r[2, j], 0.0
    if n >= 4:
        p[1] = 0.0          # a zero-gradient element at p = 0: any noise added to it shows
    return dict(p=p.float(), g=(gs / s).float(), m=mm.float(), v=(sv * sv).float(), zero=zero, probes=probes)


def adam_case(n, t, hp_i):
    d = _adam_data(n, hp_i)
    return dict(d, n=n, t=t, hp=hp32(ADAM_HP[hp_i]), hp_i=hp_i, exact=False)


EXACT_HP = (0.5, 0.75, 2.0 ** -10, 1.0, 2.0 ** -10)


def _is_f32(x):
    return torch.equal(x.float().double(), x)


@lru_cache(maxsize=2)
def adam_exact_case(n):
    """The exact case of the module docstring; every seventh element has g = 0 (then m' = v' = 0 and p' == p).  Proof: each intermediate of the kernel,
    evaluated in fp64, is its own fp32 rounding -- so the fp32 kernel, fused or not, computes the fp64 values."""
    b1, b2, eps, s, lr = EXACT_HP
    gen = torch.Generator().manual_seed(n)
    i = torch.arange(n)
    k = (i % 6 - 3).double()
    g = (2.0 ** k - 2.0 ** -10) * (((i // 6) % 2).double() * 2 - 1)
    g[i % 7 == 3] = 0.0
    p = torch.randint(-64, 65, (n,), generator=gen).double() / 64
    m = v = torch.zeros(n, dtype=torch.float64)
    steps = {}
    steps["g s"] = gs = g * s
    steps["b1 m"], steps["1 - b1"], steps["1 - b2"] = b1 * m, torch.tensor(1.0 - b1), torch.tensor(1.0 - b2)
    steps["(1 - b1) g s"] = (1.0 - b1) * gs
    steps["m'"] = m1 = b1 * m + (1.0 - b1) * gs
    steps["(1 - b2) g s"] = (1.0 - b2) * gs
    steps["(1 - b2) (g s)^2"] = (1.0 - b2) * gs * gs
    steps["v'"] = v1 = b2 * v + (1.0 - b2) * gs * gs
    bc1, bc2 = bias_corrections(b1, b2, 1)
    steps["bc1"], steps["sqrt bc2"], steps["lr / bc1"] = torch.tensor(bc1), torch.tensor(math.sqrt(bc2)), torch.tensor(lr / bc1)
    steps["lr / bc1 m'"] = num = lr / bc1 * m1
    steps["sqrt v'"] = sq = v1.sqrt()
    steps["sqrt v' / sqrt bc2"] = q = sq / math.sqrt(bc2)
    steps["+ eps"] = den = q + eps
    steps["update"] = upd = num / den
    steps["p'"] = p1 = p - upd
    for name, x in steps.items():
        if not _is_f32(x):
            raise DoesNotClose(f"exact Adam case, n = {n}: {name} is not an fp32 value")
    if not torch.equal(sq * sq, v1) or not torch.equal(upd * den, num):
        raise DoesNotClose(f"exact Adam case, n = {n}: the square root or the last quotient rounds")
    live = g != 0
    want = -torch.sign(g) * 2.0 ** -10 * (1.0 - 2.0 ** (-10 - k))
    assert torch.equal(den[live], 2.0 ** k[live]) and torch.equal((p1 - p)[live], want[live]) and torch.equal(p1[~live], p[~live])
    return dict(n=n, t=1, hp=EXACT_HP, hp_i=None, exact=True, p=p.float(), g=g.float(), m=m.float(), v=v.float(), ref_p=p1, ref_m=m1, ref_v=v1,
                zero=~live, probes=[])


ADAM_DAMAGES = ("bc_fp32", "bc_dropped", "eps_inside_sqrt", "grad_scale_ignored", "tail_untouched", "second_sweep_untouched", "neighbour_gradient",
                "zero_element_moved")
BC_VISIBLE = 17.0          # in u: see damaged_adam


def bc_deviation(hp, t, how):
    """The larger relative deviation, in u, of 1 / bc1 and 1 / sqrt(bc2) formed as `how` from the correctly formed fp32 factors."""
    a, b = _factors(hp[0], hp[1], t, "fp64"), _factors(hp[0], hp[1], t, how)
    return max(abs(a[0] / b[0] - 1.0), abs(a[1] / b[1] - 1.0)) / U


def damaged_adam(case, kind):
    """A deliberately wrong (p', m', v') (fp32) built from the positive-control emulation, or None where the damage does not exist for this case:
      bc_fp32 / bc_dropped: the bias corrections formed in fp32 (1 - powf(beta, t)) / left out.  A factor within a few u of the right one is no wrong
          result -- the bound grants the factors a rounding each -- so these two exist where 1 / bc1 or 1 / sqrt(bc2) is off by more than BC_VISIBLE = 17 u:
          at the probes (eps = 1e-3 of the denominator) the update is then off by more than 16 u, beyond the 8 u the checker allows plus the 8 u it
          allows the rest of the path.  (t = 1: 1 - beta is exact in fp32; t = 1e5: both are 1.)
      eps_inside_sqrt: sqrt(v / bc2 + eps);  grad_scale_ignored (scale 1: none);  tail_untouched: the last n % 4 elements keep p, m, v;
      second_sweep_untouched: the elements from SWEEP on;  neighbour_gradient: the last element is updated with g[n - 2];
      zero_element_moved: the first element with g = m = v = 0 has eps added to p."""
    args = (case["p"], case["g"], case["m"], case["v"], case["t"], case["hp"])
    n = case["n"]
    good = adam_emulation(*args)
    if kind in ("bc_fp32", "bc_dropped"):
        how = "fp32" if kind == "bc_fp32" else "none"
        if bc_deviation(case["hp"], case["t"], how) <= (0.0 if case["exact"] else BC_VISIBLE):
            return None
        bad = adam_emulation(*args, bc=how)
    elif kind == "eps_inside_sqrt":
        bad = adam_emulation(*args, eps_inside=True)
    elif kind == "grad_scale_ignored":
        if case["hp"][3] == 1.0:
            return None
        bad = adam_emulation(*args, use_scale=False)
    elif kind in ("tail_untouched", "second_sweep_untouched"):
        lo = n - n % 4 if kind == "tail_untouched" else SWEEP
        if lo >= n:
            return None
        bad = tuple(x.clone() for x in good)
        for b, src in zip(bad, (case["p"], case["m"], case["v"])):
            b[lo:] = src[lo:]
    elif kind == "neighbour_gradient":
        if n < 2:
            return None
        one = adam_emulation(case["p"][n - 1:], case["g"][n - 2:n - 1], case["m"][n - 1:], case["v"][n - 1:], case["t"], case["hp"])
        bad = tuple(x.clone() for x in good)
        for b, o in zip(bad, one):
            b[n - 1] = o[0]
    elif kind == "zero_element_moved":
        z = case["zero"].nonzero()
        if z.numel() == 0:
            return None
        z = int(z[0])
        bad = tuple(x.clone() for x in good)
        bad[0][z] = float(np.float32(float(case["p"][z]) + case["hp"][2]))
    else:
        raise KeyError(kind)
    if all(torch.equal(_bits(a), _bits(b)) for a, b in zip(bad, good)):
        return None
    return bad


# ---------------------------------------------------------------------------------------------------
# MSE
# ---------------------------------------------------------------------------------------------------
def mse_reference(out, y):
    """(mean((out - y)^2), 2 (out - y) / n) in fp64 from fp32 tensors."""
    d = out.double() - y.double()
    return float((d * d).sum() / d.numel()), 2.0 * d / d.numel()


def loss_blocks(n):
    return min((n + 255) // 256, 1024)


SPARSE_TERMS = 16


def _sparse_positions(n, gen):
    """SPARSE_TERMS positions of a large case: the first, the last, both sides of the end of the first sweep, the rest at random."""
    fixed = [k for k in (0, n - 1, LOSS_SWEEP - 1, LOSS_SWEEP) if 0 <= k < n]
    more = torch.randperm(n, generator=gen)[:SPARSE_TERMS * 2].tolist()
    pos = list(dict.fromkeys(fixed + more))[:SPARSE_TERMS]
    assert len(pos) == SPARSE_TERMS
    return torch.tensor(pos)


@lru_cache(maxsize=4)
def mse_case(n, kind):
    """kind 'random': randn operands.  'exact': integer y in [-1, 1] and integer out - y in [-2, 2], n a power of two: sum (out - y)^2 <= 4 n < 2^24 and 1 / n
    a power of two, so every partial sum in any order, every product with 1 / n and the gradient are fp32 values (proven here).  'sparse': out == y (random
    integers) except SPARSE_TERMS differences of +-1."""
    gen = torch.Generator().manual_seed(104729 * n + len(kind))
    if kind == "random":
        out, y = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    else:
        y = torch.randint(-1, 2, (n,), generator=gen).float()
        if kind == "exact":
            d = torch.randint(-2, 3, (n,), generator=gen).float()
        else:
            d = torch.zeros(n)
            pos = _sparse_positions(n, gen)
            d[pos] = (torch.randint(0, 2, (SPARSE_TERMS,), generator=gen) * 2 - 1).float()
        out = y + d
    loss, grad = mse_reference(out, y)
    case = dict(n=n, kind=kind, out=out, y=y, loss=loss, grad=grad, exact=kind == "exact", sum_abs=loss)
    if kind == "exact":
        if n & (n - 1) or not 4 * n < 2 ** 24:
            raise DoesNotClose(f"exact MSE case: n = {n} is not a power of two below 2^22")
        if not _is_f32(grad) or f32(loss) != loss:
            raise DoesNotClose(f"exact MSE case, n = {n}: the loss or the gradient is not an fp32 value")
    return case


def mse_check(case, loss_got, grad_got):
    """None when the loss (a float) and the gradient (fp32 tensor, or None for a call without one) pass, else what failed."""
    loss_got = float(loss_got)
    if case["exact"]:
        if not loss_got == case["loss"]:
            return f"loss: got {loss_got!r}, want {case['loss']!r} bit for bit"
        d = first_mismatch(grad_got, case["grad"]) if grad_got is not None else None
        return f"gradient: {d}" if d else None
    bound = float(gamma(case["n"] + 3)) * case["sum_abs"]
    if not abs(loss_got - case["loss"]) <= bound:
        return f"loss: got {loss_got!r}, want {case['loss']!r}, bound {bound:.3e}"
    if grad_got is not None:
        d = within_bound(grad_got, case["grad"], gamma(3) * case["grad"].abs())
        if d:
            return f"gradient: {d}"
    return None


def order_bound(case):
    """Two runs of one loss differ in the order of the atomic adds of the workgroups' partial sums alone: each order is within gamma_(blocks - 1) of the
    exact sum of the same partials, so the two results differ by at most 2 gamma_(blocks - 1) sum |partials| (one workgroup: identical)."""
    b = loss_blocks(case["n"])
    return 0.0 if b == 1 or case["exact"] else 2.0 * float(gamma(b - 1)) * case["sum_abs"] * (1 + float(gamma(case["n"] + 3)))


LOSS_DAMAGES = ("drop_one_term", "one_over_n_minus_1", "swap_gradient_pair", "label_equals_1", "no_max_subtraction")


def _median_nonzero(terms):
    nz = terms.abs().nonzero()[:, 0]
    return None if nz.numel() == 0 else int(nz[terms[nz].abs().argsort()[nz.numel() // 2]])


def _swap_last_differing_pair(grad):
    g2 = grad.reshape(-1, 2)
    rows = (g2[:, 0] != g2[:, 1]).nonzero()
    if rows.numel() == 0:
        return None
    bad = g2.clone()
    r = int(rows[-1])
    bad[r] = g2[r].flip(0)
    return bad.reshape(grad.shape)


def damaged_mse(case, kind):
    """(loss, gradient) deliberately wrong, or None where the damage does not exist: drop_one_term: the sum misses the non-zero term of median size;
    one_over_n_minus_1: loss and gradient scaled by 1 / (n - 1) (n = 1: infinite);  swap_gradient_pair: the last pair of gradient elements (2 k, 2 k + 1)
    that differ is exchanged."""
    n, loss, grad = case["n"], case["loss"], case["grad"]
    if kind == "drop_one_term":
        d = case["out"].double() - case["y"].double()
        k = _median_nonzero(d)
        return None if k is None else (loss - float(d[k] * d[k]) / n, grad)
    if kind == "one_over_n_minus_1":
        f = n / (n - 1) if n > 1 else float("inf")
        return loss * f, grad * f
    if kind == "swap_gradient_pair":
        bad = _swap_last_differing_pair(grad[:n - n % 2]) if n >= 2 else None
        return None if bad is None else (loss, torch.cat([bad, grad[n - n % 2:]]))
    return None


# ---------------------------------------------------------------------------------------------------
# contact cross entropy
# ---------------------------------------------------------------------------------------------------
def ce_reference(logits, labels):
    """fp64: (per-row terms logsumexp - logit[label], their sum / rows, gradient (softmax - onehot) / rows); any non-zero label is class 1."""
    l = logits.double()
    lab = (labels != 0).long()
    lse = torch.logsumexp(l, 1)
    terms = lse - l.gather(1, lab[:, None])[:, 0]
    rows = l.shape[0]
    grad = (torch.softmax(l, 1) - torch.nn.functional.one_hot(lab, 2).double()) / rows
    return terms, float(terms.sum() / rows), grad


GAP = 1.0e4
UNDERFLOW_GAP = 200.0


@lru_cache(maxsize=4)
def ce_case(rows, kind):
    """kind 'random': logits 3 randn (gaps up to ~25: nothing underflows), labels from {0, 1, -1, 7}.
    'gap' / 'exact_gap': every row is (0, +-1e4) or (+-1e4, 0); the row's term is exactly 0 when the label names the larger logit, 1e4 otherwise
        (SPARSE_TERMS such rows); gradient 0 or -+1 / rows.  'exact_gap' (rows a power of two <= 2^19): 16 x 1e4 / rows and -+1 / rows are fp32 values and so
        is every partial sum: loss and gradient bit for bit.
    'exact_equal' (rows a power of two): gap rows with the right label except SPARSE_TERMS rows of two EQUAL logits: term ln 2 (the loss is held to the
        bound), gradient exactly -+0.5 / rows (the gradient is held bit for bit)."""
    gen = torch.Generator().manual_seed(15485863 * rows + len(kind))
    nonzero = torch.tensor([1, -1, 7, 1], dtype=torch.int32)
    if kind == "random":
        logits = 3.0 * torch.randn(rows, 2, generator=gen)
        labels = torch.where(torch.rand(rows, generator=gen) < 0.5, torch.zeros(rows, dtype=torch.int32), nonzero[torch.randint(0, 4, (rows,), generator=gen)])
    else:
        big = torch.randint(0, 2, (rows,), generator=gen)                       # which logit is the larger one
        sgn = (torch.randint(0, 2, (rows,), generator=gen) * 2 - 1).float()      # (0, 1e4) or (-1e4, 0)
        logits = torch.zeros(rows, 2)
        r = torch.arange(rows)
        logits[r, big] = torch.where(sgn > 0, torch.tensor(GAP), torch.tensor(0.0))
        logits[r, 1 - big] = torch.where(sgn > 0, torch.tensor(0.0), torch.tensor(-GAP))
        right = torch.where(big == 1, nonzero[torch.randint(0, 4, (rows,), generator=gen)], torch.zeros(rows, dtype=torch.int32))
        labels = right.clone()
        special = _sparse_positions(rows, gen) if rows >= 2 * SPARSE_TERMS else torch.arange(0, rows, 2)
        if kind == "exact_equal":
            logits[special] = (torch.randint(-3, 4, (special.numel(), 1), generator=gen).float() * 0.5).expand(-1, 2)
        else:
            labels[special] = torch.where(big[special] == 1, torch.zeros(special.numel(), dtype=torch.int32), nonzero[:1].expand(special.numel()))
    terms, loss, grad = ce_reference(logits, labels)
    case = dict(rows=rows, n=rows, kind=kind, logits=logits, labels=labels, terms=terms, loss=loss, grad=grad, exact_grad=kind.startswith("exact"),
                exact=kind == "exact_gap", sum_abs=float(terms.sum() / rows))
    if case["exact_grad"]:
        if rows & (rows - 1) or not _is_f32(grad):
            raise DoesNotClose(f"exact CE case, rows = {rows}: the gradient is not made of fp32 values")
    if kind == "exact_gap":
        if not float(terms.sum()) < 2 ** 24 or f32(loss) != loss or not bool(((terms == 0) | (terms == GAP)).all()):
            raise DoesNotClose(f"exact CE case, rows = {rows}: the loss is not an fp32 value")
    return case


def ce_bounds(case, K):
    """(bound of the loss, bound of the gradient [rows, 2]) in fp64.  K: the error of expf and of logf in ulp.  With d = min - max logit (rounded: relative
    error |d| u of its exponential), e = exp(d), z = 1 + e, p_min = e / z:
        z          relative error (K + 1 + |d| p_min) u                              (expf of the maximum's 0 and of d, the addition)
        row term   (K + 1 + |d| p_min) u + K u |log z| + gamma_2 (|log z| + |max| + |logit[label]|)       (logf, then + max and - logit[label])
        loss       (sum of the rows' bounds + gamma_(rows + 2) sum (terms + bounds)) / rows      (rows - 1 additions in any order, 1 / rows, the product)
        softmax_j  relative error (2 K + 2 + |d_j| + |d| p_min) u;   gradient entry: that times softmax_j, + gamma_3 |softmax_j - onehot_j|, all / rows
    First-order terms with a factor 1 + 2^-10 for the products of errors left out.  A row whose gap exceeds UNDERFLOW_GAP = 200 (exp(-200) is far below the
    smallest fp32 subnormal) has e = 0, z = 1 and logf(1) = 0 exactly, so its term is fl(max - logit[label]): bound u |max - logit[label]|, 0 when the label
    names the maximum -- such rows add no error budget, which is what lets a few live rows among 2^18 silent ones be policed."""
    l = case["logits"].double()
    rows = l.shape[0]
    lab = (case["labels"] != 0).long()
    mx = l.max(1).values
    d = (l - mx[:, None])                      # 0 for the maximum, the negative gap for the other
    gap = d.min(1).values.abs()
    e = torch.exp(-gap)
    z = 1.0 + e
    w = gap * e / z
    logz = torch.log(z)
    picked = l.gather(1, lab[:, None])[:, 0]
    slack = 1.0 + 2.0 ** -10
    row = ((K + 1 + w) * U + K * U * logz + gamma(2) * (logz + mx.abs() + picked.abs())) * slack
    row = torch.where(gap > UNDERFLOW_GAP, U * (mx - picked).abs(), row)
    loss_bound = float((row.sum() + gamma(rows + 2) * (case["terms"].abs() + row).sum()) / rows)
    soft = torch.softmax(l, 1)
    onehot = torch.nn.functional.one_hot(lab, 2).double()
    rel = (2 * K + 2 + d.abs() + w[:, None]) * U
    grad_bound = (rel * soft + gamma(3) * (soft - onehot).abs()) / rows * slack
    return loss_bound, grad_bound


def ce_check(case, loss_got, grad_got, K):
    loss_got = float(loss_got)
    loss_bound, grad_bound = ce_bounds(case, K)
    if case["exact"]:
        if not loss_got == case["loss"]:
            return f"loss: got {loss_got!r}, want {case['loss']!r} bit for bit"
    elif not abs(loss_got - case["loss"]) <= loss_bound:
        return f"loss: got {loss_got!r}, want {case['loss']!r}, bound {loss_bound:.3e}"
    if grad_got is not None:
        d = first_mismatch(grad_got, case["grad"]) if case["exact_grad"] else within_bound(grad_got, case["grad"], grad_bound)
        if d:
            return f"gradient: {d}"
    return None


def ce_needed_ulp(case, loss_got, grad_got):
    """The smallest K >= 0 with which (loss, gradient) pass ce_bounds: the bounds are affine in K.  For the one-off measurement on the device."""
    (l0, g0), (l1, g1) = ce_bounds(case, 0.0), ce_bounds(case, 1.0)
    err = (grad_got.detach().double().cpu().reshape(g0.shape) - case["grad"]).abs()
    over = torch.cat([(err - g0).reshape(-1), torch.tensor([abs(float(loss_got) - case["loss"]) - l0], dtype=torch.float64)])
    per_k = torch.cat([(g1 - g0).reshape(-1), torch.tensor([l1 - l0], dtype=torch.float64)])
    need = torch.where(over <= 0, torch.zeros_like(over), over / per_k)      # (an excess where K buys nothing: infinite)
    return float(need.max())


def ce_emulation(logits, labels, max_subtraction=True, equals_1=False):
    """k_ce in fp32 torch operations (terms summed in fp64 and rounded once: any order is allowed).  Returns (loss, gradient fp32)."""
    l = logits.float()
    rows = l.shape[0]
    lab = (labels == 1).long() if equals_1 else (labels != 0).long()
    mx = l.max(1).values if max_subtraction else torch.zeros(rows)
    e = torch.exp(l - mx[:, None])
    z = e[:, 0] + e[:, 1]
    terms = torch.log(z) + mx - l.gather(1, lab[:, None])[:, 0]
    inv = float(np.float32(1.0) / np.float32(rows))
    grad = (e / z[:, None] - torch.nn.functional.one_hot(lab, 2).float()) * inv
    return float(np.float32(float(terms.double().sum())) * np.float32(inv)), grad


def damaged_ce(case, kind):
    """(loss, gradient) deliberately wrong or None: the three of damaged_mse (swap: the two entries of the last row whose entries differ), and
    label_equals_1: labels -1 and 7 read as class 0;  no_max_subtraction: expf of the raw logits (exists where a logit overflows it: > 88)."""
    rows, loss, grad = case["rows"], case["loss"], case["grad"]
    if kind == "drop_one_term":
        k = _median_nonzero(case["terms"])
        return None if k is None else (loss - float(case["terms"][k]) / rows, grad)
    if kind == "one_over_n_minus_1":
        f = rows / (rows - 1) if rows > 1 else float("inf")
        return loss * f, grad * f
    if kind == "swap_gradient_pair":
        bad = _swap_last_differing_pair(grad)
        return None if bad is None else (loss, bad)
    if kind == "label_equals_1":
        if not bool(((case["labels"] != 0) & (case["labels"] != 1)).any()):
            return None
        return ce_emulation(case["logits"], case["labels"], equals_1=True)
    if kind == "no_max_subtraction":
        if not float(case["logits"].max()) > 88.0:
            return None
        return ce_emulation(case["logits"], case["labels"], max_subtraction=False)
    raise KeyError(kind)


# ---------------------------------------------------------------------------------------------------
# the GPU tables (tests/test_train_ops_exact_gpu.py runs them, tests/test_train_ops_reference.py polices them)
# ---------------------------------------------------------------------------------------------------
S = SWEEP
ADAM_N = [1, 3, 4, 5, 7, 1023, 1024, 1025, S, S + 1, S + 4, S + 1027, 2 * S + 5]
ADAM_T = [1, 2, 3, 10, 1000, 100000]
ADAM_T_AT = [5, 7, 1025]                  # the full list of step counts, under every hyperparameter set, runs at these n
ADAM_EXACT_N = [5, 1027, S + 1027]


def all_adam_cases():
    """('random', n, t, hyperparameter index) | ('exact', n): every n at t = 2 under the default hyperparameters (where fp32 bias corrections are worst),
    every t x every hyperparameter set at a few small n, the other hyperparameter sets in the second and third sweep, the exact case in tail and sweeps."""
    out = [("random", n, 2, 0) for n in ADAM_N]
    out += [("random", n, t, h) for n in ADAM_T_AT for h in range(len(ADAM_HP)) for t in ADAM_T]
    out += [("random", S + 4, 3, 1), ("random", 2 * S + 5, 10, 2)]
    out += [("exact", n) for n in ADAM_EXACT_N]
    return list(dict.fromkeys(out))


def build_adam_case(key):
    return adam_exact_case(key[1]) if key[0] == "exact" else adam_case(*key[1:])


LOSS_N = [1, 63, 64, 65, 255, 256, 257]
LOSS_BIG = LOSS_SWEEP + 1                 # 262145: one element / row in the second sweep
MSE_CASES = [(n, "random") for n in LOSS_N] + [(LOSS_BIG, "sparse"), (2 ** 18, "exact"), (2 ** 19, "exact")]
CE_CASES = [(n, "random") for n in LOSS_N] + [(LOSS_BIG, "gap"), (1, "exact_gap"), (1024, "exact_gap"), (2 ** 19, "exact_gap"), (2, "exact_equal"),
                                             (2 ** 18, "exact_equal")]
