"""Host-side references, data, checkers and damaged variants for the flat optimizers and gradient clipping (csrc/mshgnn_train_ops.hip: k_sgd, k_adamw,
k_grad_norm, k_grad_clip behind mshgnn_sgd_step / _adamw_step / _grad_norm / _grad_clip): test infrastructure, no GPU.  Built on tests/ops_reference.py and
tests/train_ops_reference.py, with their rule: exact data where every intermediate is an fp32 value (proven here, DoesNotClose otherwise), bounds counted
rounding by rounding on random data, an fp32 emulation of every kernel path as the positive control, and deliberately damaged results that every checker of
every table case has to reject (tests/test_optim_reference.py, which also pins the fp64 references to torch's own optimizers).

Hyperparameters are the fp32 values the C ABI receives (`hp32`); everything else of the references is fp64.  u = 2^-24, gamma_k = k u / (1 - k u); per
element, no normalisation by a maximum.  An FMA contraction only removes roundings, so the bounds hold with or without it.

SGD (hp = lr, momentum, dampening, weight_decay, nesterov, grad_scale).  With D = |g s| + |wd p| and kd the roundings of d = g s + wd p:
    d:     g s                                              = 1 (kd = 1 without weight decay);   g s, wd p, the sum                          = 3 (kd = 3 with it)
    buf':  first step  buf' = d                             = kd:      |got - ref| <= gamma_kd D
           later       mom buf, 1 - damp, (1 - damp) d, the sum, and d's own = kd + 4:      |got - ref| <= gamma_(kd+4) (|mom buf| + |1 - damp| D)
    p':    plain       lr d, and d's own                    = kd + 1:  |got - (p - lr d)| <= gamma_(kd+1) lr D + u |got|
           momentum    lr buf' FROM THE DEVICE'S OWN buf' (errors do not stack)  = 1:  |got - (p - lr buf')| <= gamma_1 lr |buf'| + u |got|
           nesterov    d (kd), mom buf', the sum, lr .      = kd + 3:  |got - (p - lr (d + mom buf'))| <= gamma_(kd+3) lr (D + |mom buf'|) + u |got|
    u |got| is the final subtraction.  An element whose bound is 0 must be exactly 0 in buf' and keep p' == p BITWISE.

Adam with weight decay (hp = beta1, beta2, eps, grad_scale, lr, weight_decay, decoupled).  Coupled: g' = g s + wd p has kd = 3 roundings and D as above;
otherwise kd = 1, D = |g s|:
    m':  g' (kd), b1 m, 1 - b1, (1 - b1) g', the sum = kd + 4:                               |got - ref| <= gamma_(kd+4) (|b1 m| + (1 - b1) D)
    v':  g' (it enters twice: 2 kd), 1 - b2, two products, b2 v, the sum = 2 kd + 5:          |got - ref| <= gamma_(2kd+5) (|b2 v| + (1 - b2) D^2)
    p':  decoupled: p0 = p (1 - lr wd): lr wd, the difference, the product = 3:              |p0 error| <= gamma_3 |p| (1 + lr wd)
         then U from the device's own m', v' as for Adam (8 roundings, tests/train_ops_reference.py):
                                                                    |got - (p0 - U)| <= gamma_8 |U| + gamma_3 |p| (1 + lr wd) [decoupled] + u |got|
    An element with U = 0 (and p = 0 when the decay is decoupled) keeps its bits.

Norm: sqrt(sum g_i^2) in fp64; the reference is math.fsum of the exact squares.  Any summation order of n non-negative fp64 terms is within (n - 1) 2^-53 of
the sum, the square root halves a relative error and adds 2^-53: n 2^-53 relative in all (n >= 2; n = 1 is exact up to the correctly rounded root).  Exact
data (small integers: every partial sum is an integer below 2^53) is compared bit for bit with math.sqrt of the exact sum.  `norm_emulation` restates
k_grad_norm's order: lanes over their grid-stride quads, the xor butterfly of a wave, the waves in order, the workgroups' partials in index order.

Clip: c = min(1, max_norm / (norm + 1e-6)) in fp64, rounded to fp32 (1), the product (1): |got - g c| <= gamma_2 |g c|; c == 1: every bit as it was.

The tables at the end are the cases of tests/test_optim_exact_gpu.py; the host tests iterate over the same objects.
"""
import math
from functools import lru_cache

import numpy as np
import torch

from tests.ops_reference import U, DoesNotClose, first_mismatch, gamma, within_bound
from tests.train_ops_reference import SWEEP, _adam_data, _bits, _is_f32, bias_corrections, f32


def _hp(hp):
    return tuple(f32(v) if isinstance(v, float) else v for v in hp)


def _kept_bits(got, src, still, what):
    moved = still & (_bits(got) != _bits(src))
    if bool(moved.any()):
        i = int(moved.nonzero()[0])
        return f"{what}[{i}]: an element without update changed its bits ({float(src[i])!r} -> {float(got[i])!r})"
    return None


# ---------------------------------------------------------------------------------------------------
# SGD
# ---------------------------------------------------------------------------------------------------
SGD_HP = [(1e-2, 0.0, 0.0, 0.0, False, 1.0), (1e-2, 0.9, 0.0, 1e-2, True, 1.0 / 3.0), (3e-3, 0.5, 0.25, 0.0, False, 1.0),
          (1e-2, 0.9, 0.125, 1e-3, False, 1.0 / 8.0)]      # (lr, momentum, dampening, weight_decay, nesterov, grad_scale)
SGD_EXACT_HP = [(2.0 ** -3, 0.5, 0.5, 0.25, False, 1.0), (2.0 ** -3, 0.5, 0.0, 0.25, True, 1.0), (2.0 ** -3, 0.0, 0.0, 0.25, False, 1.0)]


def sgd_reference(p, g, buf, first, hp):
    """One torch.optim.SGD step in fp64 from fp32 tensors.  Returns (p', buf' | None without momentum); `buf` is not read on the first step."""
    lr, mom, damp, wd, nesterov, s = hp
    p, g = p.double(), g.double()
    d = g * s
    if wd != 0:
        d = d + wd * p
    if mom == 0:
        return p - lr * d, None
    b = d.clone() if first else mom * buf.double() + (1.0 - damp) * d
    return p - lr * (d + mom * b if nesterov else b), b


def sgd_emulation(p, g, buf, first, hp, damage=None):
    """k_sgd in fp32 torch operations, one rounding per operation.  damage: None | 'dampening_on_first_step' | 'buf_init_dampened' (the same result, the
    issue names both) | 'nesterov_without_momentum_term' | 'decay_after_momentum'."""
    lr, mom, damp, wd, nesterov, s = hp
    assert p.dtype == g.dtype == torch.float32
    keep = float(np.float32(1.0) - np.float32(damp))
    d = g * s
    late = damage == "decay_after_momentum"
    if wd != 0 and not late:
        d = d + p * wd
    if mom == 0:
        return p - d * lr, None
    if first:
        b = d * keep if damage in ("dampening_on_first_step", "buf_init_dampened") else d.clone()
    else:
        b = buf * mom + d * keep
    if nesterov:
        upd = d.clone() if damage == "nesterov_without_momentum_term" else d + b * mom
    else:
        upd = b
    if wd != 0 and late:
        upd = upd + p * wd
    return p - upd * lr, b


def sgd_check(case, p_got, buf_got):
    """None when (p', buf') (fp32; buf' None without momentum) pass the case's checker, else the first offenders."""
    lr, mom, damp, wd, nesterov, s = case["hp"]
    p_got = p_got.detach().cpu().reshape(-1)
    buf_got = None if buf_got is None else buf_got.detach().cpu().reshape(-1)
    if (mom != 0) != (buf_got is not None):
        return "a momentum buffer exactly with momentum"
    ref_p, ref_b = sgd_reference(case["p"], case["g"], case["buf"], case["first"], case["hp"])
    if case["exact"]:
        for name, got, ref in (("buf'", buf_got, ref_b), ("p'", p_got, ref_p)):
            d = first_mismatch(got, ref) if ref is not None else None
            if d:
                return f"{name}: {d}"
        return None
    p, g = case["p"].double(), case["g"].double()
    kd = 3 if wd != 0 else 1
    D = (g * s).abs() + (wd * p).abs()
    if mom == 0:
        bound, target = gamma(kd + 1) * lr * D, ref_p
    else:
        bb = gamma(kd) * D if case["first"] else gamma(kd + 4) * ((mom * case["buf"].double()).abs() + abs(1.0 - damp) * D)
        d = within_bound(buf_got, ref_b, bb)
        if d:
            return f"buf': {d}"
        b1 = buf_got.double()
        if nesterov:
            dd = g * s + (wd * p if wd != 0 else 0.0)
            bound, target = gamma(kd + 3) * lr * (D + (mom * b1).abs()), p - lr * (dd + mom * b1)
        else:
            bound, target = gamma(1) * lr * b1.abs(), p - lr * b1
    still = bound == 0
    bound = torch.where(still, torch.zeros_like(bound), bound + U * p_got.double().abs())
    d = within_bound(p_got, target, bound)
    if d:
        return f"p': {d}"
    return _kept_bits(p_got, case["p"], still, "p'")


@lru_cache(maxsize=2)
def _sgd_data(n, hp_i):
    """|g s| and |buf| exactly 0 or log-uniform in [1e-6, 1e2].  Every element 1 (mod 4) has g = buf = 0 (the normal case of this project), 3 (mod 8) has
    g = 0 alone, 7 (mod 8) buf = 0 alone.  The PROBES -- elements 0, 2, n - 2, n - 1 -- have |g s|, |buf| and |p| within [0.5, 2]: every term of the update
    is of one size there, so a misplaced or missing term shows undiluted.  A third of the other parameters are 0, a third of size 1e-4, a third of size 1."""
    s = _hp(SGD_HP[hp_i])[5]
    gen = torch.Generator().manual_seed(6007 * n + hp_i)

    def mag():
        return 10.0 ** (torch.rand(n, generator=gen, dtype=torch.float64) * 8.0 - 6.0)

    def sign():
        return torch.randint(0, 2, (n,), generator=gen).double() * 2 - 1
    gs, bb = mag() * sign(), mag() * sign()
    p = torch.randn(n, generator=gen, dtype=torch.float64)
    i = torch.arange(n)
    p[i % 3 == 0] = 0.0
    p[i % 3 == 1] *= 1e-4
    probes = sorted({k for k in (0, 2, n - 2, n - 1) if 0 <= k < n})
    zero, g0, b0 = (i % 4 == 1) & (i < n - 2), i % 8 == 3, i % 8 == 7
    for k in probes:
        zero[k] = g0[k] = b0[k] = False
    gs[zero | g0] = 0.0
    bb[zero | b0] = 0.0
    r = torch.rand(3, len(probes), generator=gen, dtype=torch.float64) * 1.5 + 0.5
    sg = torch.randint(0, 2, (3, len(probes)), generator=gen).double() * 2 - 1
    for j, k in enumerate(probes):
        gs[k], bb[k], p[k] = r[0, j] * sg[0, j], r[1, j] * sg[1, j], r[2, j] * sg[2, j]
    if n >= 4:
        p[1] = 0.0          # a zero-gradient element at p = 0: any noise added to it shows
    return dict(p=p.float(), g=(gs / s).float(), buf=bb.float(), zero=zero, probes=probes)


def sgd_case(n, t, hp_i):
    return dict(_sgd_data(n, hp_i), n=n, t=t, first=t == 1, hp=_hp(SGD_HP[hp_i]), hp_i=hp_i, exact=False)


@lru_cache(maxsize=2)
def sgd_exact_case(n, t, hp_i):
    """lr, momentum, dampening and weight_decay powers of two on dyadic data (multiples of 1/64 in [-1, 1]; every fifth gradient 0): every intermediate of the
    kernel is an fp32 value -- proven here -- so p' and buf' are compared bit for bit."""
    hp = SGD_EXACT_HP[hp_i]
    lr, mom, damp, wd, nesterov, s = hp
    gen = torch.Generator().manual_seed(31 * n + hp_i)
    p, g, buf = (torch.randint(-64, 65, (n,), generator=gen).double() / 64 for _ in range(3))
    g[torch.arange(n) % 5 == 2] = 0.0
    first = t == 1
    steps = {"g s": g * s, "wd p": wd * p, "d": g * s + wd * p, "1 - damp": torch.tensor(1.0 - damp)}
    d = steps["d"]
    if mom != 0:
        if not first:
            steps["mom buf"], steps["(1 - damp) d"] = mom * buf, (1.0 - damp) * d
        b = d if first else mom * buf + (1.0 - damp) * d
        steps["buf'"], steps["mom buf'"] = b, mom * b
        upd = d + mom * b if nesterov else b
    else:
        upd = d
    steps["update"], steps["lr update"], steps["p'"] = upd, lr * upd, p - lr * upd
    for name, x in steps.items():
        if not _is_f32(x):
            raise DoesNotClose(f"exact SGD case, n = {n}, t = {t}, set {hp_i}: {name} is not an fp32 value")
    return dict(n=n, t=t, first=first, hp=hp, hp_i=hp_i, exact=True, p=p.float(), g=g.float(), buf=buf.float(), zero=g == 0, probes=[])


SGD_DAMAGES = ("dampening_on_first_step", "buf_init_dampened", "nesterov_without_momentum_term", "decay_after_momentum", "tail_untouched",
               "second_sweep_untouched")


def _untouched(good, srcs, n, kind):
    lo = n - n % 4 if kind == "tail_untouched" else SWEEP
    if lo >= n:
        return None
    bad = tuple(None if x is None else x.clone() for x in good)
    for b, src in zip(bad, srcs):
        if b is not None:
            b[lo:] = src[lo:]
    return bad


def _differs(bad, good):
    return any(a is not None and not torch.equal(_bits(a), _bits(b)) for a, b in zip(bad, good))


def damaged_sgd(case, kind):
    """A deliberately wrong (p', buf') built from the positive-control emulation, or None where the damage does not exist for this case (no dampening, not the
    first step, no nesterov, no weight decay with momentum, no tail, one sweep -- or it leaves every bit as it is)."""
    args = (case["p"], case["g"], case["buf"], case["first"], case["hp"])
    good = sgd_emulation(*args)
    if kind in ("tail_untouched", "second_sweep_untouched"):
        bad = _untouched(good, (case["p"], case["buf"]), case["n"], kind)
    else:
        bad = sgd_emulation(*args, damage=kind)
    return bad if bad is not None and _differs(bad, good) else None


# ---------------------------------------------------------------------------------------------------
# Adam with weight decay
# ---------------------------------------------------------------------------------------------------
ADAMW_HP = [(0.9, 0.999, 1e-8, 1.0, 1e-3, 1e-2, 1), (0.9, 0.999, 1e-8, 1.0, 1e-3, 1e-2, 0), (0.5, 0.9, 1e-3, 1.0 / 3.0, 1e-2, 0.0, 1)]
_ADAM_DATA_SET = [0, 0, 1]      # the hyperparameter set of tests/train_ops_reference.ADAM_HP whose (betas, eps, grad_scale, lr) each row shares
ADAMW_EXACT_HP = (0.5, 0.75, 2.0 ** -10, 1.0, 2.0 ** -10, 2.0 ** -3, 1)
#                 (beta1, beta2, eps, grad_scale, lr, weight_decay, decoupled)


def adamw_reference(p, g, m, v, t, hp):
    """One step of torch.optim.Adam(weight_decay) (decoupled == 0) / torch.optim.AdamW (decoupled != 0) in fp64 from fp32 tensors: (p', m', v')."""
    b1, b2, eps, s, lr, wd, decoupled = hp
    p, g, m, v = (x.double() for x in (p, g, m, v))
    gs = g * s
    if wd != 0:
        if decoupled:
            p = p * (1.0 - lr * wd)
        else:
            gs = gs + wd * p
    m1 = b1 * m + (1.0 - b1) * gs
    v1 = b2 * v + (1.0 - b2) * gs * gs
    bc1, bc2 = bias_corrections(b1, b2, t)
    return p - lr / bc1 * m1 / (v1.sqrt() / math.sqrt(bc2) + eps), m1, v1


def adamw_emulation(p, g, m, v, t, hp, damage=None):
    """k_adamw in fp32 torch operations, one rounding each.  damage: None | 'decay_without_lr' (p *= 1 - wd) | 'other_decay' (coupled where decoupled was
    asked for, and the reverse)."""
    b1, b2, eps, s, lr, wd, decoupled = hp
    assert p.dtype == g.dtype == m.dtype == v.dtype == torch.float32
    if damage == "other_decay":
        decoupled = not decoupled
    gs = g * s
    if wd != 0:
        if decoupled:
            lw = np.float32(wd) if damage == "decay_without_lr" else np.float32(lr) * np.float32(wd)
            p = p * float(np.float32(1.0) - lw)
        else:
            gs = gs + p * wd
    om1, om2 = float(np.float32(1.0) - np.float32(b1)), float(np.float32(1.0) - np.float32(b2))
    m1 = m * b1 + gs * om1
    v1 = v * b2 + (gs * om2) * gs
    bc1, bc2 = bias_corrections(b1, b2, t)
    step = float(np.float32(lr) / np.float32(bc1))
    return p - (m1 * step) / (v1.sqrt() / f32(math.sqrt(bc2)) + eps), m1, v1


def adamw_check(case, p_got, m_got, v_got):
    p_got, m_got, v_got = (x.detach().cpu().reshape(-1) for x in (p_got, m_got, v_got))
    b1, b2, eps, s, lr, wd, decoupled = case["hp"]
    ref_p, ref_m, ref_v = adamw_reference(case["p"], case["g"], case["m"], case["v"], case["t"], case["hp"])
    if case["exact"]:
        for name, got, ref in (("m'", m_got, ref_m), ("v'", v_got, ref_v), ("p'", p_got, ref_p)):
            d = first_mismatch(got, ref)
            if d:
                return f"{name}: {d}"
        return None
    p, g, m, v = (case[k].double() for k in "pgmv")
    coupled = wd != 0 and not decoupled
    kd = 3 if coupled else 1
    D = (g * s).abs() + ((wd * p).abs() if coupled else 0.0)
    d = within_bound(m_got, ref_m, gamma(kd + 4) * ((b1 * m).abs() + (1.0 - b1) * D))
    if d:
        return f"m': {d}"
    d = within_bound(v_got, ref_v, gamma(2 * kd + 5) * ((b2 * v).abs() + (1.0 - b2) * D * D))
    if d:
        return f"v': {d}"
    bc1, bc2 = bias_corrections(b1, b2, case["t"])
    upd = lr / bc1 * m_got.double() / (v_got.double().sqrt() / math.sqrt(bc2) + eps)
    decay = wd != 0 and bool(decoupled)
    p0 = p * (1.0 - lr * wd) if decay else p
    base = gamma(8) * upd.abs() + (gamma(3) * p.abs() * (1.0 + lr * wd) if decay else 0.0)
    still = base == 0
    d = within_bound(p_got, p0 - upd, torch.where(still, torch.zeros_like(base), base + U * p_got.double().abs()))
    if d:
        return f"p': {d}"
    return _kept_bits(p_got, case["p"], still, "p'")


@lru_cache(maxsize=2)
def _adamw_data(n, hp_i):
    """The data of the Adam table (tests/train_ops_reference._adam_data: exact-zero gradients on most elements, probes at both ends where eps is 1e-3 of
    the denominator) with the probes' parameters of the size of the update, lr (0.75 + j / 2) with alternating sign, instead of 0: there the decay -- coupled
    (wd p beside g s) or decoupled (lr wd p beside the update) -- is a visible share of what the checker bounds."""
    d = _adam_data(n, _ADAM_DATA_SET[hp_i])
    lr = _hp(ADAMW_HP[hp_i])[4]
    p = d["p"].clone()
    for j, k in enumerate(d["probes"]):
        p[k] = lr * (0.75 + 0.5 * j) * (1 if j % 2 else -1)
    return dict(d, p=p)


def adamw_case(n, t, hp_i):
    return dict(_adamw_data(n, hp_i), n=n, t=t, hp=_hp(ADAMW_HP[hp_i]), hp_i=hp_i, exact=False)


@lru_cache(maxsize=2)
def adamw_exact_case(n):
    """tests/train_ops_reference.adam_exact_case (t = 1, m = v = 0, beta1 = 1/2, beta2 = 3/4, eps = lr = 2^-10, g = +-(2^k - 2^-10), p a multiple of 1/64) with
    the decoupled decay wd = 2^-3: 1 - lr wd = 1 - 2^-13 and p (1 - 2^-13) are fp32 values, and so is the difference with the update -- proven here."""
    from tests.train_ops_reference import adam_exact_case
    base = adam_exact_case(n)
    b1, b2, eps, s, lr, wd, decoupled = ADAMW_EXACT_HP
    p = base["p"].double()
    steps = {"lr wd": torch.tensor(lr * wd), "1 - lr wd": torch.tensor(1.0 - lr * wd), "p (1 - lr wd)": p * (1.0 - lr * wd)}
    upd = p - base["ref_p"]                      # (the update of the plain case: exact, proven there)
    steps["p'"] = p * (1.0 - lr * wd) - upd
    for name, x in steps.items():
        if not _is_f32(x):
            raise DoesNotClose(f"exact AdamW case, n = {n}: {name} is not an fp32 value")
    case = dict(base, hp=ADAMW_EXACT_HP)
    ref = adamw_reference(case["p"], case["g"], case["m"], case["v"], 1, ADAMW_EXACT_HP)
    if not (torch.equal(ref[0], steps["p'"]) and torch.equal(ref[1], base["ref_m"]) and torch.equal(ref[2], base["ref_v"])):
        raise DoesNotClose(f"exact AdamW case, n = {n}: the fp64 reference rounds")
    return case


ADAMW_DAMAGES = ("decay_without_lr", "other_decay", "tail_untouched", "second_sweep_untouched")


def damaged_adamw(case, kind):
    args = (case["p"], case["g"], case["m"], case["v"], case["t"], case["hp"])
    good = adamw_emulation(*args)
    if kind in ("tail_untouched", "second_sweep_untouched"):
        bad = _untouched(good, (case["p"], case["m"], case["v"]), case["n"], kind)
    elif case["hp"][5] == 0 or (kind == "decay_without_lr" and not case["hp"][6]):
        return None
    else:
        bad = adamw_emulation(*args, damage=kind)
    return bad if bad is not None and _differs(bad, good) else None


# ---------------------------------------------------------------------------------------------------
# gradient norm and clipping
# ---------------------------------------------------------------------------------------------------
NORM_THREADS, NORM_BLOCKS = 256, 256
NORM_SHARE = NORM_THREADS * 4                     # elements of one workgroup in one round of the grid
NORM_ROUND = NORM_BLOCKS * NORM_SHARE             # elements of one round of the full grid: the grid-stride loop starts at this n


def norm_blocks(n):
    """The grid of mshgnn_grad_norm, as include/mshgnn.h documents it."""
    return min(-(-(-(-n // 4)) // NORM_THREADS), NORM_BLOCKS)


def norm_reference(g):
    """sqrt(sum g_i^2): the squares are exact in fp64, math.fsum adds them without error, one rounding in the root."""
    x = g.double().numpy()
    return math.sqrt(math.fsum((x * x).tolist()))


def norm_partials(g):
    """The workgroups' partial sums as k_grad_norm forms them (fp64 numpy)."""
    n = g.numel()
    blocks = norm_blocks(n)
    threads = blocks * NORM_THREADS
    rounds = -(-(-(-n // 4)) // threads)
    x = np.zeros(rounds * threads * 4, dtype=np.float64)
    x[:n] = g.double().numpy()
    x = x.reshape(rounds, threads, 4)
    s = np.zeros(threads, dtype=np.float64)
    for r in range(rounds):
        for e in range(4):
            s = s + x[r, :, e] * x[r, :, e]
    s = s.reshape(blocks * NORM_THREADS // 64, 64)
    lane = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        s = s + s[:, lane ^ m]
    waves = s[:, 0].reshape(blocks, NORM_THREADS // 64)
    part = np.zeros(blocks, dtype=np.float64)
    for k in range(NORM_THREADS // 64):
        part = part + waves[:, k]
    return part


def norm_emulation(g, drop_partial=None):
    t = 0.0
    for b, v in enumerate(norm_partials(g).tolist()):
        if b != drop_partial:
            t += v
    return math.sqrt(t)


def norm_check(case, got):
    got, ref = float(got), case["norm"]
    if case["exact"]:
        return None if got == ref else f"norm: got {got!r}, want {ref!r} bit for bit"
    bound = case["n"] * 2.0 ** -53 * ref
    return None if abs(got - ref) <= bound else f"norm: got {got!r}, want {ref!r}, error {abs(got - ref):.3e}, bound {bound:.3e}"


@lru_cache(maxsize=4)
def norm_case(n, kind):
    """kind 'random': the gradient of the SGD table (mostly exact zeros, magnitudes over eight decades).  'integers': small integers in [-3, 3] -- the sum of
    squares is an integer below 2^53, exact in any order.  'one@k': a single 1.0 at element k (negative: from the end) among zeros: the norm is exactly 1."""
    if kind == "random":
        g = _sgd_data(n, 0)["g"]
    elif kind == "integers":
        g = torch.randint(-3, 4, (n,), generator=torch.Generator().manual_seed(n)).float()
        g[n - 1] = 3.0
    else:
        g = torch.zeros(n)
        g[int(kind[4:])] = 1.0
    exact = kind != "random"
    norm = norm_reference(g)
    if exact:
        x = g.double()
        total = float((x * x).sum())
        if not (total < 2.0 ** 53 and total == math.fsum((x * x).tolist()) and bool((x == x.round()).all())):
            raise DoesNotClose(f"exact norm case, n = {n}: the sum of squares is not an exact integer")
        if kind.startswith("one@") and norm != 1.0:
            raise DoesNotClose("a single 1.0 must have norm 1")
    return dict(n=n, kind=kind, g=g, norm=norm, exact=exact)


def damaged_norm(case):
    """One partial of the norm dropped: the last workgroup's non-zero partial is missing from the sum.  None where no partial is non-zero."""
    part = norm_partials(case["g"])
    nz = np.nonzero(part)[0]
    return None if nz.size == 0 else norm_emulation(case["g"], drop_partial=int(nz[-1]))


def clip_coefficient(norm, max_norm, eps=1e-6, clamp=True):
    c = max_norm / (norm + eps)
    return min(c, 1.0) if clamp else c


def clip_reference(g, norm, max_norm):
    """torch.nn.utils.clip_grad_norm_'s scaling in fp64: g min(1, max_norm / (norm + 1e-6))."""
    return g.double() * clip_coefficient(norm, max_norm)


def clip_emulation(g, norm, max_norm, damage=None):
    """k_grad_clip: the coefficient formed in fp64 and rounded to fp32 once, one fp32 product.  damage: 'no_eps' | 'not_clamped'."""
    c = clip_coefficient(norm, max_norm, eps=0.0 if damage == "no_eps" else 1e-6, clamp=damage != "not_clamped")
    return g * f32(c)


def clip_check(case, got):
    got = got.detach().cpu().reshape(-1)
    c = clip_coefficient(case["norm"], case["max_norm"])
    if c == 1.0:
        same = _bits(got) == _bits(case["g"])
        return None if bool(same.all()) else f"clip: element {int((~same).nonzero()[0])} changed although the norm is below max_norm"
    ref = clip_reference(case["g"], case["norm"], case["max_norm"])
    d = within_bound(got, ref, gamma(2) * ref.abs())
    return f"clip: {d}" if d else None


@lru_cache(maxsize=4)
def clip_case(n, above):
    """The norm case's gradient scaled to a norm of about 0.25 (the 1e-6 of the coefficient is then 4e-6 of it: 30 gamma_2), with -0.0 at element 1 mod 4 of
    every other quad; max_norm = norm / 2 (above: clipped by about a half) or 2 norm (below: every bit must stay)."""
    g = _sgd_data(n, 0)["g"].clone()
    if float(g.abs().max()) == 0:
        g[0] = 1.0
    g = (g.double() * (0.25 / norm_reference(g))).float()
    i = torch.arange(n)
    g[(i % 8 == 1) & (g == 0)] = -0.0
    norm = norm_reference(g)
    return dict(n=n, g=g, norm=norm, max_norm=f32(norm / 2 if above else norm * 2), above=above)


CLIP_DAMAGES = ("no_eps", "not_clamped")


def damaged_clip(case, kind):
    good, bad = clip_emulation(case["g"], case["norm"], case["max_norm"]), clip_emulation(case["g"], case["norm"], case["max_norm"], damage=kind)
    return bad if not torch.equal(_bits(bad), _bits(good)) else None


# ---------------------------------------------------------------------------------------------------
# the GPU tables (tests/test_optim_exact_gpu.py runs them, tests/test_optim_reference.py polices them)
# ---------------------------------------------------------------------------------------------------
S = SWEEP
OPT_N = list(range(1, 10)) + [1023, 1024, 1025, S, S + 3]
OPT_T = [1, 2, 1000]
OPT_EXACT_N = [5, 1027, S + 3]


def all_sgd_cases():
    """('random', n, t, set) for every n x t x the first three hyperparameter sets (the fourth -- dampening, weight decay and grad_scale together -- at three
    n), and ('exact', n, t, exact set) in tail and sweeps."""
    out = [("random", n, t, h) for n in OPT_N for t in OPT_T for h in range(3)]
    out += [("random", n, t, 3) for n in (7, 1025, S + 3) for t in (1, 2)]
    out += [("exact", n, t, h) for n in OPT_EXACT_N for t in (1, 2) for h in range(len(SGD_EXACT_HP))]
    return out


def build_sgd_case(key):
    return sgd_exact_case(*key[1:]) if key[0] == "exact" else sgd_case(*key[1:])


def all_adamw_cases():
    out = [("random", n, t, h) for n in OPT_N for t in OPT_T for h in range(len(ADAMW_HP))]
    out += [("exact", n) for n in OPT_EXACT_N]
    return out


def build_adamw_case(key):
    return adamw_exact_case(key[1]) if key[0] == "exact" else adamw_case(*key[1:])


NORM_N = [1, 3, 4, 5, 255, 256, 257, NORM_SHARE - 1, NORM_SHARE, NORM_SHARE + 1, NORM_ROUND - 1, NORM_ROUND, NORM_ROUND + 1, S + 3]


def all_norm_cases():
    out = []
    for n in NORM_N:
        out += [(n, "random"), (n, "integers"), (n, "one@0"), (n, "one@-1")]
        if n > 8:
            out.append((n, f"one@{n // 2 + 1}"))
    return out


CLIP_N = [1, 5, 1025, S + 3]
