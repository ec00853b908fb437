"""Host-side test infrastructure of the fused MLP on the split-bf16 parity plan (engine.MLPEngine(dtype="x3"), the k_mlp_*_x3 kernels of
csrc/mshgnn_mlp.hip), built on tests/mlp_reference.py.

  split()        v -> (hi, lo) = (bf16(v), bf16(v - hi)), both roundings to nearest even, as the kernels split.
  emulate_x3()   the kernels' algebra in fp64: every operand of a product a (hi, lo) pair, every product the three terms hi hi + lo hi + hi lo (left factor
                 first: the activation or activation gradient; right factor: the weight, or the layer input in a weight gradient).  `drop` omits one cross
                 term and `swap` exchanges the hi and lo planes of one stash: the damaged variants.
  reference_with_decisions()   the fp64 forward and backward under GIVEN ReLU decisions (the engine's, read from its stashes), with the pre-activations.
  family_case()  rounding-free data over mr.exact_case whose operands carry non-zero lo halves: in every family one operand class is wide (10 to 16
                 significant bits), yet every product has one factor with lo = 0, so the dropped lo lo term is zero and the kernels must equal fp64 bit for
                 bit.  "narrow" is mr.exact_case itself (lo = 0 everywhere).
  check_family() closure of one case on the host (the emulation equals the fp64 reference bit for bit, every stored value is hi + lo exactly, every result
                 is an fp32 value, every accumulation fits 2^24 units of its grid: in any order for a layer's sum over K, per row slab for a weight gradient, whose slabs are then
                 added in slab order) and the operand classes that carry non-zero lo halves.
"""
import numpy as np
import torch
from torch import nn

from tests import mlp_reference as mr
from tests.exact_data import GOUT_EXP, _mse_targets

FAMILIES = ("narrow", "wide_x", "wide_dz", "wide_w1", "wide_w2", "wide_wL")
WIDE_DZ_RANGE = 700      # gout = k 2^GOUT_EXP, |k| <= 700: ten significant bits


def split(t):
    t = t.double()
    hi = mr.bf16(t)
    return hi, mr.bf16(t - hi)


def _mm3(left, right, drop=None):
    """left (hi, lo) [M, K], right (hi, lo) [N, K] -> [M, N]: hi hi + lo hi + hi lo."""
    (lh, ll), (rh, rl) = left, right
    r = lh @ rh.t()
    if drop != "lo_hi":
        r = r + ll @ rh.t()
    if drop != "hi_lo":
        r = r + lh @ rl.t()
    return r


def _loss_gradient(out, loss, target):
    if loss == "mse":
        d = out - target.double()
        return (d * d).mean(), 2 * d / d.numel()
    lo = out.reshape(-1, 2); t = target.reshape(-1).long()
    return nn.functional.cross_entropy(lo, t), ((torch.softmax(lo, 1) - nn.functional.one_hot(t, 2).double()) / lo.shape[0]).view_as(out)


def emulate_x3(params, x, gout=None, loss=None, target=None, drop=None, swap=None):
    """The split kernels' algebra in fp64.  drop: None, "lo_hi" or "hi_lo" (that cross term of EVERY product is omitted); swap: None or l (1-based): the
    hi and lo planes of the stash A_l are exchanged for everything that reads it.  Returns dict(out, acts [A_l = hi + lo], act_pairs, zs [Z_l + b_l], loss,
    grads [(dW, db)], dz [dZ_l = hi + lo], dz_pairs, x_pair, w_pairs)."""
    L = len(params)
    xp = split(x)
    wp = [split(W) for W, _ in params]
    bs = [b.double() for _, b in params]
    a, pairs, zs = xp, [], []
    for i in range(L):
        z = _mm3(a, wp[i], drop) + bs[i]
        zs.append(z)
        if i < L - 1:
            a = split(torch.relu(z))
            if swap == i + 1:
                a = (a[1], a[0])
            pairs.append(a)
    out = zs[-1]
    res = dict(out=out, acts=[h + l for h, l in pairs], act_pairs=pairs, zs=zs, loss=None, grads=None, dz=None, dz_pairs=None, x_pair=xp, w_pairs=wp)
    if loss is not None:
        res["loss"], g = _loss_gradient(out, loss, target)
    elif gout is not None:
        g = gout.double().view_as(out)
    else:
        return res
    dz = split(g)
    grads, dzs = [None] * L, [None] * L
    for i in range(L - 1, -1, -1):
        dzs[i] = dz
        a_in = pairs[i - 1] if i > 0 else xp
        grads[i] = (_mm3((dz[0].t(), dz[1].t()), (a_in[0].t(), a_in[1].t()), drop), (dz[0] + dz[1]).sum(0))
        if i > 0:
            dz = split(_mm3(dz, (wp[i][0].t(), wp[i][1].t()), drop) * (pairs[i - 1][0] > 0))      # the mask: [hi > 0] of the stashed pair
    res["grads"], res["dz"], res["dz_pairs"] = grads, [h + l for h, l in dzs], dzs
    return res


def reference_with_decisions(params, x, masks, gout=None, loss=None, target=None):
    """fp64 forward and backward of the MLP with relu(z) replaced by z . masks[l] (bool [B, hidden], l = 0 .. L - 2) in both directions.  Returns
    dict(out, zs [pre-activations of every layer], loss, grads [(dW, db)])."""
    L = len(params)
    a, ins, zs = x.double(), [], []
    for i, (W, b) in enumerate(params):
        ins.append(a)
        z = a @ W.double().t() + b.double()
        zs.append(z)
        if i < L - 1:
            a = z * masks[i].double()
    out = zs[-1]
    res = dict(out=out, zs=zs, loss=None, grads=None)
    if loss is not None:
        res["loss"], g = _loss_gradient(out, loss, target)
    elif gout is not None:
        g = gout.double().view_as(out)
    else:
        return res
    grads = [None] * L
    for i in range(L - 1, -1, -1):
        grads[i] = (g.t() @ ins[i], g.sum(0))
        if i > 0:
            g = (g @ params[i][0].double()) * masks[i - 1].double()
    res["grads"] = grads
    return res


# ---------------------------------------------------------------------------------------------------
# the exact families
# ---------------------------------------------------------------------------------------------------
def family_case(family, in_channels, history, hidden, num_layers, out_channels, B, seed=mr.SEED):
    """mr.exact_case with one operand class widened (None: the family does not exist at this depth).  y / gout_mse are rebuilt for the widened data."""
    if family == "wide_w2" and num_layers < 3:
        return None
    case = mr.exact_case(in_channels, history, hidden, num_layers, out_channels, B, seed, gout_range=WIDE_DZ_RANGE if family == "wide_dz" else 2)
    case["family"] = family
    if family in ("narrow", "wide_dz"):
        return case
    if family == "wide_x":
        g = torch.Generator().manual_seed(seed * 7919 + in_channels + B)
        x = case["x"]
        case["x"] = x + torch.sign(x) * torch.randint(0, 4, x.shape, generator=g).double() * 2.0 ** -8
        case.pop("series"); case.pop("starts")      # (the rows are no windows of the series any more; the split plan has no series form)
    else:
        i = {"wide_w1": 0, "wide_w2": 1, "wide_wL": num_layers - 1}[family]
        W, b = case["params"][i]
        case["params"] = list(case["params"])
        case["params"][i] = (W * (1 + 2.0 ** -9), b)
    out = mr.reference(case["params"], case["x"])["out"]
    y, gm = _mse_targets(out, seed, 2)
    case["y"], case["gout_mse"] = y.view(B, out_channels), gm.view(B, out_channels)
    return case


def _grid(*ts):
    """the coarsest power of two that divides every entry of the tensors (1.0 when all are zero)"""
    e_min = None
    for t in ts:
        v = t.double().reshape(-1).numpy()
        v = v[v != 0]
        if v.size == 0:
            continue
        m, e = np.frexp(v)
        mi = np.abs(m * 2.0 ** 53).astype(np.int64)
        low = np.log2((mi & -mi).astype(np.float64)).astype(np.int64)
        k = int((e.astype(np.int64) - 53 + low).min())
        e_min = k if e_min is None else min(e_min, k)
    return 2.0 ** (e_min if e_min is not None else 0)


def _is_pair_exact(t):
    h, l = split(t)
    return bool(torch.equal(h + l, t.double()))


def _is_fp32(t):
    return bool(torch.equal(t.double().float().double(), t.double()))


def _fits(left, right, extra=None):
    """sum over k of (|hi| + |lo|)(|hi| + |lo|) (+ |extra|) stays below 2^24 units of the products' grid: the fp32 sum of the three split products is exact
    in any order"""
    (lh, ll), (rh, rl) = left, right
    grid = _grid(lh, ll) * _grid(rh, rl)
    s = (lh.abs() + ll.abs()) @ (rh.abs() + rl.abs()).t()
    if extra is not None:
        grid = min(grid, _grid(extra))
        s = s + extra.abs()
    return bool((s / grid).max() < 2.0 ** 24)


def slab_bounds(B):
    """the row slabs of the weight-gradient launch (csrc/mshgnn_mlp.hip, mlp_layout: at most 8 slabs of at least 2048 rows, whole 32-row tiles); the reduce
    launch adds the slabs' sums in slab order"""
    nslab = min(8, max(1, -(-B // 2048)))
    rows = -(-(-(-B // nslab)) // 32) * 32
    return [(r0, min(r0 + rows, B)) for r0 in range(0, B, rows)]


def _fits_over_rows(dz, a_in, B):
    """a weight-gradient sum: inside a slab the three split products of every row may be added in any order (each slab's sum of |terms| stays below 2^24
    units of the grid); the slabs' exact sums are then added in slab order, and every prefix of that sum is an fp32 value"""
    grid = _grid(*dz) * (_grid(*a_in) if a_in is not None else 1.0)
    prefix = None
    for r0, r1 in slab_bounds(B):
        zh, zl = dz[0][r0:r1], dz[1][r0:r1]
        if a_in is None:
            s_abs, s = (zh.abs() + zl.abs()).sum(0), (zh + zl).sum(0)
        else:
            ah, al = a_in[0][r0:r1], a_in[1][r0:r1]
            s_abs, s = (zh.abs() + zl.abs()).t() @ (ah.abs() + al.abs()), (zh + zl).t() @ (ah + al)
        if not bool((s_abs / grid).max() < 2.0 ** 24):
            return False
        prefix = s if prefix is None else prefix + s
        if not _is_fp32(prefix):
            return False
    return True


def check_family(case, gout_key="gout"):
    """Closure of one case (asserted) -> (the fp64 reference for case[gout_key], the set of operand classes with non-zero lo halves).  Classes: "X", "A<l>",
    "dZ<l>", "W<l>" (the forward image of layer l), "W<l>T" (the transposed image of the backward sweep, l >= 2)."""
    params, x, gout = case["params"], case["x"], case[gout_key]
    L = len(params)
    ref = mr.reference(params, x, gout=gout)
    em = emulate_x3(params, x, gout=gout)
    for a, b in zip(mr._tensors(ref), mr._tensors(em)):
        assert torch.equal(a, b), "the three-product emulation differs from the fp64 reference"
    # every stored value is hi + lo exactly, every result an fp32 value
    assert _is_pair_exact(x) and all(_is_pair_exact(W) for W, _ in params), "an input or a weight is not hi + lo"
    assert all(_is_pair_exact(torch.relu(z)) for z in em["zs"][:-1]), "an activation is not hi + lo"
    g = gout.double()
    for i in range(L - 1, -1, -1):      # the unsplit activation gradients, rebuilt from the reference
        assert _is_pair_exact(g), f"dZ_{i + 1} is not hi + lo"
        assert torch.equal(em["dz"][i], g)
        if i > 0:
            g = (g @ params[i][0].double()) * (ref["acts"][i - 1] > 0)
    assert _is_fp32(ref["out"]) and all(_is_fp32(t) for dW, db in ref["grads"] for t in (dW, db)) and all(_is_fp32(b) for _, b in params), "a result is not an fp32 value"
    # every product has a factor with lo = 0 (the dropped lo lo term is zero), every accumulation fits 2^24 units of its grid
    a_in = em["x_pair"]
    for i in range(L):
        wp, dz = em["w_pairs"][i], em["dz_pairs"][i]
        assert not bool((a_in[1] != 0).any()) or not bool((wp[1] != 0).any()), f"forward product of layer {i + 1}: both factors are wide"
        assert not bool((dz[1] != 0).any()) or not bool((a_in[1] != 0).any()), f"dW_{i + 1}: both factors are wide"
        assert _fits(a_in, wp, params[i][1].double()), f"forward sum of layer {i + 1}"
        assert _fits_over_rows(dz, a_in, x.shape[0]), f"dW sum of layer {i + 1}"
        assert _fits_over_rows(dz, None, x.shape[0]), f"db sum of layer {i + 1}"
        if i > 0:
            assert not bool((dz[1] != 0).any()) or not bool((wp[1] != 0).any()), f"backward product of layer {i + 1}: both factors are wide"
            assert _fits(dz, (wp[0].t(), wp[1].t())), f"dA sum of layer {i + 1}"
        if i < L - 1:
            a_in = em["act_pairs"][i]
    wide = set()
    if bool((em["x_pair"][1] != 0).any()):
        wide.add("X")
    for i in range(L):
        if bool((em["w_pairs"][i][1] != 0).any()):
            wide.add(f"W{i + 1}")
            if i > 0:
                wide.add(f"W{i + 1}T")
        if bool((em["dz_pairs"][i][1] != 0).any()):
            wide.add(f"dZ{i + 1}")
        if i < L - 1 and bool((em["act_pairs"][i][1] != 0).any()):
            wide.add(f"A{i + 1}")
    return ref, wide


def named_classes(family, L):
    """the operand classes a family must widen"""
    if family == "narrow":
        return set()
    if family == "wide_x":
        return {"X"} | {f"A{l}" for l in range(1, L)}
    if family == "wide_dz":
        return {f"dZ{l}" for l in range(1, L + 1)}
    if family == "wide_w1":
        return {"W1"} | {f"A{l}" for l in range(1, L)}
    if family == "wide_w2":
        return {"W2", "W2T", "dZ1"} | {f"A{l}" for l in range(2, L)}
    return {f"W{L}", f"W{L}T"} | {f"dZ{l}" for l in range(1, L)}


def all_classes(L):
    """what the families cover between them: X, every A_l and dZ_l, the K-padded input image, a hidden image and the output image with their transposes"""
    s = {"X", "W1", f"W{L}", f"W{L}T"} | {f"A{l}" for l in range(1, L)} | {f"dZ{l}" for l in range(1, L + 1)}
    return s | ({"W2", "W2T"} if L >= 3 else set())


def damaged_variants(case, gout_key="gout"):
    """(name, emulate_x3 result): a dropped cross term, the planes of the input-layer stash exchanged"""
    p, x, g = case["params"], case["x"], case[gout_key]
    return [("lo_hi", emulate_x3(p, x, gout=g, drop="lo_hi")), ("hi_lo", emulate_x3(p, x, gout=g, drop="hi_lo")), ("swap", emulate_x3(p, x, gout=g, swap=1))]
