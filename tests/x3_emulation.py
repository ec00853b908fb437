"""Host-side test infrastructure of the graph engines on the split-bf16 parity plan ("x3"): rounding-free data whose LO halves are not zero.

On tests/exact_data.py every operand is a bf16 value, so every lo half, both cross products, the lo planes of every stash and the lo images of every
weight pack run on zeros.  Here one operand class at a time is widened to 9 .. 16 significant bits -- it needs its lo half -- while every product keeps
one factor whose lo is zero: the lo.lo term the kernels drop is then exactly zero, every fp32 sum stays exact, and the split plan (and the fp32 plan, whose
single product is the sum of the three terms) must still reproduce the fp64 oracle BIT FOR BIT, each stored hi and lo plane being split() of the oracle's value.

  split()            v -> (hi, lo) = (bf16(v), bf16(v - hi)), both roundings to nearest even, as split_oct of the kernels (csrc/mshgnn_device.hpp).
  emulate_step_x3()  the kernels' algebra in fp64 (tests/exact_data._kernel_algebra's restructuring with an explicit backward sweep): every operand of a
                     product a (hi, lo) pair, every product hi.hi + lo.hi + hi.lo (left factor: the activation or activation gradient; right factor: the
                     weight image, or the layer input of a weight gradient).  The rounding points, read off the kernels:
                       * the masked fp32 inputs are split while they are staged (k_enc_x3; again by k_gradw_x3_lean and mshgnn_input_grad's W_enc image);
                       * every weight pack is split AFTER the root weights of a destination type are summed in fp32 (prep_one<__bf16, true>); the transposed images
                         of the backward sweep hold the same pairs;
                       * X_0 = split(relu(acc)) (k_enc_x3); X_{l+1} = split(f(H) + (hi + lo of X_l)) (x3_fwd_layer); the ReLU bits are taken from the fp32
                         accumulator (relu_with_bits), on closed data the same as [hi > 0];
                       * base_transform: H is split into LDS and the stash, T1 = split(relu(.)), both products through mlp_mac3; the backward masks dT1
                         with [T1_hi > 0] (the hi half carries the sign), dU and dH are split;
                       * the decoder, its backward and every bias sum are plain fp32 on hi + lo (decoder_tail, k_dec_bwd<__bf16, true>): no cross term exists there;
                       * dX_L = split(g W_dec); dX_l = split(residual + products), layer 0 masked by the encoder's ReLU bits; dH of a ReLU node is both
                         planes of dX_{l+1} masked (chunk_mask_bits);
                       * k_gradw_x3_lean: dW = P_hi Q_hi + P_hi Q_lo + P_lo Q_hi over the stashed planes;
                       * the generic engine (generic=True, csrc/mshgnn_gen.hip) sums a relation's source rows (hi + lo each, fp32) and stages that
                         aggregate as ONE pair in front of the product (gather8 + split_oct), in both sweeps and in its weight gradients;
                       * mshgnn_input_grad: dx = m . (dY_enc (hi, lo) x W_enc (hi, lo)), three products.
                     `drop` = (term, product class) omits one cross term ("lo_hi" or "hi_lo") of one product class; `swap` names one stash whose hi and lo
                     planes are exchanged for everything that reads it.  The damaged variants exist only for the host proof.
  wide_case()        exact_data.exact_case with one operand class widened (the families below); MSE targets rebuilt on the widened output.
  check_wide()       closure of one case, asserted -> (the fp64 oracle reference, the operand classes that carry non-zero lo halves).

Families: "narrow" (exact_case itself), "wide_x" (x += sign(x) j 2^-8, j in 0..3), "wide_gout" (|k| <= 700 units of 2^-14), "wide_enc", "wide_conv<l>",
"wide_dec" (the weight matrices of encoder.*, convs.<l>.*, decoder.* times 1 + 2^-9) and "wide_bt0" / "wide_bt2" (base_transform.0 / .2; only where the base
is a destination in exactly one layer: the shared matrices compound over several).  "wide_bt", both matrices at once, exists for wide_case but closes on no
model: T1 = relu(H W1 + b1) is wide with W1, and meets the wide W2 in the next product -- check_wide refuses it by (a) (and (d)) for every seed.

Product classes (drop): "enc"; "root<l>", "rel<l>", "bt<l>"; "rootT<l>", "relT<l>", "btT<l>" (the backward sweep); "dW_enc", "dW_root<l>", "dW_rel<l>",
"dW_bt<l>"; "dx" (the input gradient).  The decoder has no class: it is plain fp32 on every plan, there is no cross term to drop.
Stashes (swap): "X<l>" (l = 0 .. L - 1 and, on the two-call route, L), "dX<l>" (l = 0 .. L), "T1_<l>".

Operand classes (the set check_wide returns): "X", "X<l>", "dX<l>", "T1_<l>", "W_enc", "W_root<l>", "W_rel<l>", "W_bt" and the transposed images
"W_root<l>T", "W_rel<l>T", "W_btT" (the same pairs, read by the backward sweep), "W_dec" / "W_decT" (fp32 rows, "wide" when they are no bf16 values), and for
the generic engine "agg" / "aggT" (the staged aggregates of the forward and the backward sweep).
A class counts only where the plan computes it: X_l and dX_l on the nodes that are live, weight images of the relations into live types.  The emulation
keeps a stored tensor on the nodes the default plan computes (spec.node_liveness) and zero elsewhere: a row that reaches no output feeds no live row and gets
no gradient, so nothing compared changes, and closure is asked of what the kernels compute, not of rows nobody reads.
"""
import math
import os
from unittest import mock

import torch

from morphsym_hgnn_amd.spec import rel_key
from oracle import ms_hgnn_oracle as orc  # noqa: F401  (the reference of exact_data.reference)
from tests import exact_data as xd
from tests import helpers

WIDE_GOUT_RANGE = 700
WIDE_SCALE = 1 + 2.0 ** -9


def _bf16(t):
    return t.float().to(torch.bfloat16).double()


def split(v):
    """(hi, lo) = (bf16(v), bf16(v - hi)): round to nearest even, twice."""
    v = v.double()
    hi = _bf16(v)
    return hi, _bf16(v - hi)


def _join(p):
    return p[0] + p[1]


def _T(p):
    return p[0].t(), p[1].t()


def _is_fp32(t):
    t = t.double()
    return bool(torch.equal(t.float().double(), t))


class _Run:
    """What one emulation records beside its results: split points that rounded, products whose factors are both wide, sums of |terms| per accumulation."""

    def __init__(self, quant, drop, swap):
        self.quant, self.drop, self.swap = quant, drop, swap
        self.lean = drop is not None or swap is not None      # a damaged variant: values only, no bookkeeping
        self.inexact, self.both_wide, self.sums, self.zeros = [], [], {}, {}
        self.lo_seen = {}      # product class -> [a left factor carries a lo half, a right factor does]

    def sp(self, name, v, rows=None):
        """rows: the nodes (dimension 1) the plan computes -- what rounds on a row nobody computes or reads is no finding"""
        if not self.quant:
            return v, torch.zeros_like(v)
        p = split(v)
        if not self.lean:
            ok = torch.equal(p[0] + p[1], v) if rows is None else torch.equal((p[0] + p[1])[:, rows], v[:, rows])
            if not ok:
                self.inexact.append(name)
        return p

    def sw(self, name, p):
        return (p[1], p[0]) if self.swap == name else p

    def mm3(self, cls, left, right):
        """left (hi, lo) [..., K], right (hi, lo) [N, K] -> ([..., N], the same sum over the pairs' magnitudes, the grid exponent of the products)."""
        (lh, ll), (rh, rl) = left, right
        r = lh @ rh.t()
        d = self.drop[0] if self.drop is not None and self.drop[1] == cls else None
        if d != "lo_hi":
            r = r + ll @ rh.t()
        if d != "hi_lo":
            r = r + lh @ rl.t()
        if self.lean:
            return r, torch.zeros_like(r), math.inf
        wl, wr = bool((ll != 0).any()), bool((rl != 0).any())
        seen = self.lo_seen.setdefault(cls, [False, False])
        seen[0], seen[1] = seen[0] or wl, seen[1] or wr
        if wl and wr:
            self.both_wide.append(cls)
        a = (lh.abs() + ll.abs()) @ (rh.abs() + rl.abs()).t()
        return r, a, min(xd.lsb_exponent(lh), xd.lsb_exponent(ll)) + min(xd.lsb_exponent(rh), xd.lsb_exponent(rl))

    def mm3t(self, cls, p, q):
        """p (hi, lo) [..., O], q (hi, lo) [..., K] -> dW [O, K] = P^T Q summed over every leading index"""
        pf = tuple(t.reshape(-1, t.shape[-1]).t() for t in p)
        qf = tuple(t.reshape(-1, t.shape[-1]).t() for t in q)
        return self.mm3(cls, pf, qf)

    def fits(self, name, abs_sum, grid):
        """an accumulation: the sum of |terms| in units of the finest grid of its terms (asserted below 2^24 by check_wide)"""
        if math.isfinite(grid):
            self.sums[name] = max(self.sums.get(name, 0.0), float(abs_sum.max()) / 2.0 ** grid)


_LEAN = [False]


def _lsb(t):
    return math.inf if _LEAN[0] else xd.lsb_exponent(t)


def _grid_of(*ts):
    return min(_lsb(t) for t in ts)


def emulate_step_x3(spec, params, x, B, gout, drop=None, swap=None, generic=False, quant=True, run=None):
    """The split plan's algebra in fp64 (module docstring).  params / x: the reference's dicts (fp64), gout: [B * n_out * d] or None (forward only).
    Returns dict(out, hidden [X_l = hi + lo, [B, NN, h], l = 0 .. L], hidden_pairs, dx [dX_l, l = 0 .. L], dx_pairs, t1_pairs {l: pair}, w_pairs {name: pair},
    x_pairs {type: pair}, agg_pairs / aggT_pairs (generic), grads {name: tensor}, xgrads {type: [B * n_t, F_t]}, run)."""
    R = run if run is not None else _Run(quant, drop, swap)
    _LEAN[0] = R.lean
    P = {k: v.double() for k, v in params.items()}
    L, nn_, types = spec.num_layers, spec.num_nodes, spec.node_types
    im = spec.input_masks()
    h = spec.hidden
    bt = spec.has_base_transform
    wp = {}

    def w_pair(name, v):
        if name not in wp:
            wp[name] = R.sp(name, v)
        return wp[name]

    def dense(d):
        return (torch.cat([d[t][0] for t in types], 1), torch.cat([d[t][1] for t in types], 1))

    def rels_into(t):
        return [et for et in spec.edge_types if et[2] == t]

    def edge_lists(et):
        e = spec.topology.edges(et)
        sc = xd.mean_scales(spec, et) or [1.0] * len(e)
        return e, sc

    liv, need = liveness(spec)
    LX = [{t: sorted((need[0] if l == 0 else liv[l - 1])[t]) for t in types} for l in range(L + 1)]      # the nodes whose X_l / dX_l the plan computes
    LO = [{t: sorted(liv[l][t]) for t in types} for l in range(L)]                                       # the nodes live in layer l

    def only(pair, t, rows):
        """a stored tensor on the nodes the plan computes; the others (they reach no live node and no gradient reaches them) are zero"""
        k = torch.zeros(nn_[t], dtype=torch.float64)
        k[rows] = 1.0
        return pair[0] * k.view(1, -1, 1), pair[1] * k.view(1, -1, 1)

    # ---- encoder ----
    xp, X, m0 = {}, {}, {}
    for t in types:
        xp[t] = R.sp(f"X.{t}", x[t].double().view(B, nn_[t], -1) * im[t].unsqueeze(0), LX[0][t])
        w = w_pair(f"W_enc.{t}", P[f"encoder.lins.{t}.weight"])
        b = P[f"encoder.lins.{t}.bias"]
        pre, a, g = R.mm3("enc", xp[t], w)
        pre = pre + b
        R.fits(f"enc.{t}", a + b.abs(), min(g, _lsb(b)))
        m0[t] = pre > 0
        R.zeros[-1] = R.zeros.get(-1, 0) + int((pre == 0).sum())
        X[t] = only(R.sp(f"X0.{t}", torch.relu(pre), LX[0][t]), t, LX[0][t])
    Xs = [{t: R.sw("X0", X[t]) for t in types}]
    masks, Hp, T1, agg_f, agg_b = {}, {}, {}, [], []

    # ---- the layers ----
    for l in range(L):
        Xl, new = Xs[l], {}
        for t in spec.live_types(l):
            rels = rels_into(t)
            wr = w_pair(f"W_root{l}.{t}", sum(P[f"convs.{l}.convs.{rel_key(et)}.lin_root.weight"] for et in rels))
            bs = sum(P[f"convs.{l}.convs.{rel_key(et)}.lin_rel.bias"] for et in rels)
            H, A, g = R.mm3(f"root{l}", Xl[t], wr)
            H, A, G = H + bs, A + bs.abs(), min(g, _lsb(bs))
            for et in rels:
                e, sc = edge_lists(et)
                if not e:
                    continue
                w = w_pair(f"W_rel{l}.{rel_key(et)}", P[f"convs.{l}.convs.{rel_key(et)}.lin_rel.weight"])
                src = Xl[et[0]]
                if generic:
                    for i in sorted({i for _, i in e}):
                        s = sum(s_ * _join((src[0][:, j], src[1][:, j])) for (j, i2), s_ in zip(e, sc) if i2 == i)
                        ap = R.sp(f"agg{l}.{rel_key(et)}.{i}", s) if i in LO[l][t] else split(s)
                        agg_f.append(ap if i in LO[l][t] else (ap[0] * 0, ap[1] * 0))
                        m, a, g = R.mm3(f"rel{l}", ap, w)
                        H, A, G = H.index_add(1, torch.tensor([i]), m.unsqueeze(1)), A.index_add(1, torch.tensor([i]), a.unsqueeze(1)), min(G, g)
                else:
                    js, is_ = torch.tensor([j for j, _ in e]), torch.tensor([i for _, i in e])
                    scv = torch.tensor(sc, dtype=torch.float64).view(1, -1, 1)
                    m, a, g = R.mm3(f"rel{l}", (src[0][:, js], src[1][:, js]), w)
                    H, A, G = H.index_add(1, is_, m * scv), A.index_add(1, is_, a * scv), min(G, g)
            R.fits(f"H{l}.{t}", A, G)
            if bt and t == "base":
                Hp[l] = only(R.sp(f"Hb{l}", H, LO[l][t]), t, LO[l][t])
                w1, w2 = w_pair("W_bt.0", P["base_transform.0.weight"]), w_pair("W_bt.2", P["base_transform.2.weight"])
                b1, b2 = P["base_transform.0.bias"], P["base_transform.2.bias"]
                u, a, g = R.mm3(f"bt{l}", Hp[l], w1)
                u = u + b1
                R.fits(f"T1pre{l}", a + b1.abs(), min(g, _lsb(b1)))
                R.zeros[l] = R.zeros.get(l, 0) + int((u == 0).sum())
                T1[l] = R.sw(f"T1_{l}", only(R.sp(f"T1_{l}", torch.relu(u), LO[l][t]), t, LO[l][t]))
                Y, a, g = R.mm3(f"bt{l}", T1[l], w2)
                Y = Y + b2
                R.fits(f"Y{l}", a + b2.abs(), min(g, _lsb(b2)))
            else:
                masks[l, t] = H > 0
                R.zeros[l] = R.zeros.get(l, 0) + int((H == 0).sum())
                Y = torch.relu(H)
            new[t] = only(R.sp(f"X{l + 1}.{t}", Y + _join(Xl[t]) if spec.residual else Y, LO[l][t]), t, LO[l][t])
        Xs.append({t: R.sw(f"X{l + 1}", new[t]) if t in new else only(Xl[t], t, []) for t in types})

    # ---- decoder: plain fp32 on hi + lo ----
    ot = spec.out_type
    om = spec.output_mask().unsqueeze(0)
    xl = _join(Xs[L][ot])
    wd, bd = P["decoder.weight"], P["decoder.bias"]
    out = (xl @ wd.t() + bd) * om
    R.fits("out", xl.abs() @ wd.abs().t() + bd.abs(), min(_lsb(xl) + _lsb(wd), _lsb(bd)))
    res = dict(out=out.reshape(-1), hidden_pairs=[dense(X_) for X_ in Xs], t1_pairs=T1, hb_pairs=Hp, w_pairs=wp, x_pairs=xp, agg_pairs=agg_f, aggT_pairs=agg_b, run=R,
               masks=masks, m0=m0)
    res["hidden"] = [_join(p) for p in res["hidden_pairs"]]
    if gout is None:
        return res

    # ---- backward ----
    grads = {k: torch.zeros_like(v) for k, v in P.items()}
    gsum, ggrid = {}, {}

    def add_grad(name, r, a=None, g=None):
        """a parameter gradient: one accumulation over windows, nodes and edges"""
        grads[name] = grads[name] + r
        if a is not None:
            gsum[name] = gsum.get(name, 0) + a
            ggrid[name] = min(ggrid.get(name, math.inf), g)

    def plain(name, r, terms_abs, grid):
        add_grad(name, r, terms_abs, grid)

    zero = {t: (torch.zeros(B, nn_[t], h, dtype=torch.float64),) * 2 for t in types}
    go = gout.double().view(B, nn_[ot], -1) * om
    plain("decoder.weight", torch.einsum("bnd,bnh->dh", go, xl), torch.einsum("bnd,bnh->dh", go.abs(), xl.abs()), _lsb(go) + _lsb(xl))
    plain("decoder.bias", go.sum((0, 1)), go.abs().sum((0, 1)), _lsb(go))
    R.fits("dX_L", go.abs() @ wd.abs(), _lsb(go) + _lsb(wd))
    dXs = [None] * (L + 1)
    dXs[L] = dict(zero)
    dXs[L][ot] = R.sw(f"dX{L}", R.sp(f"dX{L}.{ot}", go @ wd, LX[L][ot]))
    for l in range(L - 1, -1, -1):
        Gd, Xl = dXs[l + 1], Xs[l]
        acc = {t: torch.zeros(B, nn_[t], h, dtype=torch.float64) for t in types}
        aab = {t: torch.zeros(B, nn_[t], h, dtype=torch.float64) for t in types}
        agr = {t: math.inf for t in types}
        for t in spec.live_types(l):
            G = Gd[t]
            rels = rels_into(t)
            if spec.residual:
                acc[t], aab[t], agr[t] = acc[t] + _join(G), aab[t] + G[0].abs() + G[1].abs(), min(agr[t], _grid_of(*G))
            if bt and t == "base":
                w1, w2 = wp["W_bt.0"], wp["W_bt.2"]
                d1, a, g = R.mm3(f"btT{l}", G, _T(w2))
                R.fits(f"dT1_{l}", a, g)
                dU = R.sp(f"dU{l}", d1 * (T1[l][0] > 0), LO[l][t])
                dh, a, g = R.mm3(f"btT{l}", dU, _T(w1))
                R.fits(f"dHb{l}", a, g)
                dH = R.sp(f"dHb{l}", dh, LO[l][t])
                add_grad("base_transform.2.weight", *R.mm3t(f"dW_bt{l}", G, T1[l]))
                plain("base_transform.2.bias", _join(G).sum((0, 1)), (G[0].abs() + G[1].abs()).sum((0, 1)), _grid_of(*G))
                add_grad("base_transform.0.weight", *R.mm3t(f"dW_bt{l}", dU, Hp[l]))
                plain("base_transform.0.bias", _join(dU).sum((0, 1)), (dU[0].abs() + dU[1].abs()).sum((0, 1)), _grid_of(*dU))
            else:
                mk = masks[l, t].double()
                dH = (G[0] * mk, G[1] * mk)
            r, a, g = R.mm3(f"rootT{l}", dH, _T(wp[f"W_root{l}.{t}"]))
            acc[t], aab[t], agr[t] = acc[t] + r, aab[t] + a, min(agr[t], g)
            gw = R.mm3t(f"dW_root{l}", dH, Xl[t])
            gb = (_join(dH).sum((0, 1)), (dH[0].abs() + dH[1].abs()).sum((0, 1)), _grid_of(*dH))
            for et in rels:
                k = f"convs.{l}.convs.{rel_key(et)}."
                add_grad(k + "lin_root.weight", *gw)
                plain(k + "lin_rel.bias", *gb)
                e, sc = edge_lists(et)
                if not e:
                    continue
                w = wp[f"W_rel{l}.{rel_key(et)}"]
                s_t, src = et[0], Xl[et[0]]
                if generic:
                    for j in sorted({j for j, _ in e}):
                        s = sum(s_ * _join((dH[0][:, i], dH[1][:, i])) for (j2, i), s_ in zip(e, sc) if j2 == j)
                        ap = R.sp(f"aggT{l}.{rel_key(et)}.{j}", s) if j in LX[l][s_t] else split(s)
                        agg_b.append(ap if j in LX[l][s_t] else (ap[0] * 0, ap[1] * 0))
                        r, a, g = R.mm3(f"relT{l}", ap, _T(w))
                        ix = torch.tensor([j])
                        acc[s_t], aab[s_t], agr[s_t] = acc[s_t].index_add(1, ix, r.unsqueeze(1)), aab[s_t].index_add(1, ix, a.unsqueeze(1)), min(agr[s_t], g)
                    for i in sorted({i for _, i in e}):
                        s = sum(s_ * _join((src[0][:, j], src[1][:, j])) for (j, i2), s_ in zip(e, sc) if i2 == i)
                        add_grad(k + "lin_rel.weight", *R.mm3t(f"dW_rel{l}", (dH[0][:, i], dH[1][:, i]), split(s)))
                else:
                    js, is_ = torch.tensor([j for j, _ in e]), torch.tensor([i for _, i in e])
                    scv = torch.tensor(sc, dtype=torch.float64).view(1, -1, 1)
                    r, a, g = R.mm3(f"relT{l}", (dH[0][:, is_], dH[1][:, is_]), _T(w))
                    acc[s_t], aab[s_t], agr[s_t] = acc[s_t].index_add(1, js, r * scv), aab[s_t].index_add(1, js, a * scv), min(agr[s_t], g)
                    add_grad(k + "lin_rel.weight", *R.mm3t(f"dW_rel{l}", (dH[0][:, is_] * scv, dH[1][:, is_] * scv), (src[0][:, js], src[1][:, js])))
        dXs[l] = {}
        for t in types:
            R.fits(f"dX{l}.{t}", aab[t], agr[t])
            v = acc[t] * m0[t].double() if l == 0 else acc[t]
            dXs[l][t] = R.sw(f"dX{l}", R.sp(f"dX{l}.{t}", v, LX[l][t]))
    xg = {}
    for t in types:
        dY = dXs[0][t]
        add_grad(f"encoder.lins.{t}.weight", *R.mm3t("dW_enc", dY, xp[t]))
        plain(f"encoder.lins.{t}.bias", _join(dY).sum((0, 1)), (dY[0].abs() + dY[1].abs()).sum((0, 1)), _grid_of(*dY))
        r, a, g = R.mm3("dx", dY, _T(wp[f"W_enc.{t}"]))
        R.fits(f"dx.{t}", a, g)
        xg[t] = (r * im[t].unsqueeze(0)).reshape(B * nn_[t], -1)
    for name, a in gsum.items():
        R.fits(f"grad {name}", a, ggrid[name])
    res.update(grads=grads, xgrads=xg, dx_pairs=[dense(d) for d in dXs])
    res["dx"] = [_join(p) for p in res["dx_pairs"]]
    return res


# ---------------------------------------------------------------------------------------------------
# the families
# ---------------------------------------------------------------------------------------------------
def liveness(spec):
    """liveness(spec) of the default plan (node-level, MSHGNN_PRUNE unset): what every plan computes, whatever the switch says"""
    with mock.patch.dict(os.environ, {"MSHGNN_PRUNE": "1"}):
        return spec.node_liveness()


def bt_layers(spec):
    """the layers in which base_transform runs (a base node is a destination that can reach the decoder)"""
    return [l for l in range(spec.num_layers) if spec.has_base_transform and liveness(spec)[0][l]["base"]]


def families(spec):
    """every family this model has"""
    f = ["narrow", "wide_x", "wide_gout", "wide_enc"] + [f"wide_conv{l}" for l in range(spec.num_layers)] + ["wide_dec"]
    return f + (["wide_bt0", "wide_bt2"] if len(bt_layers(spec)) == 1 else [])


def wide_case(spec, family, B, seed, **knobs):
    """exact_data.exact_case with one operand class widened.  Nothing is rescaled to make a case close: check_wide refuses what does not."""
    assert family in families(spec) or family.startswith("wide_bt"), family
    if family.startswith("wide_bt"):
        assert len(bt_layers(spec)) == 1, f"wide_bt needs a model whose base_transform runs in exactly one layer, not {bt_layers(spec)}"
    if family == "wide_gout":
        knobs = dict(knobs, gout_range=WIDE_GOUT_RANGE)
    case = xd.exact_case(spec, B, seed, **knobs)
    case["family"] = family
    if family in ("narrow", "wide_gout"):
        return case
    if family == "wide_x":
        g = torch.Generator().manual_seed(seed * 7919 + B)
        for t in spec.node_types:
            v = case["x"][t]
            case["x"][t] = v + torch.sign(v) * torch.randint(0, 4, v.shape, generator=g).double() * 2.0 ** -8
    else:
        prefix = {"wide_enc": "encoder.", "wide_dec": "decoder.", "wide_bt": "base_transform.", "wide_bt0": "base_transform.0.",
                  "wide_bt2": "base_transform.2."}.get(family) or f"convs.{int(family[len('wide_conv'):])}."
        for k, v in case["params"].items():
            if k.startswith(prefix) and v.dim() == 2:
                case["params"][k] = v * WIDE_SCALE
    if case.get("y") is not None:
        out = xd.reference(spec, case)["out"]
        case["y"], case["gout_mse"] = xd._mse_targets(out, seed, knobs.get("gout_range", 2))
    return case


def _live_nodes(spec):
    """per X_l (l = 0 .. L) the dense node indices the plan computes"""
    liv, need = liveness(spec)
    sl = helpers.node_slices(spec)
    return [torch.tensor(sorted(sl[t].start + n for t in spec.node_types for n in (need[0] if l == 0 else liv[l - 1])[t]), dtype=torch.long)
            for l in range(spec.num_layers + 1)]


def operand_classes(spec, em, generic=False, plane=1):
    """{class: [lo planes]} (plane=0: hi planes) of an emulation result, on what the plan computes"""
    live = _live_nodes(spec)
    L = spec.num_layers
    c = {"X": [em["x_pairs"][t][plane] for t in spec.node_types if liveness(spec)[1][0][t]]}
    for l in range(L + 1):
        c[f"X{l}"] = [em["hidden_pairs"][l][plane][:, live[l]]]
        c[f"dX{l}"] = [em["dx_pairs"][l][plane][:, live[l]]]
    liv, need = liveness(spec)
    bl = bt_layers(spec)
    for l, p in em["t1_pairs"].items():
        if l in bl:
            c[f"T1_{l}"] = [p[plane]]
    dest = {rel_key(et): et[2] for et in spec.edge_types}
    for name, p in em["w_pairs"].items():
        k, rest = name.split(".", 1)
        if k == "W_enc":
            ok = bool(need[0][rest])
        elif k == "W_bt":
            ok = bool(bl)
        else:      # W_root<l>.<type>, W_rel<l>.<relation>
            l = int(k[len("W_root"):] if k.startswith("W_root") else k[len("W_rel"):])
            ok = bool(liv[l][rest if k.startswith("W_root") else dest[rest]])
        if not ok:
            continue
        c.setdefault(k, []).append(p[plane])
        if k != "W_enc":
            c.setdefault(k + "T", []).append(p[plane].t())
    if generic:
        c["agg"] = [p[plane] for p in em["agg_pairs"]]
        c["aggT"] = [p[plane] for p in em["aggT_pairs"]]
    return c


def all_classes(spec, generic=False):
    """every operand class the model has on the split plan"""
    L = spec.num_layers
    s = {"X", "W_enc", "W_dec", "W_decT"} | {f"X{l}" for l in range(L + 1)} | {f"dX{l}" for l in range(L + 1)}
    for l in range(L):
        s |= {f"W_root{l}", f"W_root{l}T", f"W_rel{l}", f"W_rel{l}T"}
    if bt_layers(spec):
        s |= {"W_bt", "W_btT"} | {f"T1_{l}" for l in bt_layers(spec)}
    return s | ({"agg", "aggT"} if generic else set())


def named_classes(spec, family, generic=False):
    """{operand class the family must widen: "slices" | "some"} for check_wide (f).  "slices": every 32-feature slice of the class that holds a non-zero
    value at all holds a non-zero lo (a slice of zeros has no lo half to speak of: with one entry per weight row the activation gradients are
    column-sparse, dX_L lives in the out_channels columns W_dec reaches).  "some": the class holds a non-zero lo -- dX_l of wide_conv<l> and T1 / dX of
    wide_bt, where the columns only the (narrow) residual term reaches stay bf16 values by construction."""
    L = spec.num_layers
    bl = bt_layers(spec)
    if family == "narrow":
        return {}
    if family in ("wide_x", "wide_enc"):
        s = {f"X{l}" for l in range(L + 1)} | {f"T1_{l}" for l in bl} | ({"X"} if family == "wide_x" else {"W_enc"}) | ({"agg"} if generic else set())
        return {k: "slices" for k in s}
    if family in ("wide_gout", "wide_dec"):
        s = {f"dX{l}" for l in range(L + 1)} | ({"W_dec", "W_decT"} if family == "wide_dec" else set()) | ({"aggT"} if generic else set())
        return {k: "slices" for k in s}
    if family.startswith("wide_bt"):      # (what the chain feeds reaches the other nodes through the relations out of the base only: "some")
        d = {k: "slices" for k in {"W_bt", "W_btT"}}
        d.update({k: "some" for k in {f"X{m}" for m in range(bl[0] + 1, L + 1)} | {f"dX{m}" for m in range(bl[0] + 1)} | ({f"T1_{bl[0]}"} if family != "wide_bt2" else set())})
        return d
    l = int(family[len("wide_conv"):])
    d = {k: "slices" for k in {f"W_root{l}", f"W_root{l}T", f"W_rel{l}", f"W_rel{l}T"} | {f"X{m}" for m in range(l + 1, L + 1)} | {f"dX{m}" for m in range(l)}}
    d[f"dX{l}"] = "some"
    return d


def _slices_hold(planes, values):
    """every 32-feature slice (last dimension) in which the class holds a non-zero value holds a non-zero lo"""
    width = max(p.shape[-1] for p in planes)
    for c in range(0, width, 32):
        if any(bool((v[..., c:c + 32] != 0).any()) for v in values if v.shape[-1] > c) and not any(bool((p[..., c:c + 32] != 0).any()) for p in planes if p.shape[-1] > c):
            return False
    return True


def compared(spec, res, input_grads=False):
    """what the GPU test compares of a result (oracle reference or emulation), as a flat list of (name, tensor): the output, the hi and lo plane of every
    X_l and dX_l on the live nodes, every parameter gradient, the input gradients"""
    live = _live_nodes(spec)
    items = [("out", res["out"])]
    for l in range(spec.num_layers + 1):
        for what, key in (("X", "hidden_pairs"), ("dX", "dx_pairs")):
            for i, plane in enumerate(("hi", "lo")):
                items.append((f"{what}{l} {plane}", res[key][l][i][:, live[l]]))
    items += [(f"grad {k}", v) for k, v in res["grads"].items()]
    if input_grads:
        items += [(f"xgrad {t}", v) for t, v in res["xgrads"].items()]
    return items


def check_wide(spec, case, gout=None, input_grads=False, generic=False, stats=None):
    """Closure of `case` for output gradient `gout` (default: the case's gout_mse when it has targets, else its gout), asserted (module docstring, (a) .. (f)
    of the issue this file answers) -> (the fp64 oracle reference with the reference planes `hidden_pairs` / `dx_pairs` = split() of its values, the set of
    operand classes with non-zero lo halves)."""
    B = case["B"]
    if gout is None:
        gout = case["gout_mse"] if case.get("gout_mse") is not None else case["gout"]
    stats = {} if stats is None else stats
    ref = xd.reference(spec, case, gout, input_grads=True)
    em = emulate_step_x3(spec, case["params"], case["x"], B, gout, generic=generic)
    R = em["run"]
    live = _live_nodes(spec)
    # (a) the undamaged emulation is the oracle, bit for bit
    assert torch.equal(em["out"], ref["out"]), f"(a) output: {xd.first_difference(em['out'], ref['out'])}"
    for l in range(spec.num_layers + 1):
        d = xd.first_difference(em["hidden"][l][:, live[l]], ref["hidden"][l][:, live[l]])
        assert d is None, f"(a) hidden state X{l}: {d}"
    for k, g in ref["grads"].items():
        d = xd.first_difference(em["grads"][k], g)
        assert d is None, f"(a) gradient {k}: {d}"
    if input_grads:
        for t, g in ref["xgrads"].items():
            d = xd.first_difference(em["xgrads"][t], g)
            assert d is None, f"(a) input gradient {t}: {d}"
    # (b) every packed input and weight image, every stored activation and activation gradient, every staged aggregate is hi + lo exactly
    assert not R.inexact, f"(b) not hi + lo: {sorted(set(R.inexact))[:8]}"
    # (c) every result and every hidden state is an fp32 value
    for name, v in [("out", ref["out"])] + [(f"X{l}", v[:, live[l]]) for l, v in enumerate(ref["hidden"])] + [(f"grad {k}", v) for k, v in ref["grads"].items()] + \
            ([(f"xgrad {t}", v) for t, v in ref["xgrads"].items()] if input_grads else []) + [(k, v) for k, v in case["params"].items()]:
        assert _is_fp32(v), f"(c) {name} is not an fp32 value"
    # (d) every product has a factor whose lo is zero
    assert not R.both_wide, f"(d) both factors carry lo halves in {sorted(set(R.both_wide))}"
    # (e) every accumulation: the sum of (|hi| + |lo|)(|hi| + |lo|) plus bias below 2^24 units of the finest grid of its terms
    worst = max(R.sums.items(), key=lambda kv: kv[1])
    stats["sum_bound"] = (worst[0], worst[1] / 2.0 ** 24)
    assert worst[1] < 2.0 ** 24, f"(e) the sum of |terms| of {worst[0]} is {worst[1] / 2.0 ** 24:.3g} of 2^24 units of its grid"
    # (f) coverage
    live_random = xd._live_nonzero_in_random_case(spec)
    dead_here = sorted(k for k in live_random if float(ref["grads"][k].abs().max()) == 0)
    assert not dead_here, f"(f) gradients live on random data are zero here: {dead_here}"
    for l in range(spec.num_layers + 1):
        X = ref["hidden"][l]
        for n in live[l].tolist():
            for c in range(0, X.shape[-1], 32):
                assert bool((X[:, n, c:c + 32] != 0).any()), f"(f) X{l} node {n}: column slice {c // 32} is all zero"
    for l in [-1] + list(range(spec.num_layers)):
        assert R.zeros.get(l, 0) > 0, f"(f) no exact-zero relu pre-activation in {'the encoder' if l < 0 else f'layer {l}'}"
    if input_grads:
        _, need = liveness(spec)
        masks, neg = spec.input_masks(), 0
        for t in spec.node_types:
            dx = ref["xgrads"][t].view(B, spec.num_nodes[t], -1)
            if not need[0][t]:
                assert float(dx.abs().max()) == 0.0, f"(f) {t}: the encoder computes no node of this type, yet its dx is non-zero"
                continue
            for c in range(0, dx.shape[-1], 16):
                assert bool((dx[..., c:c + 16] != 0).any()), f"(f) {t}: the input gradient is all zero in column tile {c // 16}"
            neg += int(((dx != 0) & (masks[t] < 0).unsqueeze(0)).sum())
        if any(bool((masks[t] < 0).any()) for t in spec.node_types if need[0][t]):
            assert neg > 0, "(f) no negative symmetry sign meets a non-zero input gradient"
    cls = operand_classes(spec, em, generic)
    dec = case["params"]["decoder.weight"]
    wide = {k for k, planes in cls.items() if any(bool((p != 0).any()) for p in planes)}
    if not xd.bf16_exact(dec):
        wide |= {"W_dec", "W_decT"}
    his = operand_classes(spec, em, generic, plane=0)
    for k, how in sorted(named_classes(spec, case.get("family", "narrow"), generic).items()):
        assert k in wide, f"(f) the family's class {k} is not wide"
        if how == "slices" and k not in ("W_dec", "W_decT"):
            assert _slices_hold(cls[k], his[k]), f"(f) the family's class {k} has a 32-feature slice of values without a non-zero lo"
    stats["wide"] = sorted(wide)
    # the reference planes: split() of the oracle's values (equal to the emulation's by (a) and (b))
    ref["hidden_pairs"] = [split(v) for v in ref["hidden"]]
    ref["dx_pairs"] = [tuple(p.clone() for p in pr) for pr in em["dx_pairs"]]
    for l in range(spec.num_layers + 1):      # (the emulation's dX_l are exactly hi + lo by (b): split() of the sum gives the planes back -- asserted)
        s = split(em["dx"][l])
        assert torch.equal(s[0], em["dx_pairs"][l][0]) and torch.equal(s[1], em["dx_pairs"][l][1])
        s = split(em["hidden"][l][:, live[l]])
        assert torch.equal(s[0], em["hidden_pairs"][l][0][:, live[l]]) and torch.equal(s[1], em["hidden_pairs"][l][1][:, live[l]])
    ref["gout"] = gout.clone()
    ref["lo_seen"] = R.lo_seen
    return ref, wide


def damaged_variants(spec, generic=False):
    """every (drop, swap) the host proof must see: each cross term of each product class, each stash's planes exchanged"""
    L, bl = spec.num_layers, bt_layers(spec)
    classes = ["enc", "dW_enc", "dx"]
    for l in range(L):
        classes += [f"root{l}", f"rel{l}", f"rootT{l}", f"relT{l}", f"dW_root{l}", f"dW_rel{l}"]
    for l in bl:
        classes += [f"bt{l}", f"btT{l}", f"dW_bt{l}"]
    v = [dict(drop=(term, c)) for c in classes for term in ("lo_hi", "hi_lo")]
    v += [dict(swap=f"X{l}") for l in range(L + 1)] + [dict(swap=f"dX{l}") for l in range(L + 1)] + [dict(swap=f"T1_{l}") for l in bl]
    return v


def unseeable(spec):
    """the damaged variants no data that closes can show.  Where base_transform runs in more than one layer its two matrices cannot be widened (the shared
    matrices compound over the layers and the rows leave hi + lo: no wide_bt family), so their lo images are zero on every family, and the cross term that
    multiplies them -- hi.lo of the chain's forward and transposed products -- is a sum of zeros whether the kernel forms it or not.  The lo.hi term of the same
    products, and both cross terms of the chain's weight gradients, are seen (T1, H and the gradients through the chain are wide in other families)."""
    bl = bt_layers(spec)
    return [dict(drop=("hi_lo", f"{c}{l}")) for l in bl for c in ("bt", "btT")] if len(bl) > 1 else []


def variant_is_seen(spec, case, ref, variant, input_grads=True, generic=False):
    """a damaged emulation differs from the reference in a quantity the GPU test compares"""
    if "drop" in variant:      # (a cross term whose lo factor is zero in every product of the class on this case: nothing to run)
        term, cls = variant["drop"]
        if not ref["lo_seen"].get(cls, [False, False])[0 if term == "lo_hi" else 1]:
            return False
    em = emulate_step_x3(spec, case["params"], case["x"], case["B"], ref["gout"], generic=generic, **variant)
    good = dict(compared(spec, ref, input_grads))
    return any(not torch.equal(v, good[k]) for k, v in compared(spec, em, input_grads))
