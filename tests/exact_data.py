"""Rounding-free test data for the bf16 plan (test infrastructure, host only).

Every weight matrix has one signed entry per row (+-1, the relation weights scaled by 0.5 or 1), biases are integers, inputs small integers and the
output gradient a few units of 2^-14.  On such data every value the kernels store in bf16 is exactly representable and every fp32 accumulation is exact
in any order, so the bf16, split (x3) and fp32 plans must reproduce the fp64 oracle BIT FOR BIT -- at any batch size, on every kernel set.  A single wrong
element anywhere (a dropped 16-window tile, a mis-indexed 32-feature column slice) is then a failure, where the bf16 plan's tolerance tests
(tests/test_bf16_emulation.py, 1.5e-2 L2) cannot see it.  Every operand being a bf16 value, every lo half of the split plan is ZERO on this data: its cross
products, lo planes and lo weight images are held by tests/x3_emulation.py (this generator with one operand class widened) and tests/test_x3_exact_gpu.py.

`check_exact` proves the three preconditions on the host before it hands out the fp64 reference:
  (a) bf16 closure: the rounding-point emulation with and without rounding and the oracle agree bit for bit, and every activation and activation gradient
      of the kernels' algebra is a bf16 value (so a storage point the emulation does not model rounds nothing either);
  (b) fp32 closure: for every accumulation the sum of the absolute values of its terms fits in 2^24 units of the finest dyadic grid of its terms;
  (c) coverage: every gradient tensor that is live on random data is non-zero, every 32-feature column slice of every live X_l holds non-zero values,
      and every layer has exact-zero relu pre-activations (relu'(0) = 0 is exercised).
With input_grads=True a fourth, for the gradient with respect to the inputs dx = m . (dY_enc @ W_enc) (csrc/mshgnn_input_grad.hip):
  (d) input-gradient closure and coverage: dY_enc is bf16-exact, for every (window, node, feature) the sum of |dY_enc[j]| |W_enc[j][f]| fits in 2^24 units
      of the finest dyadic grid of its terms, every input type the encoder computes has a non-zero dx in every 16-column tile of its width, and a negative
      symmetry sign meets a non-zero element (apply_symmetry's negation is exercised).
"""
import math

import numpy as np
import torch

from morphsym_hgnn_amd.spec import rel_key, relation_aggr
from oracle import ms_hgnn_oracle as orc
from tests import helpers
from tests.bf16_emulation import emulate_step

GOUT_EXP = -14          # output gradients are k * 2^GOUT_EXP, |k| <= gout_range


# ---------------------------------------------------------------------------------------------------
# generator
# ---------------------------------------------------------------------------------------------------
def _signed_rows(g, out_f, in_f, scales, density=1.0):
    """[out_f, in_f] with at most one entry per row (a row holds one with probability `density`): a random column, a random sign, a scale drawn from
    `scales`."""
    w = torch.zeros(out_f, in_f, dtype=torch.float64)
    cols = torch.randint(0, in_f, (out_f,), generator=g)
    sign = torch.randint(0, 2, (out_f,), generator=g).double() * 2 - 1
    sc = torch.tensor(scales, dtype=torch.float64)[torch.randint(0, len(scales), (out_f,), generator=g)]
    keep = (torch.rand(out_f, generator=g, dtype=torch.float64) < density).double()
    w[torch.arange(out_f), cols] = sign * sc * keep
    return w


def exact_case(spec, B, seed, x_range=2, bias_range=(-1, 1), rel_scales=(0.5, 1.0), density=1.0, per_matrix=False, gout_range=2, mse=None,
               enc_cover=False, thin=None, gain=None):
    """Rounding-free inputs, parameters and output gradient for `spec` at batch size B.
    thin: {destination type: row density} for the lin_rel weights of every relation INTO that type (the other matrices keep `density`): a sum over the
    many in-edges of one node (the base of a many-limb robot) then reaches only that share of the destination's features, and what it feeds back into
    its sources stays within bf16's 8 significant bits over the layers.
    gain: {relation name: power of two} multiplying the lin_rel weights of the relations of that name: a 'mean' relation over in-degrees up to 4 with gain 4
    hands its destination whole numbers (W . mean = 4 . sum / degree), where quarters would use up two of bf16's bits in every layer that follows.
    enc_cover: dense encoder columns over zero inputs (`_cover_encoder_tiles`) -- with one entry per row, the few features that carry dY_enc reach only
    a few input columns, and the input gradient of a 900-wide input would be zero in most of its column tiles.
    Returns a dict: x (reference convention, fp64 [B*n_t, F_t]), params, gout (fp64 [B*n_out*d], k * 2^-14), and for the one-call MSE step (mse=True, default
    for regression models) y (fp32-exact targets) and gout_mse: the gradient the fused MSE computes from them, 2 (out - y) * fl32(1 / N) evaluated in fp32,
    every element a short dyadic number (`_mse_targets`)."""
    g = torch.Generator().manual_seed(seed)
    params = {}
    thinned = {f"convs.{l}.convs.{rel_key(et)}.lin_rel.weight": d for et in spec.edge_types for l in range(spec.num_layers)
               for t, d in (thin or {}).items() if et[2] == t}
    for name, shape in spec.param_shapes().items():
        if len(shape) == 2:
            rel = ".lin_rel." in name or ".lin_root." in name
            sc = (rel_scales[int(torch.randint(0, len(rel_scales), (1,), generator=g))],) if (rel and per_matrix) else (rel_scales if rel else (1.0,))
            params[name] = _signed_rows(g, shape[0], shape[1], sc, 1.0 if name.startswith(("encoder.", "decoder.")) else thinned.get(name, density))
        else:
            params[name] = torch.randint(bias_range[0], bias_range[1] + 1, shape, generator=g).double()
    for et in spec.edge_types:
        if et[1] in (gain or {}):
            for l in range(spec.num_layers):
                params[f"convs.{l}.convs.{rel_key(et)}.lin_rel.weight"] *= float(gain[et[1]])
    x = {t: torch.randint(-x_range, x_range + 1, (B * spec.num_nodes[t], spec.widths[t]), generator=g).double() for t in spec.node_types}
    if enc_cover:
        _cover_encoder_tiles(spec, params, x, seed)
    n = B * spec.num_nodes[spec.out_type] * spec.out_channels
    gout = torch.randint(-gout_range, gout_range + 1, (n,), generator=g).double() * 2.0 ** GOUT_EXP
    case = dict(spec=spec, B=B, seed=seed, x=x, params=params, gout=gout, y=None, gout_mse=None)
    if mse if mse is not None else spec.regression:
        out = reference(spec, case)["out"]
        case["y"], case["gout_mse"] = _mse_targets(out, seed, gout_range)
    return case


def _cover_encoder_tiles(spec, params, x, seed):
    """Give every encoder weight matrix a dense column in every 4-column group of the input width that no row's own entry uses: +-1, +-0.5 or +-0.25
    in every row (a generator of its own), and set those input columns to 0 in every window.  Where every group has a free column, the forward, the
    activation gradients and the parameter gradients outside those columns are the unchanged case's (the added weights multiply zeros), but every such
    column of dx is a sum over all K rows of dY_enc."""
    gc = torch.Generator().manual_seed(seed + 7919)
    for t in spec.node_types:
        w = params[f"encoder.lins.{t}.weight"]
        H, F = w.shape
        free = ~(w != 0).any(0)
        cols = []
        for c in range(0, F, 4):
            idx = free[c:c + 4].nonzero()[:, 0] + c
            if idx.numel() == 0 and F > 1:      # (every column of the group in use -- a hidden width above F: the rows using the one taken lose their input)
                idx = torch.arange(c, min(c + 4, F))
            if idx.numel():
                cols.append(idx[torch.randint(0, idx.numel(), (1,), generator=gc)])
        if not cols:
            continue
        z = torch.cat(cols)
        sign = torch.randint(0, 2, (H, z.numel()), generator=gc).double() * 2 - 1
        w[:, z] = sign * torch.tensor([1.0, 0.5, 0.25], dtype=torch.float64)[torch.randint(0, 3, (H, z.numel()), generator=gc)]
        x[t][:, z] = 0.0


def _mse_targets(out, seed, gout_range):
    """Targets y for the fused MSE gradient 2 * (out - y) * inv_n (fp32, left to right, inv_n = fl32(1 / N): csrc/mshgnn.hip, the decoder-backward step
    arguments).  Per element a wanted gradient k 2^-14 (|k| <= gout_range, drawn) and the fp32 targets near out - k N 2^-15 (that one and its neighbours,
    a few ulps either way): the first whose fp32 formula, evaluated on the host as the kernels evaluate it, gives exactly k 2^-14 is kept (none: the
    element keeps y = out, gradient 0).  The oracle is handed those gradients."""
    f32 = np.float32
    o = out.reshape(-1).numpy()
    N = o.size
    inv_n = f32(1.0) / f32(N)
    o32 = o.astype(f32)
    assert np.array_equal(o32.astype(np.float64), o), "the output is not an fp32 value"
    rng = np.random.Generator(np.random.PCG64(seed + 977))
    want = rng.integers(-gout_range, gout_range + 1, size=N).astype(np.float64) * 2.0 ** GOUT_EXP
    base = (o - want * N / 2.0).astype(f32)
    y, go, done = o32.copy(), np.zeros(N), want == 0
    for m in (0, 1, -1, 2, -2, 3, -3, 4, -4, 5, -5, 6, -6, 7, -7, 8, -8):
        ym = base
        for _ in range(abs(m)):
            ym = np.nextafter(ym, f32(np.inf) if m > 0 else f32(-np.inf))
        r = (f32(2.0) * (o32 - ym) * inv_n).astype(np.float64)
        ok = ~done & (r == want)
        y[ok], go[ok] = ym[ok], r[ok]
        done |= ok
    return torch.from_numpy(y.astype(np.float64)), torch.from_numpy(go)


# ---------------------------------------------------------------------------------------------------
# fp64 reference (the oracle, plain torch.relu)
# ---------------------------------------------------------------------------------------------------
def reference(spec, case, gout=None, input_grads=False):
    """The oracle's output, hidden states X_0..X_L ([B, NN, h] in the engine's node order), parameter gradients for output gradient `gout`, with
    input_grads=True the gradients with respect to the inputs (`xgrads`: {type: [B*n_t, F_t]}, the same `gout`) and, when the case has targets, the MSE
    loss."""
    B = case["B"]
    cfg = helpers.oracle_config(spec)
    leaves = {k: v.clone().requires_grad_(True) for k, v in case["params"].items()}
    xl = {k: v.clone().requires_grad_(input_grads) for k, v in case["x"].items()}
    out, hidden = orc.forward(cfg, leaves, xl, spec.topology.edge_index_dict(B), return_hidden=True)
    res = {"out": out.detach().reshape(-1).clone(), "hidden": [helpers.dense_hidden(spec, {t: v.detach() for t, v in h.items()}, B) for h in hidden]}
    if gout is not None:
        out.backward(gout.reshape(out.shape))
        res["grads"] = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()}
        if input_grads:
            res["xgrads"] = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in xl.items()}
    if case.get("y") is not None:
        res["loss"] = float(((res["out"] - case["y"]) ** 2).mean())
    return res


# ---------------------------------------------------------------------------------------------------
# the kernels' algebra (tests/bf16_emulation.py's restructuring, no rounding), with its intermediates
# ---------------------------------------------------------------------------------------------------
def _kernel_algebra(spec, P, x_dict, B, relu_masks=None, reseed=None):
    """Forward of the kernels' algebra (root weights pre-summed per destination type, relation sums per edge) in fp64.  relu_masks=None: relu decisions
    from the values (recorded); otherwise the given decisions.  Returns (out [B*n_out*d], intermediates {name: tensor (grad retained)}, masks, zero counts)."""
    inter, masks, zeros = {}, {}, {}
    nn_ = spec.num_nodes

    def keep(name, v):
        if reseed is not None:
            return _Reseed.apply(v, name, reseed)
        v.retain_grad()
        inter[name] = v
        return v

    def relu(key, h):
        if relu_masks is None:
            m = h.detach() > 0
            masks[key] = m
            zeros[key] = int((h.detach() == 0).sum())
        else:
            m = relu_masks[key]
        return h * m.to(h.dtype)

    im = spec.input_masks()
    X = {}
    for t in spec.node_types:
        x = x_dict[t].view(B, nn_[t], -1) * im[t].unsqueeze(0)
        pre = keep(f"enc.{t}", x @ P[f"encoder.lins.{t}.weight"].t() + P[f"encoder.lins.{t}.bias"])
        X[t] = keep(f"X0.{t}", relu(("enc", t), pre))
    for l in range(spec.num_layers):
        new = {}
        for t in spec.live_types(l):
            rels = [et for et in spec.edge_types if et[2] == t]
            w_root = keep(f"wroot{l}.{t}", sum(P[f"convs.{l}.convs.{rel_key(et)}.lin_root.weight"] for et in rels))
            H = X[t] @ w_root.t() + sum(P[f"convs.{l}.convs.{rel_key(et)}.lin_rel.bias"] for et in rels)
            for et in rels:
                e = spec.topology.edges(et)
                if not e:
                    continue
                js = torch.tensor([j for j, _ in e]); is_ = torch.tensor([i for _, i in e])
                msg = X[et[0]][:, js, :] @ P[f"convs.{l}.convs.{rel_key(et)}.lin_rel.weight"].t()
                sc = mean_scales(spec, et)
                if sc is not None:      # ('mean' over an in-degree above 1: the generic engine's 1 / in-degree, per edge)
                    msg = msg * torch.tensor(sc, dtype=msg.dtype).view(1, -1, 1)
                H = H.index_add(1, is_, msg)
            H = keep(f"H{l}.{t}", H)
            if spec.has_base_transform and t == "base":
                t1 = keep(f"T1pre{l}", H @ P["base_transform.0.weight"].t() + P["base_transform.0.bias"])
                t1 = keep(f"T1{l}", relu(("t1", l), t1))
                Y = keep(f"Y{l}", t1 @ P["base_transform.2.weight"].t() + P["base_transform.2.bias"])
            else:
                Y = keep(f"Y{l}.{t}", relu(("layer", l, t), H))
            new[t] = keep(f"X{l + 1}.{t}", Y + X[t] if spec.residual else Y)
        for t in spec.node_types:
            new.setdefault(t, X[t])
        X = new
    out = X[spec.out_type] @ P["decoder.weight"].t() + P["decoder.bias"]
    out = (out * spec.output_mask().unsqueeze(0)).reshape(-1)
    return out, inter, masks, zeros


def mean_scales(spec, et):
    """Per edge of relation `et` the 1 / in-degree of its destination (repeated edges counted as often as they are listed, as PyG's mean does), or None
    where every scale is 1: an 'add' relation, or a 'mean' one whose destinations all have in-degree 1 (every robot of the reference)."""
    if relation_aggr(spec.kind, et) != "mean":
        return None
    e = spec.topology.edges(et)
    deg = {}
    for _, i in e:
        deg[i] = deg.get(i, 0) + 1
    sc = [1.0 / deg[i] for _, i in e]
    return sc if any(v != 1.0 for v in sc) else None


def aggregates_not_bf16(spec, inter, B):
    """The generic-width engine stages a relation's aggregate (the sum or mean of a destination's source rows, and in the backward pass of the dH rows of a
    source's destinations) as ONE bf16 operand row in front of the product, where the LDS-resident kernels add the products in fp32.  Names of the aggregates
    of live destinations that are not bf16 values (empty: the engine rounds nothing there either).  `inter`: the intermediates of `_kernel_algebra` after
    its backward."""
    live, _ = spec.node_liveness()
    bad = []
    for l in range(spec.num_layers):
        for et in spec.edge_types:
            e = spec.topology.edges(et)
            if not e or f"H{l}.{et[2]}" not in inter:
                continue
            sc = mean_scales(spec, et) or [1.0] * len(e)
            Xs, dH = inter[f"X{l}.{et[0]}"].detach(), inter[f"H{l}.{et[2]}"].grad
            fwd, bwd = {}, {}
            for (j, i), s in zip(e, sc):
                if i not in live[l][et[2]]:
                    continue
                fwd[i] = fwd.get(i, 0) + s * Xs[:, j]
                if dH is not None:
                    bwd[j] = bwd.get(j, 0) + s * dH[:, i]
            bad += [f"sum of X{l}.{et[0]} rows into {et[2]} node {i} ({rel_key(et)})" for i, v in fwd.items() if not bf16_exact(v)]
            bad += [f"sum of dH{l}.{et[2]} rows into {et[0]} node {j} ({rel_key(et)})" for j, v in bwd.items() if not bf16_exact(v)]
    return bad


class _Reseed(torch.autograd.Function):
    """Sums of |terms|, one accumulation at a time: the absolute-value run of the kernels' algebra records what arrives here (forward: the sum of |terms|
    of this intermediate's accumulation over the REAL operands' magnitudes; backward: the same for its gradient) and passes the real magnitudes on."""
    @staticmethod
    def forward(ctx, v, name, rs):
        ctx.name, ctx.rs = name, rs
        rs["fwd"][name] = float(v.max())
        return rs["val"][name].abs().clone()

    @staticmethod
    def backward(ctx, g):
        ctx.rs["bwd"][ctx.name] = float(g.max())
        real = ctx.rs["grad"][ctx.name]
        return (real.abs() if real is not None else torch.zeros_like(g)), None, None


def lsb_exponent(t):
    """Smallest exponent e such that every non-zero element of `t` is an integer multiple of 2^e (+inf for an all-zero tensor)."""
    t = t.detach().double().reshape(-1)
    t = t[t != 0]
    if t.numel() == 0:
        return math.inf
    m, e = torch.frexp(t)
    mi = (m.abs() * 2.0 ** 53).long()
    tz = torch.log2((mi & -mi).double()).long()
    return int((e.long() - 53 + tz).min())


def bf16_exact(t):
    t = t.detach().double()
    return bool(torch.equal(t.to(torch.bfloat16).double(), t))


# ---------------------------------------------------------------------------------------------------
# comparison
# ---------------------------------------------------------------------------------------------------
def first_difference(got, ref):
    """None when `got` (any float dtype, any device) equals `ref` bit for bit after .double() (-0.0 == 0.0), else a description of the first differing
    element and how many differ."""
    got = got.detach().double().cpu().reshape(ref.shape)
    ref = ref.detach().double().cpu()
    if torch.equal(got, ref):
        return None
    bad = (got != ref) | (torch.isnan(got) != torch.isnan(ref))
    idx = tuple(int(i) for i in bad.nonzero()[0])
    return f"{int(bad.sum())} of {ref.numel()} elements differ; first at {idx}: got {float(got[idx])!r}, reference {float(ref[idx])!r}"


def locate(idx, what):
    """Where a hidden-state index (window, node, feature) sits in the kernels' tiling."""
    w, n, f = idx
    return f"{what}: window {w} (tile {w // 16}), node {n}, feature {f} (column slice {f // 32})"


# ---------------------------------------------------------------------------------------------------
# the preconditions
# ---------------------------------------------------------------------------------------------------
def _live_nonzero_in_random_case(spec):
    """Gradient tensors that are non-zero for helpers.random_case at this spec (4 windows: which tensors are live depends on the model, not the batch)."""
    x, y, params = helpers.random_case(spec, 4, seed=1)
    _, _, grads = orc.step(helpers.oracle_config(spec), params, x, spec.topology.edge_index_dict(4), y, 4)
    return {k for k, g in grads.items() if float(g.abs().max()) > 0}


def check_exact(spec, case, gout=None, stats=None, input_grads=False):
    """The fp64 reference for `case` with output gradient `gout` (default: the case's `gout_mse` when it has targets, else its `gout`), after asserting
    the preconditions (a) bf16 closure, (b) fp32 closure and (c) coverage (module docstring); input_grads=True: also the gradients with respect to the
    inputs (`xgrads`) after (d).  `stats`: a dict that receives what was measured."""
    B = case["B"]
    if gout is None:
        gout = case["gout_mse"] if case.get("gout_mse") is not None else case["gout"]
    stats = {} if stats is None else stats
    ref = reference(spec, case, gout, input_grads=input_grads)
    go = gout.clone()

    # (a) bf16 closure: emulation with and without rounding and the oracle, bit for bit
    def lg(out):
        return (out.reshape(-1) * go).sum()
    for quant in (True, False):
        e_out, _, e_grads = emulate_step(spec, case["params"], case["x"], None, B, quant=quant, loss_grad=lg)
        d = first_difference(e_out.reshape(-1), ref["out"])
        assert d is None, f"(a) emulation (quant={quant}) output != oracle: {d}"
        for k, gr in ref["grads"].items():
            d = first_difference(e_grads[k], gr)
            assert d is None, f"(a) emulation (quant={quant}) gradient {k} != oracle (mean aggregation over in-degree != 1, or a rounding): {d}"

    # the kernels' algebra: real values (decisions, intermediates), then absolute values under the same decisions (sums of |terms|)
    P = {k: v.clone().requires_grad_(True) for k, v in case["params"].items()}
    out, inter, masks, zeros = _kernel_algebra(spec, P, case["x"], B)
    assert torch.equal(out.detach(), ref["out"]), "the kernels' algebra != oracle"
    out.backward(go)
    for name, v in inter.items():
        if name.startswith("wroot"):
            continue
        if name.startswith("X") or (name.startswith("T1") and not name.startswith("T1pre")):      # (the others are fp32 accumulators)
            assert bf16_exact(v), f"(a) activation {name} is not a bf16 value"
        if v.grad is not None:
            assert bf16_exact(v.grad), f"(a) activation gradient d{name} is not a bf16 value"
    stats["aggregates_not_bf16"] = aggregates_not_bf16(spec, inter, B)      # (asserted empty by the generic engine's cases: tests/test_exact_data.py)
    # (b) fp32 closure
    acts = [case["x"][t] for t in spec.node_types] + [v for v in inter.values()]
    weights = [v for k, v in case["params"].items() if v.dim() == 2] + [v for k, v in inter.items() if k.startswith("wroot")]
    biases = [v for v in case["params"].values() if v.dim() == 1]
    agrads = [go] + [v.grad for k, v in inter.items() if v.grad is not None and not k.startswith("wroot")]
    e_act, e_w, e_b, e_g = (min(lsb_exponent(t) for t in ts) for ts in (acts, weights, biases, agrads))
    grid_f = min(e_act + e_w, e_b)                   # forward: activation x weight products, biases
    grid_b = e_g + min(e_w, e_act, 0)                # backward: gradient x weight (activation gradients), gradient x activation (weight gradients), bias sums
    Pa = {k: v.abs().clone().requires_grad_(True) for k, v in case["params"].items()}
    rs = {"fwd": {}, "bwd": {}, "val": {k: v.detach() for k, v in inter.items()}, "grad": {k: v.grad for k, v in inter.items()}}
    out_a, _, _, _ = _kernel_algebra(spec, Pa, {t: v.abs() for t, v in case["x"].items()}, B, relu_masks=masks, reseed=rs)
    out_a.backward(go.abs())
    fwd_max = max([float(out_a.detach().max())] + list(rs["fwd"].values()))
    bwd_max = max(list(rs["bwd"].values()) + [float(v.grad.max()) for v in Pa.values() if v.grad is not None])
    stats.update(fwd_sum_bound=fwd_max / 2.0 ** (24 + grid_f), bwd_sum_bound=bwd_max / 2.0 ** (24 + grid_b))
    assert fwd_max <= 2.0 ** (24 + grid_f), f"(b) a forward sum of |terms| {fwd_max} exceeds 2^24 units of 2^{grid_f}"
    assert bwd_max <= 2.0 ** (24 + grid_b), f"(b) a backward sum of |terms| {bwd_max} exceeds 2^24 units of 2^{grid_b}"

    # (c) coverage
    live_random = _live_nonzero_in_random_case(spec)
    dead_here = sorted(k for k in live_random if float(ref["grads"][k].abs().max()) == 0)
    assert not dead_here, f"(c) gradients live on random data are zero here: {dead_here}"
    liv, need = spec.node_liveness()
    sl = helpers.node_slices(spec)
    for l, X in enumerate(ref["hidden"]):
        nodes = need[0] if l == 0 else liv[l - 1]
        for t in spec.node_types:
            for n in nodes[t]:
                xn = X[:, sl[t].start + n]
                for c in range(0, xn.shape[-1], 32):      # (a width that is not a multiple of 32: a ragged last slice)
                    assert bool((xn[:, c:c + 32] != 0).any()), f"(c) X{l} {t} node {n}: column slice {c // 32} is all zero"
    per_layer = {}
    for key, z in zeros.items():
        per_layer[key[1] if key[0] != "enc" else -1] = per_layer.get(key[1] if key[0] != "enc" else -1, 0) + z
    for l in [-1] + list(range(spec.num_layers)):
        assert per_layer.get(l, 0) > 0, f"(c) no exact-zero relu pre-activation in {'the encoder' if l < 0 else f'layer {l}'}"
    stats.update(zero_decisions=sum(zeros.values()), nonzero_grads=sum(1 for g in ref["grads"].values() if float(g.abs().max()) > 0),
                 grads=len(ref["grads"]), nonzero_gout=int((go != 0).sum()), gout=go.numel())
    if input_grads:
        _check_input_grads(spec, case, ref, inter, stats)
    ref["gout"] = go
    return ref


def _check_input_grads(spec, case, ref, inter, stats):
    """(d): dx = m . (dY_enc @ W_enc) closes in fp32 on every plan's operands and covers every 16-column tile and a negative symmetry sign."""
    B = case["B"]
    masks = spec.input_masks()
    _, need = spec.node_liveness()
    bound, neg = 0.0, 0
    for t in spec.node_types:
        dy = inter[f"enc.{t}"].grad                                  # [B, n_t, H]: relu'(X_0) . dX_0, the stash mshgnn_input_grad reads
        assert dy is not None and bf16_exact(dy), f"(d) dY_enc {t} is not a bf16 value"
        W = case["params"][f"encoder.lins.{t}.weight"]              # [H, F]
        grid = lsb_exponent(dy) + lsb_exponent(W)
        if math.isfinite(grid):
            s = float((dy.detach().abs() @ W.abs()).max())
            assert s <= 2.0 ** (24 + grid), f"(d) an input-gradient sum of |terms| {s} ({t}) exceeds 2^24 units of 2^{grid}"
            bound = max(bound, s / 2.0 ** (24 + grid))
        dx = ref["xgrads"][t].view(B, spec.num_nodes[t], -1)
        assert torch.equal(dx, (dy.detach() @ W) * masks[t].unsqueeze(0)), f"(d) the oracle's dx {t} is not m . (dY_enc @ W_enc)"
        if not need[0][t]:
            assert float(dx.abs().max()) == 0.0, f"(d) {t}: the encoder computes no node of this type, yet its dx is non-zero"
            continue
        for c in range(0, dx.shape[-1], 16):
            assert bool((dx[..., c:c + 16] != 0).any()), f"(d) {t}: the input gradient is all zero in column tile {c // 16}"
        neg += int(((dx != 0) & (masks[t] < 0).unsqueeze(0)).sum())
    if any(bool((masks[t] < 0).any()) for t in spec.node_types if need[0][t]):
        assert neg > 0, "(d) no negative symmetry sign meets a non-zero input gradient"
    stats.update(xgrad_sum_bound=bound, xgrad_negative=neg)


# ---------------------------------------------------------------------------------------------------
# the fused cross-entropy steps: cases on which the softmax gradient itself is exact
# ---------------------------------------------------------------------------------------------------
CE_SHIFT = 7            # the decoder's weight and bias times 2^CE_SHIFT: logits that differ at all differ by >= 128
CE_TILE = 16            # windows per tile of the LDS-resident kernels


def _pow2(n):
    return n > 0 and n & (n - 1) == 0


def ce_gout(logits, labels, inv_n):
    """dL/dlogit as the kernels evaluate it in fp32 (m = fmaxf(l0, l1); e_i = expf(l_i - m); se = e0 + e1; g_i = (e_i / se - onehot_i) * inv_n), on the
    host and in the two regimes ONLY in which no correct expf rounds: a tie (e0 = e1 = 1, se = 2, e_i / se = 0.5) and a saturated pair (|l0 - l1| >= 128:
    the smaller exponential is exactly 0 -- e^-128 is far below fp32's smallest denormal -- so se = 1 and e_i / se is 1 or 0).  logits fp64 [R, 2] (fp32
    values), labels [R] in {0, 1}, inv_n an np.float32.  Returns fp64 [R, 2]; any other row raises."""
    f32 = np.float32
    l = logits.numpy().astype(f32)
    assert np.array_equal(l.astype(np.float64), logits.numpy()), "a logit is not an fp32 value"
    d = l[:, 0].astype(np.float64) - l[:, 1].astype(np.float64)
    tie, sat = d == 0, np.abs(d) >= 128.0
    assert bool((tie | sat).all()), f"{int((~(tie | sat)).sum())} logit pairs are neither a tie nor 128 apart: the softmax would round"
    p0 = np.where(tie, f32(0.5), np.where(d > 0, f32(1.0), f32(0.0))).astype(f32)      # e0 / se
    p1 = np.where(tie, f32(0.5), np.where(d < 0, f32(1.0), f32(0.0))).astype(f32)
    lab = labels.numpy().astype(bool)
    g0 = (p0 - np.where(lab, f32(0.0), f32(1.0)).astype(f32)) * inv_n
    g1 = (p1 - np.where(lab, f32(1.0), f32(0.0)).astype(f32)) * inv_n
    return torch.from_numpy(np.stack([g0, g1], axis=1).astype(np.float64))


def ce_regimes(logits, labels):
    """Per row (fp64 logits [R, 2], labels [R]): tie, right (the label is the larger logit), wrong -- boolean tensors."""
    d = logits[:, 0] - logits[:, 1]
    tie = d == 0
    larger = (d < 0).long()
    right = ~tie & (labels.long() == larger)
    return tie, right, ~tie & ~right


def ce_case(spec, B, seed, wrong_share=0.5, label_seed=0, flip_row=None, **knobs):
    """`exact_case` for the one-call cross-entropy step of a two-logit classification model: the decoder's weight and bias times 2^CE_SHIFT, so that
    every (window, output node) is a tie or saturated (asserted), labels drawn per (window, node) from a generator of their own (a saturated row
    is labelled with its smaller logit with probability `wrong_share`, a tie with either), and
      gout_ce  the gradient the kernels' fp32 formula gives there (`ce_gout`: 0, +-1 or +-2 units of 0.5 * inv_n, inv_n = fl32(1 / (B n_out))), asserted
               within 2^-149 per element of the fp64 softmax gradient of the same logits (the true distance is e^-128 / N: fp64 keeps what fp32 drops),
      loss_ce  the fp64 mean cross entropy, loss_terms its fp64 terms,
      labels   int32 [B, n_out], counts {"ties", "right", "wrong"}.
    flip_row: a row of the decoder's weight to negate.  The decoder has one signed entry per row; where l0 - l1 has one sign in every row of a batch (the
    families' seeds: `check_exact_ce` (ii) refuses that), negating one row changes no magnitude -- closure is what it was -- and gives both signs."""
    assert spec.out_channels == 2 and not spec.regression, "a two-logit classification model"
    case = exact_case(spec, B, seed, mse=False, **knobs)
    case["params"]["decoder.weight"] = case["params"]["decoder.weight"] * 2.0 ** CE_SHIFT
    if flip_row is not None:
        case["params"]["decoder.weight"][flip_row] *= -1.0
    case["params"]["decoder.bias"] = case["params"]["decoder.bias"] * 2.0 ** CE_SHIFT
    n_out = spec.num_nodes[spec.out_type]
    logits = reference(spec, case)["out"].view(B * n_out, 2)
    g = torch.Generator().manual_seed(seed * 7907 + 31 + label_seed)
    coin = torch.randint(0, 2, (B * n_out,), generator=g)
    wrong = torch.rand(B * n_out, generator=g, dtype=torch.float64) < wrong_share
    d = logits[:, 0] - logits[:, 1]
    larger = (d < 0).long()
    labels = torch.where(d == 0, coin, torch.where(wrong, 1 - larger, larger))
    inv_n = np.float32(1.0) / np.float32(B * n_out)
    gout = ce_gout(logits, labels, inv_n)
    lg = logits.clone().requires_grad_(True)
    terms = torch.nn.functional.cross_entropy(lg, labels, reduction="none")
    terms.mean().backward()
    err = float((lg.grad - gout).abs().max())
    assert err <= 2.0 ** -149, f"the fp32 softmax gradient is {err} from the fp64 one"
    tie, right, wr = ce_regimes(logits, labels)
    case.update(labels=labels.to(torch.int32).view(B, n_out), gout_ce=gout.reshape(-1), loss_ce=float(terms.detach().mean()), loss_terms=terms.detach(),
                counts=dict(ties=int(tie.sum()), right=int(right.sum()), wrong=int(wr.sum())), ce_gout_err=err, wrong_share=wrong_share)
    return case


def ce_loss_bound(case):
    """What the fused fp32 loss may differ from `loss_ce` by, relative to it.  Without ties every term (m + logf(1)) - l_label is 0 or a multiple of 128 and
    the mean a short dyadic number: 0 (the kernels' loss must be `loss_ce`).  With ties: (gamma_{n+4} + 2^-23), gamma_k = k u / (1 - k u), u = 2^-24, n the
    number of rows -- an fp32 sum of non-negative terms in any fixed order, and one rounding of logf(2) per tie."""
    if case["counts"]["ties"] == 0:
        return 0.0
    u, k = 2.0 ** -24, case["loss_terms"].numel() + 4
    return k * u / (1 - k * u) + 2.0 ** -23


def check_exact_ce(spec, case, ties, stats=None):
    """`check_exact` with the case's cross-entropy gradient, plus the coverage that gradient needs:
      (i)   B * n_out is a power of two (inv_n is one: every non-zero element of gout_ce is +-0.5 inv_n or +-inv_n);
      (ii)  every output node sees both labels; right and wrong rows each occur with both signs of l0 - l1; a case declared `ties` has a tie under
            each label, one declared without has none;
      (iii) from 32 windows on, every regime the case has occurs in the first and in the last 16-window tile;
    and, for the loss, that the sum of the terms is an fp32 value where the test asks for equality (no ties)."""
    B = case["B"]
    n_out = spec.num_nodes[spec.out_type]
    stats = {} if stats is None else stats
    assert _pow2(B * n_out), f"(i) B * n_out = {B * n_out} is not a power of two"
    assert bool((spec.output_mask() == 1).all()), "an output mask other than ones: gout_ce does not model it"
    ref = check_exact(spec, case, gout=case["gout_ce"], stats=stats)
    logits = ref["out"].view(B * n_out, 2)
    labels = case["labels"].reshape(-1).long()
    assert torch.equal(ce_gout(logits, labels, np.float32(1.0) / np.float32(B * n_out)).reshape(-1), case["gout_ce"]), "gout_ce is not this case's"
    tie, right, wrong = ce_regimes(logits, labels)
    pos = logits[:, 0] > logits[:, 1]
    lab2 = labels.view(B, n_out)
    for f in range(n_out):
        assert set(lab2[:, f].tolist()) == {0, 1}, f"(ii) output node {f} sees one label only"
    for name, reg in (("right", right), ("wrong", wrong)):
        assert bool((reg & pos).any()) and bool((reg & ~pos).any()), f"(ii) no {name} row with l0 {'>' if not bool((reg & pos).any()) else '<'} l1"
    if ties:
        assert bool((tie & (labels == 0)).any()) and bool((tie & (labels == 1)).any()), "(ii) declared with ties: no tie under each label"
    else:
        assert not bool(tie.any()), "(ii) declared without ties, yet it has some"
    if B >= 2 * CE_TILE:
        for name, reg in (("tie", tie), ("right", right), ("wrong", wrong)):
            r = reg.view(B, n_out)
            if bool(reg.any()):
                assert bool(r[:CE_TILE].any()) and bool(r[(B - 1) // CE_TILE * CE_TILE:].any()), f"(iii) no {name} row in the first or in the last tile"
    t = case["loss_terms"]
    if not ties:
        s = float(t.sum())
        assert bool((t == torch.round(t / 128.0) * 128.0).all()) and s <= 2.0 ** 24 * 128.0, "the loss terms are not multiples of 128 whose sum fp32 holds"
        assert float(np.float32(case["loss_ce"])) == case["loss_ce"], "the mean loss is not an fp32 value"
    else:      # the bound covers a tie's own roundings too: (m + logf(2)) - m rounds at m's magnitude (half an ulp of |m| + 1), logf within 2 ulps of log 2
        u, s = 2.0 ** -24, float(t.sum())
        own = float(((logits[tie, 0].abs() + 1.0) * u + 2 * u).sum())
        n = t.numel()
        assert own + (n - 1) * u / (1 - (n - 1) * u) * s <= ce_loss_bound(case) * s, "the ties' own roundings do not fit the loss bound"
    stats.update(case["counts"], loss_bound=ce_loss_bound(case))
    ref["loss"] = case["loss_ce"]
    return ref


def ce_damaged_variants(spec, case):
    """(name, gout) of what a subtly wrong cross-entropy tail would hand the backward pass on this case -- each is run through the reference and must change a
    compared gradient (tests/test_exact_data.py).  The output mask of channel dd taken for dd ^ 1 is not among them: `check_exact_ce` asserts that the mask
    is all ones on every model with two logits, so that exchange changes nothing there."""
    B = case["B"]
    n_out = spec.num_nodes[spec.out_type]
    N = B * n_out
    inv_n = np.float32(1.0) / np.float32(N)
    logits = reference(spec, case)["out"].view(N, 2)
    labels = case["labels"].long()
    good = case["gout_ce"].view(B, n_out, 2)
    tile = (B - 1) // CE_TILE      # the last tile (the only one below 17 windows)
    rows = slice(tile * CE_TILE, min(B, (tile + 1) * CE_TILE))

    lab = labels.clone()      # one foot's labels from the next window, on one tile
    lab[rows, 1] = torch.roll(labels[:, 1], -1, 0)[rows]
    yield "labels of one foot from the next window on one tile", ce_gout(logits, lab.reshape(-1), inv_n).reshape(-1)
    g = good.clone()
    g[:, 2] = good[:, 2].flip(-1)
    yield "the two logits' gradients exchanged on one foot", g.reshape(-1)
    yield "inv_n of a 64-window sub-step", ce_gout(logits, labels.reshape(-1), np.float32(1.0) / np.float32(64 * n_out)).reshape(-1)
    g = good.clone()
    g[rows] = 0.0
    yield "one 16-window tile left out", g.reshape(-1)
