"""Host-side test infrastructure of the MLP baselines (morphsym_hgnn_amd.engine.MLPEngine, csrc/mshgnn_mlp.hip).

  reference()    the fp64 reference: torch nn.Sequential in fp64 with its autograd.
  emulate()      the rounding-point emulation of the fused path: fp64 arithmetic with a bf16 rounding exactly where the kernels round (DESIGN.md section 8:
                 every weight, A_l = relu(Z_l + b_l) for l < L, dZ_L = the output gradient, dZ_l for l < L).  quant=False rounds nowhere.  The `damage`
                 argument builds the wrong results a broken kernel would give (a dropped K chunk, a dropped row tile, a transposed weight, a skipped bias).
  exact_case()   rounding-free data in the manner of tests/exact_data.py: the rows are windows of an integer series (entries +-1, +-2), W_1 has one +-1 entry
                 per COLUMN (column i feeds hidden unit i mod H), the hidden layers are signed permutations (three signs in four positive), output row j adds the units i = j mod out with
                 signs, biases are integers in [-1, 1], and the output gradient is k 2^-14.  Every stored bf16 value is then exact and every fp32 sum exact in
                 any order, so the kernels must reproduce the fp64 reference bit for bit.
  check_exact()  proves closure and coverage of one case on the host and returns the reference; compare() is the checker the GPU tests and the damaged
                 variants go through.
"""
import numpy as np
import torch
from torch import nn

from tests.exact_data import GOUT_EXP, _mse_targets

# (in_channels, history T, hidden, num_layers, out_channels, batches): the matrix of tests/test_mlp_exact_gpu.py; in_channels = T x columns
EXACT_MATRIX = [
    (24, 1, 128, 2, 6, (1, 17)),
    (35, 7, 128, 3, 4, (16, 17, 1000)),
    (450, 150, 128, 3, 4, (17, 1000, 8193)),
    (450, 150, 384, 3, 8, (17,)),
    (1200, 8, 256, 8, 8, (17, 1000)),
    (8100, 150, 128, 8, 8, (17,)),
    (8100, 150, 512, 2, 4, (17,)),
]
SEED = 11      # one seed closes every row (tests/test_mlp_reference.py proves it per (shape, batch))


def layer_dims(in_channels, hidden, out_channels, num_layers):
    return [(hidden if i < num_layers - 1 else out_channels, in_channels if i == 0 else hidden) for i in range(num_layers)]


def sequential(in_channels, hidden, out_channels, num_layers, activation=None):
    """The reference's module (gnnLightning.py:391-405)."""
    mods = []
    for i, (o, k) in enumerate(layer_dims(in_channels, hidden, out_channels, num_layers)):
        mods.append(nn.Linear(k, o))
        if i < num_layers - 1:
            mods.append(activation if activation is not None else nn.ReLU())
    return nn.Sequential(*mods)


def flatten(params):
    """[(W, b)] -> the flat buffer in state_dict order (0.weight, 0.bias, 2.weight, ...)."""
    return torch.cat([t.reshape(-1) for W, b in params for t in (W, b)])


def unflatten(flat, dims):
    out, o = [], 0
    for (of, kf) in dims:
        W = flat[o:o + of * kf].view(of, kf); o += of * kf
        b = flat[o:o + of]; o += of
        out.append((W, b))
    return out


def bf16(t):
    return t.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def is_bf16(t):
    return bool(torch.equal(bf16(t), t.to(torch.float64)))


def reference(params, x, gout=None, loss=None, target=None):
    """fp64 nn.Sequential + autograd.  gout: dL/d out; or loss = "mse" / "ce" with target.  Returns dict(out, acts [A_1 ..], loss, grads [(dW, db)])."""
    ps = [(W.detach().double().clone().requires_grad_(True), b.detach().double().clone().requires_grad_(True)) for W, b in params]
    a, acts = x.double(), []
    for i, (W, b) in enumerate(ps):
        a = a @ W.t() + b
        if i < len(ps) - 1:
            a = torch.relu(a)
            acts.append(a.detach())
    out = a
    res = dict(out=out.detach(), acts=acts, loss=None, grads=None)
    if loss == "mse":
        lv = ((out - target.double()) ** 2).mean()
    elif loss == "ce":
        lv = nn.functional.cross_entropy(out.reshape(-1, 2), target.reshape(-1).long())
    elif gout is not None:
        lv = (out * gout.double().view_as(out)).sum()
    else:
        return res
    lv.backward()
    res["loss"] = lv.detach() if loss else None
    res["grads"] = [(W.grad, b.grad) for W, b in ps]
    return res


def emulate(params, x, gout=None, loss=None, target=None, quant=True, damage=None):
    """The kernels' algebra in fp64 with their bf16 rounding points.  damage: None or one of ("k_chunk", k0, k1) -- input columns [k0, k1) never reach the
    input layer or dW_1; ("row_tile", r0, r1) -- rows [r0, r1) produce no output and no gradient; ("transpose", l) -- hidden Linear l (0-based, square) is
    applied transposed; ("skip_bias", l) -- Linear l adds no bias."""
    q = bf16 if quant else (lambda t: t.double())
    x = q(x.double())
    kind = damage[0] if damage else None
    if kind == "k_chunk":
        x = x.clone(); x[:, damage[1]:damage[2]] = 0
    Ws = [q(W.double()) for W, _ in params]
    bs = [b.double() for _, b in params]
    if kind == "transpose":
        Ws[damage[1]] = Ws[damage[1]].t().contiguous()
    if kind == "skip_bias":
        bs[damage[1]] = torch.zeros_like(bs[damage[1]])
    L = len(params)
    acts, a = [], x
    for i in range(L):
        z = a @ Ws[i].t() + bs[i]
        if i < L - 1:
            a = q(torch.relu(z))
            acts.append(a)
    out = z
    if kind == "row_tile":
        out = out.clone(); out[damage[1]:damage[2]] = 0
    res = dict(out=out, acts=acts, loss=None, grads=None, dz=None)
    if loss == "mse":
        d = out - target.double()
        res["loss"] = (d * d).mean(); g = 2 * d / d.numel()
    elif loss == "ce":
        lo = out.reshape(-1, 2); t = target.reshape(-1).long()
        res["loss"] = nn.functional.cross_entropy(lo, t)
        g = ((torch.softmax(lo, 1) - nn.functional.one_hot(t, 2).double()) / lo.shape[0]).view_as(out)
    elif gout is not None:
        g = gout.double().view_as(out)
    else:
        return res
    dz = q(g)
    if kind == "row_tile":
        dz = dz.clone(); dz[damage[1]:damage[2]] = 0
    grads, dzs = [None] * L, [None] * L
    for i in range(L - 1, -1, -1):
        dzs[i] = dz
        a_in = acts[i - 1] if i > 0 else x
        grads[i] = (dz.t() @ a_in, dz.sum(0))
        if i > 0:
            dz = q((dz @ Ws[i]) * (acts[i - 1] > 0))
    res["grads"], res["dz"] = grads, dzs
    return res


# ---------------------------------------------------------------------------------------------------
# rounding-free data
# ---------------------------------------------------------------------------------------------------
def exact_case(in_channels, history, hidden, num_layers, out_channels, B, seed=SEED, gout_range=2):
    """dict(series [R, in / T] (fp64 integers), starts [B] (row 0 and the last valid row included), x [B, in] = the windows, column-major per column as
    get_helper_mlp flattens them, params [(W, b)], gout [B, out] = k 2^-14, y / gout_mse: fp32-exact MSE targets and the gradient the fused tail computes
    from them (tests/exact_data._mse_targets))."""
    g = torch.Generator().manual_seed(seed * 1000003 + in_channels * 31 + hidden * 7 + num_layers * 3 + out_channels + B * 101)
    T = history
    ncols = in_channels // T
    assert ncols * T == in_channels
    R = T if B == 1 else T + min(B, 40) + 3
    series = (torch.randint(1, 3, (R, ncols), generator=g) * (torch.randint(0, 2, (R, ncols), generator=g) * 2 - 1)).double()
    starts = torch.randint(0, R - T + 1, (B,), generator=g)
    starts[0] = 0
    starts[-1] = R - T
    idx = starts[:, None] + torch.arange(T)[None, :]                        # [B, T]
    x = series[idx].permute(0, 2, 1).reshape(B, in_channels).contiguous()     # [B, ncols, T] -> column-major rows
    H = hidden
    params = []
    for i, (of, kf) in enumerate(layer_dims(in_channels, hidden, out_channels, num_layers)):
        W = torch.zeros(of, kf, dtype=torch.float64)
        sign = (torch.randint(0, 2, (max(of, kf),), generator=g) * 2 - 1).double()
        if i == 0:
            perm = torch.randperm(kf, generator=g)
            W[perm % of, torch.arange(kf)] = sign[:kf]                      # every column meets one weight
        elif i < num_layers - 1:
            sign = torch.where(torch.randint(0, 4, (of,), generator=g) > 0, 1.0, -1.0).double()      # mostly +: deep stacks keep live units for dZ_1
            W[torch.arange(of), torch.randperm(kf, generator=g)] = sign           # a signed permutation
        else:
            W[torch.arange(kf) % of, torch.arange(kf)] = sign[:kf]          # output row j adds the units i = j mod out
        b = torch.randint(-1, 2, (of,), generator=g).double()
        params.append((W, b))
    gout = torch.randint(-gout_range, gout_range + 1, (B, out_channels), generator=g).double() * 2.0 ** GOUT_EXP
    case = dict(series=series, starts=starts, x=x, params=params, gout=gout, T=T, dims=(in_channels, hidden, out_channels, num_layers), B=B)
    out = reference(params, x)["out"]
    y, gm = _mse_targets(out, seed, gout_range)
    case["y"], case["gout_mse"] = y.view(B, out_channels), gm.view(B, out_channels)
    return case


def _fits_fp32(terms_abs_sum, grid):
    """sum of |terms| < 2^24 units of the finest grid of the terms"""
    return bool((terms_abs_sum / grid).max() < 2.0 ** 24)


def check_exact(case, gout_key="gout"):
    """Closure + coverage of one case, on the host.  Returns the fp64 reference for case[gout_key]."""
    params, x, gout = case["params"], case["x"], case[gout_key]
    ref = reference(params, x, gout=gout)
    em_q, em = emulate(params, x, gout=gout, quant=True), emulate(params, x, gout=gout, quant=False)
    # the emulation without rounding IS the reference, and rounding changes nothing: bit for bit
    for a, b, c in zip(_tensors(ref), _tensors(em), _tensors(em_q)):
        assert torch.equal(a, b), "quant=False differs from the fp64 reference"
        assert torch.equal(a, c), "a bf16 rounding point rounds on this data"
    # closure: every stored activation and activation gradient is a bf16 value
    assert is_bf16(x) and all(is_bf16(W) for W, _ in params)
    assert all(is_bf16(a) for a in em["acts"]) and all(is_bf16(d) for d in em["dz"]), "an activation or activation gradient is not a bf16 value"
    # every accumulation fits 2^24 units of its finest grid: forward sums are integers, backward sums multiples of 2^GOUT_EXP
    a_in = x
    for i, (W, b) in enumerate(params):
        assert _fits_fp32(a_in.abs() @ W.abs().t() + b.abs(), 1.0), f"forward sum of layer {i}"
        assert _fits_fp32(em["dz"][i].abs().t() @ a_in.abs(), 2.0 ** GOUT_EXP) and _fits_fp32(em["dz"][i].abs().sum(0), 2.0 ** GOUT_EXP), f"dW / db sum of layer {i}"
        if i > 0:
            assert _fits_fp32(em["dz"][i].abs() @ W.abs(), 2.0 ** GOUT_EXP), f"dA sum of layer {i}"
        if i < len(params) - 1:
            a_in = em["acts"][i]
    # coverage
    W1, dW1 = params[0][0], ref["grads"][0][0]
    assert bool((W1 != 0).any(0).all()), "an input column meets no weight"
    assert bool((dW1 != 0).any(0).all()), "an input column has no non-zero dW_1 entry"
    a_in = x
    for i, (W, b) in enumerate(params[:-1]):
        z = a_in @ W.t() + b
        assert bool((z == 0).any()), f"layer {i} has no exact-zero pre-activation"
        a = ref["acts"][i]
        for c in range(0, a.shape[1], 32):
            assert bool((a[:, c:c + 32] != 0).any()), f"hidden activation {i}, columns {c}..{c + 31} are all zero"
        a_in = a
    for i, (dW, db) in enumerate(ref["grads"]):
        assert bool((dW != 0).any()) and bool((db != 0).any()), f"a gradient tensor of layer {i} is zero"
    return ref


def _tensors(res):
    ts = [res["out"]] + list(res["acts"])
    for dW, db in res["grads"]:
        ts += [dW, db]
    return ts


def compare(ref, out, stash1, grads, what=""):
    """Bit-for-bit comparison of a result (out [B, out], stash1 [B, H] = relu(Z_1) as stored, grads [(dW, db)]) with a reference: the list of differing
    tensors' names (empty: equal)."""
    bad = []
    def eq(name, a, b):
        a, b = a.double().cpu(), b.double().cpu()
        if a.shape != b.shape or not torch.equal(a, b):
            bad.append(what + name)
    eq("out", out, ref["out"])
    if stash1 is not None:
        eq("stash1", stash1, ref["acts"][0])
    for i, ((dW, db), (rW, rb)) in enumerate(zip(grads, ref["grads"])):
        eq(f"dW{i}", dW, rW)
        eq(f"db{i}", db, rb)
    return bad


def damaged_variants(case):
    """The wrong results the checker must catch, as (name, emulate() result)."""
    in_channels, hidden, out_channels, L = case["dims"]
    B = case["B"]
    k0 = (in_channels // 2) // 8 * 8
    variants = [("k_chunk", ("k_chunk", k0, min(k0 + 32, in_channels))), ("row_tile", ("row_tile", 0, min(16, B))), ("skip_bias", ("skip_bias", 0))]
    if L > 2:
        variants.append(("transpose", ("transpose", 1)))
    else:
        variants.append(("skip_bias_out", ("skip_bias", L - 1)))
    return [(n, emulate(case["params"], case["x"], gout=case["gout"], quant=True, damage=d)) for n, d in variants]


def random_case(in_channels, hidden, out_channels, num_layers, B, seed=0):
    """Random data for the tolerance tests: torch's own nn.Linear initialisation, bf16-valued inputs of unit scale."""
    torch.manual_seed(seed)
    m = sequential(in_channels, hidden, out_channels, num_layers).double()
    params = [(mod.weight.detach(), mod.bias.detach()) for mod in m if isinstance(mod, nn.Linear)]
    g = torch.Generator().manual_seed(seed + 1)
    x = bf16(torch.randn(B, in_channels, generator=g, dtype=torch.float64))
    y = torch.randn(B, out_channels, generator=g, dtype=torch.float64).float().double()
    labels = torch.randint(0, 2, (B, out_channels // 2), generator=g, dtype=torch.int32)
    return dict(params=params, x=x, y=y, labels=labels)


def rel_max(a, b):
    return float((a.double().cpu() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


def rel_l2(a, b):
    return float((a.double().cpu() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


# ---------------------------------------------------------------------------------------------------
# the fused cross-entropy tail: cases on which the softmax gradient itself is exact (tests/exact_data.ce_case's construction)
# ---------------------------------------------------------------------------------------------------
CE_MATRIX = [      # (row of EXACT_MATRIX, B, seed, wrong share, ties): rows whose number of logit pairs is a power of two, at power-of-two batches
    ((35, 7, 128, 3, 4), 16, 2, 0.5, True),
    ((35, 7, 128, 3, 4), 1024, 1, 0.5, True),
    ((450, 150, 128, 3, 4), 16, 2, 0.5, False),      # (the first seed that closes; it has no ties)
    ((450, 150, 128, 3, 4), 1024, 1, 0.5, True),
    ((450, 150, 384, 3, 8), 16, 1, 0.5, True),
    ((450, 150, 384, 3, 8), 1024, 1, 0.5, True),
    ((1200, 8, 256, 8, 8), 16, 1, 0.5, False),
    ((1200, 8, 256, 8, 8), 1024, 2, 0.5, False),
    ((8100, 150, 128, 8, 8), 16, 1, 0.5, False),
    ((8100, 150, 128, 8, 8), 1024, 1, 0.5, True),
    ((8100, 150, 512, 2, 4), 16, 1, 0.5, False),
    ((8100, 150, 512, 2, 4), 1024, 2, 0.5, False),
]
CE_LEFT_OUT = {}      # (row, B): the condition no seed of 1..12 meets -- none: every row of EXACT_MATRIX with 2 or 4 logit pairs closes at seed 1 or 2


def ce_case(shape, B, seed, wrong_share=0.5):
    """`exact_case` with the last layer times 2^CE_SHIFT, labels [B, out / 2] and gout_ce, the gradient the loss tail of k_mlp_stack computes in fp32
    (inv = fl32(1 / (B out / 2)), csrc/mshgnn_mlp.hip) where every logit pair is a tie or saturated (asserted), held to the fp64 softmax gradient within 2^-149
    per element; loss_ce the fp64 mean cross entropy, loss_terms its terms, counts per regime."""
    from tests import exact_data as xd
    case = exact_case(*shape, B, seed=seed)
    out_channels = shape[4]
    W, b = case["params"][-1]
    case["params"][-1] = (W * 2.0 ** xd.CE_SHIFT, b * 2.0 ** xd.CE_SHIFT)
    N = B * out_channels // 2
    logits = reference(case["params"], case["x"])["out"].reshape(N, 2)
    g = torch.Generator().manual_seed(seed * 7907 + 57)
    coin = torch.randint(0, 2, (N,), generator=g)
    wrong = torch.rand(N, generator=g, dtype=torch.float64) < wrong_share
    d = logits[:, 0] - logits[:, 1]
    larger = (d < 0).long()
    labels = torch.where(d == 0, coin, torch.where(wrong, 1 - larger, larger))
    gout = xd.ce_gout(logits, labels, np.float32(1.0) / np.float32(N))
    lg = logits.clone().requires_grad_(True)
    terms = nn.functional.cross_entropy(lg, labels, reduction="none")
    terms.mean().backward()
    err = float((lg.grad - gout).abs().max())
    assert err <= 2.0 ** -149, f"the fp32 softmax gradient is {err} from the fp64 one"
    tie, right, wr = xd.ce_regimes(logits, labels)
    case.update(labels=labels.to(torch.int32).view(B, out_channels // 2), gout_ce=gout.view(B, out_channels), loss_ce=float(terms.detach().mean()),
                loss_terms=terms.detach(), counts=dict(ties=int(tie.sum()), right=int(right.sum()), wrong=int(wr.sum())), ce_gout_err=err)
    del case["y"], case["gout_mse"]      # (the MSE targets belong to the unscaled last layer)
    return case


def check_exact_ce(case, ties):
    """`check_exact` for gout_ce, plus: the number of logit pairs is a power of two; every pair column sees both labels; right and wrong pairs each occur with
    both signs of l0 - l1; a case declared `ties` has a tie under each label, one declared without has none; from 32 rows on every regime occurs in the first
    and in the last 16-row tile; without ties the loss terms are multiples of 128 and their mean an fp32 value."""
    from tests import exact_data as xd
    B, pairs = case["labels"].shape
    N = B * pairs
    assert N & (N - 1) == 0, f"{N} logit pairs: not a power of two"
    ref = check_exact(case, "gout_ce")
    logits, labels = ref["out"].reshape(N, 2), case["labels"].reshape(-1).long()
    assert torch.equal(xd.ce_gout(logits, labels, np.float32(1.0) / np.float32(N)).view_as(case["gout_ce"]), case["gout_ce"])
    tie, right, wrong = xd.ce_regimes(logits, labels)
    pos = logits[:, 0] > logits[:, 1]
    for p in range(pairs):
        assert set(case["labels"][:, p].tolist()) == {0, 1}, f"logit pair {p} sees one label only"
    for name, reg in (("right", right), ("wrong", wrong)):
        assert bool((reg & pos).any()) and bool((reg & ~pos).any()), f"{name} pairs have one sign of l0 - l1 only"
    if ties:
        assert bool((tie & (labels == 0)).any()) and bool((tie & (labels == 1)).any()), "declared with ties: no tie under each label"
    else:
        assert not bool(tie.any()), "declared without ties, yet it has some"
        t = case["loss_terms"]
        assert bool((t == torch.round(t / 128.0) * 128.0).all()) and float(np.float32(case["loss_ce"])) == case["loss_ce"]
    if ties:      # the loss bound covers a tie's own roundings: (logf(2) + m) - m rounds at m's magnitude, logf within 2 ulps of log 2 (exact_data.check_exact_ce)
        u, t = 2.0 ** -24, case["loss_terms"]
        own = float(((logits[tie, 0].abs() + 1.0) * u + 2 * u).sum())
        assert own + (N - 1) * u / (1 - (N - 1) * u) * float(t.sum()) <= xd.ce_loss_bound(case) * float(t.sum()), "the ties' own roundings do not fit the loss bound"
    if B >= 32:
        for name, reg in (("tie", tie), ("right", right), ("wrong", wrong)):
            r = reg.view(B, pairs)
            if bool(reg.any()):
                assert bool(r[:16].any()) and bool(r[(B - 1) // 16 * 16:].any()), f"no {name} pair in the first or in the last tile"
    ref["loss"] = case["loss_ce"]
    return ref
