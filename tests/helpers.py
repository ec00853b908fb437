"""Shared helpers for the parity tests: rebuild a golden case (spec, inputs, weights) from its fixture."""
import json
import os

import numpy as np
import torch
import yaml

from morphsym_hgnn_amd import synth, topology
from morphsym_hgnn_amd.spec import ModelSpec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CFG = os.path.join(ROOT, "morphsym_hgnn_amd", "cfg")

# model cases only (the directory also holds the window-assembly fixture)
GOLDEN_CASES = sorted(f[:-4] for f in os.listdir(GOLDEN) if f.endswith(".npz") and not f.startswith("windows_"))


def load_group(name):
    if not name:
        return None, None
    path = os.path.join(CFG, name + ".yaml")
    with open(path) as f:
        return yaml.safe_load(f), path


def make_spec(kind, topo_name, cfg_name, hidden, layers, regression=True, grf=3):
    topo = topology.TOPOLOGIES[topo_name]()
    group, _ = load_group(cfg_name)
    widths = synth.feature_widths(kind, regression)
    return ModelSpec(kind=kind, topology=topo, hidden=hidden, num_layers=layers, widths=widths,
                     regression=regression, grf_dimension=grf, group=group)


NARROW_WIDTHS = {"base": 24, "joint": 9, "foot": 5}      # (MI inputs of 3 time steps: the host oracle stays cheap at any hidden width)


def make_limbs_spec(limbs, hidden, layers):
    """MI-HGNN (no symmetry group, one output per foot) on the synthetic robot of `limbs` three-joint limbs, at the reference's input widths: 1 base
    node, the destination of `limbs` hip-joint rows -- live, as a destination of layer 0, from 5 layers on."""
    return ModelSpec(kind="mi", topology=topology.synthetic_limbs(limbs), hidden=hidden, num_layers=layers, widths=synth.feature_widths("mi", True),
                     regression=True, grf_dimension=1)


def random_topology(seed, nb, nj, nf):
    """A topology no robot has: random edge lists over the five relation types of the MI graph -- repeated edges, nodes without in-edges, in-degrees up to
    the node count, one relation left empty (never the one into the decoder's type: a signal path stays)."""
    import random
    rng = random.Random(seed)
    n = {"base": nb, "joint": nj, "foot": nf}
    rels = []
    for k, (s_, d_) in enumerate((("base", "joint"), ("joint", "base"), ("joint", "joint"), ("foot", "joint"), ("joint", "foot"))):
        ne = 0 if (k == seed % 5 and k != 4) else rng.randint(1, 2 * max(n[s_], n[d_]))
        pairs = [[rng.randrange(n[s_]), rng.randrange(n[d_])] for _ in range(ne)]
        if pairs and rng.random() < 0.7:
            pairs.append(list(pairs[0]))                      # a repeated edge: PyG sums it twice
        rels.append(((s_, "connect", d_), pairs))
    return topology.RobotTopology(name=f"random{seed}", num_nodes=n, relations=rels)


def make_random_topology_spec(seed, nb, nj, nf, hidden, layers):
    """MI-HGNN over `random_topology`, narrow inputs (the model of tests/test_generic_gpu.py's test_random_topologies_match_the_oracle)."""
    return ModelSpec(kind="mi", topology=random_topology(seed, nb, nj, nf), hidden=hidden, num_layers=layers, widths=dict(NARROW_WIDTHS), regression=True,
                     grf_dimension=1, group=None, num_timesteps=3)


MEAN_DEGREE_EDGES = [[1, 0], [2, 0], [0, 1], [2, 1], [3, 1], [0, 1], [1, 2], [0, 3], [2, 3]]      # in-degrees 2, 4 (one edge repeated), 1, 2


def make_mean_degree_spec(layers, regression, hidden=128):
    """MiniCheetah-K4 with its base -> base 'gt' relation (mean aggregation) given in-degrees 2, 4, 1 and 2 (tests/test_generic_gpu.py's
    test_mean_aggregation_with_in_degree_above_one, its edge list changed to power-of-two degrees: 1 / in-degree is then exact).  The LDS-resident kernels
    reject such a relation; the generic-width engine takes it at every hidden width."""
    topo = topology.mini_cheetah_k4()
    rel = dict(topo.relations)
    assert ("base", "gt", "base") in rel
    rel[("base", "gt", "base")] = [list(e) for e in MEAN_DEGREE_EDGES]
    topo.relations = [(k, rel[k]) for k, _ in topo.relations]
    group, _ = load_group("mini_cheetah-k4")
    return ModelSpec(kind="k4", topology=topo, hidden=hidden, num_layers=layers, widths=synth.feature_widths("k4", regression), regression=regression,
                     grf_dimension=1, group=group)


def load_case(name):
    fx = np.load(os.path.join(GOLDEN, name + ".npz"))
    case = json.loads(str(fx["config"]))
    spec = make_spec(case["kind"], case["topo"], case["cfg"], case["hidden"], case["layers"],
                     case["regression"], case["grf"])
    seed = int(fx["seed"])
    B = case["B"]
    x_dict, y = synth.make_windows(seed, B, spec.num_nodes, spec.widths,
                                   spec.out_channels * spec.num_nodes[spec.out_type] if case["regression"] else 4,
                                   classification=not case["regression"])
    params = synth.make_params(seed, spec.param_shapes())
    ei = spec.topology.edge_index_dict(B)
    return case, spec, fx, x_dict, y, params, ei


def sample_indices(name, numel, k=64):
    u = synth.det_uniform(7, "idx:" + name, (k,), 0.0, 1.0).numpy()
    return np.minimum((u * numel).astype(np.int64), numel - 1)


def projection_signs(name, numel, k=4):
    """k deterministic +-1 vectors per tensor (numpy PCG64 seeded from the tensor name): fixture and check draw the same ones."""
    import zlib
    rng = np.random.Generator(np.random.PCG64(zlib.crc32(("proj:" + name).encode())))
    return rng.integers(0, 2, size=(k, numel)).astype(np.float64) * 2.0 - 1.0


def oracle_config(spec):
    from oracle import ms_hgnn_oracle as orc
    return orc.OracleConfig(kind=spec.kind, num_layers=spec.num_layers, edge_types=spec.edge_types,
                            regression=spec.regression, grf_dimension=spec.grf_dimension, group=spec.group,
                            num_timesteps=spec.num_timesteps)


SAMPLE_SLACK = 2.0      # sampled gradient entries: error <= SAMPLE_SLACK x rtol in units of the reference gradient's rms (and <= rtol in units of the largest sampled entry)


def check_against_fixture(fx, out, loss, grads, rtol, what=""):
    """Compare (out, loss, grads) with a golden fixture.  Tolerance is relative to each tensor's max-abs
    (outputs) / L2 norm (gradients)."""
    ref_out = torch.from_numpy(fx["out"])
    scale = float(ref_out.abs().max())
    err = float((out.double().cpu().reshape(ref_out.shape) - ref_out).abs().max()) / scale
    assert err <= rtol, f"{what} output rel err {err:.3e} > {rtol}"
    if loss is not None:
        lerr = abs(float(loss) - float(fx["loss"])) / abs(float(fx["loss"]))
        assert lerr <= rtol, f"{what} loss rel err {lerr:.3e} > {rtol}"
    worst = (0.0, None)
    for key in fx.files:
        if not key.startswith("gnorm:"):
            continue
        name = key[len("gnorm:"):]
        g = grads[name].double().cpu().flatten().numpy()
        gn = float(fx[key])
        idx = sample_indices(name, g.size)
        denom = max(gn / np.sqrt(g.size), 1e-30)  # rms magnitude of the reference gradient
        if gn == 0.0:
            assert np.abs(g).max() == 0.0, f"{what} grad {name} should be exactly zero"
            continue
        e1 = float(np.abs(g[idx] - fx["gsample:" + name]).max()) / denom
        e2 = abs(float(np.sqrt((g ** 2).sum())) - gn) / gn
        # samples: a single entry's error in units of the tensor's rms is allowed SAMPLE_SLACK x the tolerance (an L2-relative bound of rtol would allow
        # sqrt(N) x; rounds 1-5 allowed 30 x without knowing what the plans use: measured over every golden case, tools/sample_tolerance_probe.py, the worst
        # sampled entry sits at 0.76 x rtol on the fp32 plan and 0.92 x on the split plan, 0.34 x in units of the largest sampled reference entry)
        e = max(e1 / SAMPLE_SLACK, e2)
        if e > worst[0]:
            worst = (e, name)
        assert e2 <= rtol, f"{what} grad-norm {name} rel err {e2:.3e} > {rtol}"
        # sum of all entries (|sum of errors| <= sqrt(N) * L2 error) and, when the fixture has them, four +-1 random projections:
        # a localized error that the 64 samples miss still moves these
        e3 = abs(float(g.sum()) - float(fx["gsum:" + name])) / (gn * np.sqrt(g.size))
        assert e3 <= rtol, f"{what} grad-sum {name} err {e3:.3e} > {rtol}"
        if "gproj:" + name in fx.files:
            e4 = float(np.abs(projection_signs(name, g.size) @ g - fx["gproj:" + name]).max()) / gn
            assert e4 <= 4 * rtol, f"{what} grad-projection {name} err {e4:.3e} > {4 * rtol}"
        assert e1 <= SAMPLE_SLACK * rtol, f"{what} grad samples {name} err/rms {e1:.3e} > {SAMPLE_SLACK * rtol}"
        e5 = float(np.abs(g[idx] - fx["gsample:" + name]).max()) / max(float(np.abs(fx["gsample:" + name]).max()), 1e-30)
        assert e5 <= rtol, f"{what} grad samples {name} err / largest sampled reference entry {e5:.3e} > {rtol}"
    return err, worst


# ---------------------------------------------------------------------------------------------------
# GPU parity harness (used by tests/test_engine_gpu.py, tools and __graft_entry__.smoke)
# ---------------------------------------------------------------------------------------------------
def dense_hidden(spec, hidden_dict, B):
    """oracle hidden dict {type: [B*n_t, h]} -> [B, NN, h] in the engine's node order."""
    parts = [hidden_dict[t].view(B, spec.num_nodes[t], -1) for t in spec.node_types]
    return torch.cat(parts, dim=1)


def node_slices(spec):
    out, o = {}, 0
    for t in spec.node_types:
        out[t] = slice(o, o + spec.num_nodes[t])
        o += spec.num_nodes[t]
    return out


def engine_relu_decisions(e, spec, B):
    """The relu decisions the engine took in its last training forward of batch size B, read back from its workspace:
    {("enc", type) | ("layer", l, type): bool [B*n_type, hidden]} from the relu bytes (one byte per (node, window, 8 features):
    [NN][hidden/32 column slices][ceil(B/16) tiles][4 groups][16 windows], bit j <-> feature 32 slice + 8 group + j) and
    {("t1", l): bool [B*n_base, hidden]} from the stashed base_transform activation T1 (its backward masks with T1 > 0)."""
    lay, ws = e.layout(B, True), e.workspace(B, True)
    # (a PaddedEngine's workspace holds the inner model's rows: read them at the padded width, hand back the true width's columns)
    nn_, h, tiles = e.info.total_nodes, (e.inner_spec.hidden if getattr(e, "padded", False) else spec.hidden), (B + 15) // 16
    ht = spec.hidden
    sl = node_slices(spec)

    def from_bytes(off):
        ns = h // 32                                                                    # column slices of 32 features
        raw = ws[off:off + nn_ * ns * tiles * 64].view(nn_, ns, tiles, 4, 16).cpu()
        bits = (raw.unsqueeze(-1) >> torch.arange(8, dtype=torch.uint8)) & 1            # [NN, slice, tile, group, win, bit]
        return bits.permute(2, 4, 0, 1, 3, 5).reshape(tiles * 16, nn_, h)[:B, :, :ht].bool()  # [B, NN, hidden]

    out = {}
    # (a node the plan does not compute -- spec.node_liveness -- has no decision: its rows of the relu bytes are unwritten memory; run_engine_case
    #  gives the oracle the exact decision there, row_live_mask says which rows are real)
    m0 = from_bytes(lay.dd[0])
    for t in spec.node_types:
        out[("enc", t)] = m0[:, sl[t]].reshape(-1, ht)
    for l in range(spec.num_layers):
        ml = from_bytes(lay.mask[l])
        for t in spec.live_types(l):
            if not (spec.has_base_transform and t == "base"):
                out[("layer", l, t)] = ml[:, sl[t]].reshape(-1, ht)
        if spec.has_base_transform and spec.node_liveness()[0][l]["base"]:
            nb = spec.num_nodes["base"]
            n = nb * B * h
            if e.storage == "x3":
                t1 = ws[lay.t1[l]:lay.t1[l] + 4 * n].view(torch.bfloat16).view(nb, B, 2, h)[:, :, 0]      # rows of [hi | lo]: hi carries the sign
            else:
                t1 = ws[lay.t1[l]:lay.t1[l] + n * (4 if e.storage == "f32" else 2)].view(torch.float32 if e.storage == "f32" else torch.bfloat16).view(nb, B, h)
            out[("t1", l)] = (t1[..., :ht].permute(1, 0, 2).reshape(-1, ht).float() > 0).cpu()
    return out


def check_input_grad_against_own_operands(e, spec, params, B, got):
    """Engine.input_grad's output `got` ({type: [B * n_t, pitch]}, fp32 or fp64) against dx = m . (dY_enc @ W_enc) rebuilt in fp64 from the engine's
    OWN operands: the dX_0 stash read straight from the workspace (split plan: its hi and lo halves; bf16 plan: the bf16 rows; fp32 plan: the fp32
    rows) and W_enc in the plan's operand form (bf16: round to nearest even; split: hi + lo with exactly the kernel's products hi.hi, hi.lo, lo.hi;
    fp32: as is).  Each element must lie within 2 n 2^-24 sum |terms| of it, n the products summed: K on the fp32 and bf16 plans, 3K on the split plan
    (three products per k -- the recursive-summation count; a bound of 2 K 2^-24 there would assume fewer roundings than the kernel performs).  That
    leaves the accumulation order as the only freedom; rows of nodes the plan does not compute and columns past F_t must be exact zeros.  Returns the largest error in units of that bound."""
    lay, ws = e.layout(B, True), e.workspace(B, True)
    nn_ = e.info.total_nodes
    K = e.inner_spec.hidden if getattr(e, "padded", False) else spec.hidden
    off, n = lay.dx[0], nn_ * B * K
    if e.storage == "x3":
        st = ws[off:off + 4 * n].view(torch.bfloat16).view(nn_, B, 2, K)
        parts = [(st[:, :, 0], "hi"), (st[:, :, 1], "lo")]
    elif e.storage == "bf16":
        parts = [(ws[off:off + 2 * n].view(torch.bfloat16).view(nn_, B, K), "hi")]
    else:
        parts = [(ws[off:off + 4 * n].view(torch.float32).view(nn_, B, K), "hi")]
    _, need = spec.node_liveness()
    masks = spec.input_masks()
    sl = node_slices(spec)
    worst = 0.0
    for t in spec.node_types:
        F = spec.widths[t]
        w32 = torch.zeros(K, F, dtype=torch.float32, device=e.device)
        w32[:spec.hidden] = params[f"encoder.lins.{t}.weight"].to(e.device, torch.float32)
        if e.storage == "f32":
            wp = {"hi": w32.double()}
        else:
            wh = w32.to(torch.bfloat16)
            wp = {"hi": wh.double(), "lo": (w32 - wh.float()).to(torch.bfloat16).double()}
        prods = [("hi", "hi"), ("lo", "hi"), ("hi", "lo")] if e.storage == "x3" else [("hi", "hi")]
        n_terms = K * len(prods)
        g = got[t].view(B, spec.num_nodes[t], -1)
        assert g.shape[-1] >= F
        assert torch.count_nonzero(g[..., F:]) == 0 and not bool(torch.signbit(g[..., F:]).any()), f"{t}: pad columns are not +0.0"
        for i in range(spec.num_nodes[t]):
            gi = g[:, i, :F].double()
            if i not in need[0][t]:
                assert torch.count_nonzero(gi) == 0, f"{t} node {i}: the plan does not compute this node, yet its dx is non-zero"
                continue
            dy = {name: p[sl[t].start + i].double() for p, name in parts}      # [B, K]
            ref = sum(dy[a] @ wp[b] for a, b in prods)
            bound = sum(dy[a].abs() @ wp[b].abs() for a, b in prods)
            m = masks[t][i].to(e.device)
            err = (gi - ref * m).abs()
            lim = 2.0 * n_terms * 2.0 ** -24 * bound
            bad = err > lim
            assert not bool(bad.any()), (f"{t} node {i}: {int(bad.sum())} elements outside 2 n 2^-24 sum|terms|; first at "
                                         f"{bad.nonzero()[0].tolist()}: got {float(gi[bad][0])!r}, reference {float((ref * m)[bad][0])!r}")
            nz = bound > 0
            if bool(nz.any()):
                worst = max(worst, float((err[nz] / lim[nz]).max()))
    return worst


def row_live_mask(spec, key, B):
    """bool [B * n_type] for a decision key of engine_relu_decisions: True where the engine really took that decision (the node is computed by the plan)."""
    live, need = spec.node_liveness()
    if key[0] == "enc":
        t, nodes = key[1], need[0][key[1]]
    elif key[0] == "layer":
        t, nodes = key[2], live[key[1]][key[2]]
    else:      # ("t1", l): the base_transform nodes of layer l
        t, nodes = "base", live[key[1]]["base"]
    m = torch.zeros(spec.num_nodes[t], dtype=torch.bool)
    m[list(nodes)] = True
    return m.repeat(B)


def run_engine_case(spec, x_dict, y, params, ei, B, dtype="f32", device="cuda:0", decision_tol=1e-4, engine=None):
    """Run fwd + MSE/CE + bwd through the C-ABI and through the oracle; return dict of relative errors
    (max-abs error / max-abs reference) per stage, plus the raw engine results.

    The oracle is evaluated WITH THE ENGINE'S relu decisions: a pre-activation within rounding error of zero may land on the other
    side in finite precision, and the gradient is discontinuous there (one flipped decision moves a tiny-batch weight gradient by
    1e-3..1e-2 of its scale on ANY plan, fp32 included).  Every decision that differs from the exact one must belong to a
    pre-activation within `decision_tol` x (max-abs of its tensor) of zero -- counted in errs["relu_decisions_outside_tolerance"],
    which must be 0 -- and given the same decisions every hidden state, the output, the loss and every gradient must match.
    engine: run on this engine (e.g. an `engine.make_engine` PaddedEngine) instead of a fresh `Engine(spec, dtype, device)`."""
    from morphsym_hgnn_amd import engine as eng
    from oracle import ms_hgnn_oracle as orc
    cfg = oracle_config(spec)
    e = engine or eng.Engine(spec, dtype=dtype, device=device)
    xs = e.cast_inputs(x_dict)
    flat = eng.flatten_params(spec, params, device=e.device)
    out = e.forward(xs, flat, B, training=True)
    torch.cuda.synchronize()
    decisions = engine_relu_decisions(e, spec, B)
    stats = {"differ": 0, "outside": 0}

    def relu_fn(key, h):
        if key not in decisions:
            return torch.relu(h)
        rows = row_live_mask(spec, key, B).view(-1, 1)
        m = torch.where(rows, decisions[key], h.detach() > 0)      # nodes the plan does not compute: the exact decision (they cannot reach the output)
        diff = m != (h.detach() > 0)
        if bool(diff.any()):
            stats["differ"] += int(diff.sum())
            stats["outside"] += int((h.detach().abs()[diff] > decision_tol * float(h.detach().abs().max())).sum())
        return h * m.to(h.dtype)

    # oracle (fp64, CPU)
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in params.items()}
    o_out, o_hidden = orc.forward(cfg, leaves, {k: v.clone() for k, v in x_dict.items()}, ei, return_hidden=True, relu_fn=relu_fn)
    yy, yp = orc.wrapper_outputs(cfg, o_out, y, B)
    o_loss = orc.mse_loss(yy, yp) if spec.regression else orc.cross_entropy_loss(yy, yp, B)
    gout_ref = torch.autograd.grad(o_loss, o_out, retain_graph=True)[0]
    o_loss.backward()
    o_grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()}
    errs = {"relu_decisions_outside_tolerance": float(stats["outside"])}

    def rel(a, b):
        a = a.detach().double().cpu(); b = b.detach().double().cpu()
        return float((a - b).abs().max() / max(float(b.abs().max()), 1e-300))

    sl = node_slices(spec)
    for l in range(spec.num_layers + 1):
        got = e.hidden_state(B, l)
        ref = dense_hidden(spec, o_hidden[l], B)
        liv, need = spec.node_liveness()
        nodes = need[0] if l == 0 else liv[l - 1]      # the nodes of X_l the plan computes
        for t in spec.node_types:
            if nodes[t]:
                idx = torch.tensor(nodes[t]) + sl[t].start
                errs[f"X{l}[{t}]"] = rel(got[:, idx], ref[:, idx])
    errs["out"] = rel(out.view(-1), o_out.detach().reshape(-1))
    # loss + grad seed: regression uses the engine's fused MSE, classification seeds from the oracle's CE grad
    if spec.regression:
        yd = yy.reshape(-1).to(e.device, torch.float32)
        loss, gout = e.mse_loss(out.view(-1), yd)
        errs["loss"] = rel(loss, o_loss.reshape(1))
        errs["grad_out"] = rel(gout, gout_ref.reshape(-1))
    else:
        loss = None
        gout = gout_ref.reshape(-1).to(e.device, torch.float32)
    gflat = e.backward(xs, flat, gout.contiguous(), B)
    torch.cuda.synchronize()
    grads = {k: v.detach().cpu() for k, v in eng.unflatten(spec, gflat).items()}
    for k, g in o_grads.items():
        ref_max = float(g.abs().max())
        if ref_max == 0.0:
            errs["grad:" + k] = float(grads[k].abs().max())   # must be exactly zero
        else:
            errs["grad:" + k] = rel(grads[k], g)
    run_engine_case.last_decisions_differing = stats["differ"]
    run_engine_case.last_reference = {"out": o_out.detach(), "loss": o_loss.detach(), "grads": o_grads}      # (the oracle's results under those decisions)
    return errs, out.detach().cpu(), (loss.detach().cpu() if loss is not None else o_loss.detach()), grads


def random_case(spec, B, seed):
    """Seeded random minibatch + weights at any size (torch.Generator: synth.make_windows' hash-based draws take ~3 ms per window): x_dict in the
    reference's convention (fp64, [B * n_t, F_t]), y ([B, n_out * d] regression targets or {0, 1} contact flags), params (synth.make_params)."""
    g = torch.Generator().manual_seed(seed)
    x_dict = {t: torch.randn(B * spec.num_nodes[t], spec.widths[t], generator=g, dtype=torch.float64) for t in spec.node_types}
    n_out = spec.num_nodes[spec.out_type]
    if spec.regression:
        y = torch.randn(B, n_out * spec.out_channels, generator=g, dtype=torch.float64)
    else:
        y = (torch.rand(B, n_out, generator=g) > 0.5).to(torch.float64)
    return x_dict, y, synth.make_params(seed, spec.param_shapes())


def run_step_case(spec, x_dict, y, params, B, dtype="x3", device="cuda:0", decision_tol=1e-4, engine=None):
    """The ONE-CALL training step (mshgnn_step_mse / mshgnn_step_ce: the entry points bench.py times) against the fp64 oracle evaluated with the engine's
    own relu decisions (see run_engine_case) -- usable at BASELINE's full batch sizes: the oracle does ~1 000-7 000 windows/s on the host.
    Returns (errs, out, loss, grads): errs = max-abs error / max-abs reference per stage (hidden states the plan computes, output, loss, every gradient;
    exact-zero reference gradients must be exactly zero) + the number of relu decisions that differ OUTSIDE the tolerance band (must be 0)."""
    from morphsym_hgnn_amd import engine as eng
    from oracle import ms_hgnn_oracle as orc
    cfg = oracle_config(spec)
    e = engine or eng.Engine(spec, dtype=dtype, device=device)
    xs = e.cast_inputs(x_dict)
    flat = eng.flatten_params(spec, params, device=e.device)
    n_out = spec.num_nodes[spec.out_type]
    if spec.regression:
        out, loss, gflat = e.step_mse(xs, flat, y.reshape(-1).to(e.device, torch.float32), B)
    else:
        out, loss, gflat = e.step_ce(xs, flat, y.reshape(B, n_out).to(e.device, torch.int32).contiguous(), B)
    torch.cuda.synchronize()
    decisions = engine_relu_decisions(e, spec, B)
    stats = {"differ": 0, "outside": 0, "total": 0}

    def relu_fn(key, h):
        if key not in decisions:
            return torch.relu(h)
        rows = row_live_mask(spec, key, B).view(-1, 1)
        exact = h.detach() > 0
        m = torch.where(rows, decisions[key], exact)
        diff = m != exact
        stats["total"] += int(rows.sum()) * h.shape[-1]      # decisions the engine really took (nodes its plan computes)
        if bool(diff.any()):
            stats["differ"] += int(diff.sum())
            stats["outside"] += int((h.detach().abs()[diff] > decision_tol * float(h.detach().abs().max())).sum())
        return h * m.to(h.dtype)

    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in params.items()}
    ei = spec.topology.edge_index_dict(B)
    o_out, o_hidden = orc.forward(cfg, leaves, {k: v.clone() for k, v in x_dict.items()}, ei, return_hidden=True, relu_fn=relu_fn)
    yy, yp = orc.wrapper_outputs(cfg, o_out, y, B)
    o_loss = orc.mse_loss(yy, yp) if spec.regression else orc.cross_entropy_loss(yy, yp, B)
    o_loss.backward()
    errs = {"relu_decisions_outside_tolerance": float(stats["outside"])}

    def rel(a, b):
        a = a.detach().double().cpu(); b = b.detach().double().cpu()
        return float((a - b).abs().max() / max(float(b.abs().max()), 1e-300))

    sl = node_slices(spec)
    liv, need = spec.node_liveness()
    for l in range(spec.num_layers):      # (X_L is not stashed by a one-launch step: nobody reads it -- the output and the decoder's gradients cover it)
        got = e.hidden_state(B, l)
        ref = dense_hidden(spec, o_hidden[l], B)
        nodes = need[0] if l == 0 else liv[l - 1]
        for t in spec.node_types:
            if nodes[t]:
                idx = torch.tensor(nodes[t]) + sl[t].start
                errs[f"X{l}[{t}]"] = rel(got[:, idx], ref[:, idx])
    errs["out"] = rel(out.reshape(-1), o_out.detach().reshape(-1))
    errs["loss"] = rel(loss.reshape(1), o_loss.reshape(1))
    grads = {k: v.detach().cpu() for k, v in eng.unflatten(spec, gflat).items()}
    for k, v in leaves.items():
        g = v.grad if v.grad is not None else torch.zeros_like(v)
        ref_max = float(g.abs().max())
        errs["grad:" + k] = float(grads[k].abs().max()) if ref_max == 0.0 else rel(grads[k], g)
    run_step_case.last_decisions_differing = stats["differ"]
    run_step_case.last_reference = {"out": o_out.detach(), "loss": o_loss.detach(),
                                    "grads": {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()}}
    run_step_case.last_decisions_total = stats["total"]
    return errs, out.detach().cpu(), loss.detach().cpu(), grads
