"""GPU parity tests (-m gpu) of the stand-alone operator surface: `morphsym_hgnn_amd.nn.{Linear, HeteroDictLinear, GraphConv,
HeteroConv}` called on their own (HIP operators of csrc/mshgnn_ops.hip through the C-ABI) against the oracle's restatement of the
torch_geometric==2.5.0 operators (oracle/pyg_restated, the module the reference's own model files were imported over when the golden
vectors were generated) in fp64 on the CPU: outputs and every gradient within 1e-4 relative (BASELINE.json north_star tolerance;
fp32 accumulation stays around 1e-6) -- and, since that metric is normalised by the tensor's largest entry, additionally ELEMENT BY ELEMENT: the inputs
and parameters of the single-operator tests are fp32 values (drawn in fp32, upcast to fp64 for both sides), so every output and gradient element must lie
within the derived bound gamma_n sum |terms| of tests/ops_reference.py, n the roundings on that element's own path."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-4


def _ref_nn():
    sys.path.insert(0, os.path.join(ROOT, "oracle", "pyg_restated"))
    try:
        import torch_geometric.nn as ref
    finally:
        sys.path.pop(0)
    return ref


def _rel(a, b):
    return float((a.detach().double().cpu() - b.detach().double()).abs().max() / b.detach().double().abs().max().clamp(min=1e-30))


def _fp32_values(*mods_or_tensors):
    """Round parameters / tensors (fp64) to fp32 values in place: both sides then start from the same fp32 operands."""
    with torch.no_grad():
        for m in mods_or_tensors:
            for p in (m.parameters() if isinstance(m, torch.nn.Module) else [m]):
                p.copy_(p.float().double())


def _splits(M, N, K):
    import ctypes as C
    from morphsym_hgnn_amd import engine as eng
    s = C.c_int32(0)
    eng.load_library().mshgnn_op_gemm_workspace(M, N, K, C.byref(s))
    return s.value


def _bounded(got, ref, bound, what):
    from tests import ops_reference as opr
    d = opr.within_bound(got, ref.detach().double(), bound)
    assert d is None, f"{what}: {d}"


def _check_linear_bounds(x, W, b, g, y, yr, gx, gxr, gw, gwr, gb, gbr):
    """y = x W^T + b: n = K + splits + 1; dx = g W: n = N + splits; dW = g^T x: n = M + splits; db: n = M (x [M, K], W [N, K], g [M, N], fp64 tensors
    holding fp32 values)."""
    from tests import ops_reference as opr
    (M, K), N = x.shape, W.shape[0]
    _bounded(y, yr, opr.elementwise_bound(x, W, K + _splits(M, N, K) + 1, b), "y")
    _bounded(gx, gxr, opr.elementwise_bound(g, W.t(), N + _splits(M, K, N)), "dx")
    _bounded(gw, gwr, opr.elementwise_bound(g.t(), x.t(), M + _splits(N, K, M)), "dW")
    _bounded(gb, gbr, opr.gamma(M) * g.abs().sum(0), "db")


def _check_graph_conv_bounds(mean, xs, xd, Wr, b, Wo, ei, g, y, yr, grads, grads_ref):
    """The bounds of one GraphConv (fp64 tensors holding fp32 values).  The aggregate carries deg + 2 roundings per element ('mean': fl32(1 / deg) and the
    scale product; counted for 'add' too), so everything computed from it is bounded with the aggregate of |x_src| in its place and those roundings added
    to n: gamma_a + gamma_b + gamma_a gamma_b <= gamma_(a + b).  grads: (dx_src, dx_dst, dW_rel, db, dW_root)."""
    from tests import ops_reference as opr
    src, dst = ei[0], ei[1]
    n_src, n_dst, in_s, in_d, O = xs.shape[0], xd.shape[0], xs.shape[1], xd.shape[1], Wr.shape[0]
    deg = torch.bincount(dst, minlength=n_dst)
    w = (1.0 / deg.clamp(min=1).double())[dst] if mean else torch.ones(dst.numel(), dtype=torch.float64)
    agg_abs = torch.zeros(n_dst, in_s, dtype=torch.float64).index_add(0, dst, xs.abs()[src] * w[:, None])
    n_agg = deg + 2
    _bounded(y, yr, opr.elementwise_bound(agg_abs, Wr, (n_agg + in_s + in_d + 4)[:, None], b, xd.abs() @ Wo.abs().t()), "out")
    _bounded(grads[1], grads_ref[1], opr.elementwise_bound(g, Wo.t(), O + 1), "dx_dst")
    _bounded(grads[2], grads_ref[2], opr.elementwise_bound(g.t(), agg_abs.t(), n_dst + _splits(O, in_s, n_dst) + int(n_agg.max())), "dW_rel")
    _bounded(grads[3], grads_ref[3], opr.gamma(max(n_dst, 1)) * g.abs().sum(0), "db")
    _bounded(grads[4], grads_ref[4], opr.elementwise_bound(g.t(), xd.t(), n_dst + _splits(O, in_d, n_dst)), "dW_root")
    out_deg = torch.bincount(src, minlength=n_src)
    dagg_abs = g.abs() @ Wr.abs()
    back = torch.zeros(n_src, in_s, dtype=torch.float64).index_add(0, src, dagg_abs[dst] * w[:, None])
    _bounded(grads[0], grads_ref[0], opr.gamma(out_deg + O + 3)[:, None] * back, "dx_src")


def _copy_params(dst, src):
    with torch.no_grad():
        for (kd, pd), (ks, ps) in zip(sorted(dst.named_parameters()), sorted(src.named_parameters())):
            assert kd == ks, (kd, ks)
            pd.copy_(ps)


def _require_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (there is no CPU fallback to fall through to)")


@pytest.mark.parametrize("M,K,N", [(1, 7, 5), (50, 450, 128), (3000, 900, 128), (257, 128, 3), (70000, 128, 128)])
def test_linear_matches_reference(M, K, N):
    _require_gpu()
    from morphsym_hgnn_amd import nn as pnn
    ref = _ref_nn()
    torch.manual_seed(M + K)
    r = ref.Linear(K, N).double()
    m = pnn.Linear(-1, N).double()
    x = torch.randn(M, K, dtype=torch.float32).double()      # fp32 values on both sides
    _fp32_values(r)
    xr = x.clone().requires_grad_(True)
    xg = x.cuda().requires_grad_(True)
    m.cuda()
    y = m(xg)                      # lazy weight materialises here
    assert tuple(m.weight.shape) == (N, K) and y.dtype == torch.float64
    _copy_params(m, r)
    y = m(xg)
    yr = r(xr)
    g = torch.randn(M, N, dtype=torch.float32).double()
    y.backward(g.cuda()); yr.backward(g)
    assert _rel(y, yr) < RTOL
    assert _rel(xg.grad, xr.grad) < RTOL and _rel(m.weight.grad, r.weight.grad) < RTOL and _rel(m.bias.grad, r.bias.grad) < RTOL
    _check_linear_bounds(x, r.weight.detach(), r.bias.detach(), g, y, yr, xg.grad, xr.grad, m.weight.grad, r.weight.grad, m.bias.grad, r.bias.grad)


@pytest.mark.parametrize("aggr", ["add", "mean"])
@pytest.mark.parametrize("n_src,n_dst,E,H,O", [(12, 4, 4, 128, 128), (300, 170, 2000, 96, 40), (5, 9, 0, 16, 8), (40000, 40000, 120000, 128, 128)])
def test_graph_conv_matches_reference(aggr, n_src, n_dst, E, H, O):
    """Bipartite GraphConv on random multigraphs (repeated edges, isolated destinations, an empty edge set), 'add' and 'mean'."""
    _require_gpu()
    from morphsym_hgnn_amd import nn as pnn
    ref = _ref_nn()
    g = torch.Generator().manual_seed(E + n_src)
    r = ref.GraphConv((H, H), O, aggr=aggr).double()
    m = pnn.GraphConv((H, H), O, aggr=aggr).double().cuda()
    _fp32_values(r)
    _copy_params(m, r)
    xs, xd = torch.randn(n_src, H, dtype=torch.float64, generator=g), torch.randn(n_dst, H, dtype=torch.float64, generator=g)
    _fp32_values(xs, xd)
    ei = torch.stack([torch.randint(0, n_src, (E,), generator=g), torch.randint(0, max(1, n_dst - 1), (E,), generator=g)])     # the last destination has no in-edge
    a = [t.clone().requires_grad_(True) for t in (xs, xd)]
    b = [t.cuda().requires_grad_(True) for t in (xs, xd)]
    yr = r((a[0], a[1]), ei)
    y = m((b[0], b[1]), ei.cuda())
    go = torch.randn(n_dst, O, dtype=torch.float64, generator=g)
    _fp32_values(go)
    yr.backward(go); y.backward(go.cuda())
    assert _rel(y, yr) < RTOL
    names = ("lin_rel.weight", "lin_rel.bias", "lin_root.weight")
    _check_graph_conv_bounds(aggr == "mean", xs, xd, r.lin_rel.weight.detach(), r.lin_rel.bias.detach(), r.lin_root.weight.detach(), ei, go, y, yr,
                             (b[0].grad, b[1].grad) + tuple(m.get_parameter(k).grad for k in names),
                             (a[0].grad, a[1].grad) + tuple(r.get_parameter(k).grad for k in names))
    if E:
        assert _rel(b[0].grad, a[0].grad) < RTOL
        assert _rel(m.lin_rel.weight.grad, r.lin_rel.weight.grad) < RTOL
    else:
        assert float(b[0].grad.abs().max()) == 0.0 and float(m.lin_rel.weight.grad.abs().max()) == 0.0
    assert _rel(b[1].grad, a[1].grad) < RTOL
    assert _rel(m.lin_rel.bias.grad, r.lin_rel.bias.grad) < RTOL and _rel(m.lin_root.weight.grad, r.lin_root.weight.grad) < RTOL


def test_hetero_stack_matches_reference_on_the_a1_graph():
    """The reference's own layer stack (hgnn_c2.py:88-113,143-166 without the symmetry masks) assembled from the four operator modules on
    a PyG-batched A1-C2 graph: HeteroDictLinear -> relu -> 2 x HeteroConv{GraphConv} -> relu, forward and every parameter gradient."""
    _require_gpu()
    from morphsym_hgnn_amd import nn as pnn
    from morphsym_hgnn_amd import synth
    from tests import helpers
    ref = _ref_nn()
    spec = helpers.make_spec("c2", "a1-c2", "a1-c2", 128, 2)
    B, H = 5, 64
    x_dict, _ = synth.make_windows(21, B, spec.num_nodes, spec.widths, 12)
    x_dict = {k: v.double() for k, v in x_dict.items()}
    ei = spec.topology.edge_index_dict(B)
    types, rels = spec.topology.metadata()

    def build(nnmod):
        torch.manual_seed(3)
        enc = nnmod.HeteroDictLinear(-1, H, types)
        convs = torch.nn.ModuleList([nnmod.HeteroConv({tuple(r): nnmod.GraphConv(H, H, aggr="mean" if r[1] in ("gt", "gs") else "add") for r in rels}, aggr="sum")
                                     for _ in range(2)])
        return torch.nn.ModuleList([enc, convs]).double()

    def run(net, xd, eid):
        h = {k: v.relu() for k, v in net[0](xd).items()}
        for conv in net[1]:
            h = {k: v.relu() for k, v in conv(h, eid).items()}
        return h

    r = build(ref)
    m = build(pnn)
    hr = run(r, x_dict, ei)                                   # materialises the reference's lazy encoder
    m.cuda()
    xg = {k: v.cuda() for k, v in x_dict.items()}
    eg = {k: v.cuda() for k, v in ei.items()}
    run(m, xg, eg)                                            # ... and ours
    _copy_params(m, r)
    hm = run(m, xg, eg)
    assert set(hm) == set(hr)
    lr = sum((v ** 2).sum() for v in hr.values())
    lm = sum((v ** 2).sum() for v in hm.values())
    lr.backward(); lm.backward()
    for k in hr:
        assert _rel(hm[k], hr[k]) < RTOL, k
    for (kd, pd), (ks, ps) in zip(sorted(m.named_parameters()), sorted(r.named_parameters())):
        if ps.grad is None:
            assert pd.grad is None or float(pd.grad.abs().max()) == 0.0, kd
        else:
            assert _rel(pd.grad, ps.grad) < RTOL, kd


def test_csr_cache_never_serves_another_graph():
    """Fresh edge_index tensors every call (what PyG's collate produces): the cached CSR views are keyed on storage the cache keeps alive, so a new
    graph that happens to reuse a freed address cannot hit a stale entry."""
    _require_gpu()
    from morphsym_hgnn_amd import nn as pnn
    ref = _ref_nn()
    r = ref.GraphConv((8, 8), 8, aggr="add").double()
    m = pnn.GraphConv((8, 8), 8, aggr="add").double().cuda()
    _copy_params(m, r)
    g = torch.Generator().manual_seed(0)
    xs, xd = torch.randn(30, 8, dtype=torch.float64, generator=g), torch.randn(20, 8, dtype=torch.float64, generator=g)
    for it in range(40):
        ei = torch.stack([torch.randint(0, 30, (50,), generator=g), torch.randint(0, 20, (50,), generator=g)])
        eg = ei.cuda()                       # a new device tensor per iteration; the previous one is dropped
        y = m((xs.cuda(), xd.cuda()), eg)
        assert _rel(y, r((xs, xd), ei)) < RTOL, it
        del eg
