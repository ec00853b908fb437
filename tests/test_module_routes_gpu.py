"""The parameter routes of the module's two-call path (models._EngineFn: "fast", "flat", "p", None) with and without input gradients, against EACH OTHER:
the engine's forward and backward are deterministic and every route feeds them the same fp32 parameters, so outputs and gradients are equal bit for bit
whichever way the parameters and their gradients travel.  (The values themselves are held to the oracle by test_models.py and test_input_grad_gpu.py.)
37 windows: two whole 16-window tiles and a ragged one.
Every equality asserted here was first run against the four separate Functions this one replaced (_EngineFn, _EngineFnP, _EngineFnFast, _EngineFnIn): all cases
passed there unchanged, on both plans -- no pair differed, so no weaker relation is asserted anywhere."""
import datetime
import os
import time

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import helpers
from tests.test_models import _build

CASE = "a1c2_h128_L2_d3_B37"
STALE = "the activation stash of this forward was overwritten by a later forward of the same batch size on the same engine"


def _model(case, spec, params, x_dict, eid, param_dev):
    """A model with the case's parameters on `param_dev` ("cuda": views of the flat buffer; "cpu": a device copy per forward), after its lazy-initialising forward."""
    m = _build(case, spec)
    if param_dev == "cuda":
        m = m.cuda()
    with torch.no_grad():
        m(x_dict={k: v.clone() for k, v in x_dict.items()}, edge_index_dict=eid)
    m.load_state_dict(params)
    return m


def _run(m, x_dict, eid, gout, leaf):
    """forward + backward(gout) -> (out, {name: parameter gradient in fp32 | None}, the joint leaf's gradient | None)."""
    xd = dict(x_dict)
    if leaf:
        xd["joint"] = x_dict["joint"].clone().requires_grad_(True)
    m.zero_grad()
    out = m(x_dict=xd, edge_index_dict=eid)
    out.backward(gout)
    torch.cuda.synchronize()
    grads = {k: (p.grad.detach().to("cpu", torch.float32).clone() if p.grad is not None else None) for k, p in m.named_parameters()}
    return out.detach().cpu(), grads, (xd["joint"].grad.detach().cpu() if leaf else None)


def _same(a, b):
    return a.keys() == b.keys() and all((a[k] is None and b[k] is None) or torch.equal(a[k], b[k]) for k in a)


def _setup(shard=None):
    """The golden case on the device in fp64 (optionally one rank's shard of it) and a fixed upstream gradient.  (The plan is MSHGNN_DTYPE's, read when a model is built.)"""
    from morphsym_hgnn_amd import ddp
    torch.set_default_dtype(torch.float64)
    case, spec, fx, x_dict, y, params, ei = helpers.load_case(CASE)
    B = case["B"]
    if shard is not None:
        x_dict, (b, en) = ddp.shard_x_dict(x_dict, spec.num_nodes, B, *shard)
        B = en - b
    x_dict = {k: v.cuda() for k, v in x_dict.items()}
    eid = spec.topology.edge_index_dict(B, device="cuda")
    gout = torch.randn(B, 12, generator=torch.Generator().manual_seed(5)).cuda()
    return case, spec, params, x_dict, eid, gout, B


@pytest.mark.gpu
@pytest.mark.parametrize("plan", ["bf16", "x3"])
def test_route_matrix_is_bit_identical(plan, monkeypatch):
    """Device parameters ("fast") or host parameters ("flat"), without or with an fp64 joint leaf that requires grad: one output, one set of parameter gradients,
    one leaf gradient.  Then the device model frozen (route None): no parameter gets a .grad and the leaf's gradient is still the same."""
    monkeypatch.setenv("MSHGNN_DTYPE", plan)
    case, spec, params, x_dict, eid, gout, B = _setup()
    got = {}
    for dev in ("cuda", "cpu"):
        m = _model(case, spec, params, x_dict, eid, dev)
        for leaf in (False, True):
            got[dev, leaf] = _run(m, x_dict, eid, gout, leaf)
        if dev == "cuda":
            m.requires_grad_(False)
            frozen = _run(m, x_dict, eid, gout, True)
    ref_out, ref_grads, _ = got["cuda", False]
    assert all(g is not None for g in ref_grads.values()) and bool(ref_grads["decoder.weight"].abs().max() > 0)
    for key, (out, grads, gx) in got.items():
        assert torch.equal(out, ref_out), key
        assert _same(grads, ref_grads), key
    gx_fast, gx_flat = got["cuda", True][2], got["cpu", True][2]
    assert gx_fast.dtype == torch.float64 and bool(gx_fast.abs().max() > 0) and torch.equal(gx_fast, gx_flat)
    assert torch.equal(frozen[0], ref_out) and all(g is None for g in frozen[1].values()) and torch.equal(frozen[2], gx_fast)


@pytest.mark.gpu
@pytest.mark.parametrize("plan", ["bf16", "x3"])
def test_stale_stash_raises_on_every_route(plan, monkeypatch):
    """forward(A), forward(B) at the same batch size, backward(A): the engine's stash holds B's activations -- an error, not a wrong gradient."""
    monkeypatch.setenv("MSHGNN_DTYPE", plan)
    case, spec, params, x_dict, eid, gout, B = _setup()
    other = {k: v * 2 for k, v in x_dict.items()}
    for dev, leaf in (("cuda", False), ("cpu", False), ("cuda", True)):
        m = _model(case, spec, params, x_dict, eid, dev)
        xa, xb = dict(x_dict), dict(other)
        if leaf:
            xa["joint"], xb["joint"] = xa["joint"].clone().requires_grad_(True), xb["joint"].clone().requires_grad_(True)
        out = m(x_dict=xa, edge_index_dict=eid)
        m(x_dict=xb, edge_index_dict=eid)
        with pytest.raises(RuntimeError) as err:
            out.backward(gout)
        assert STALE in str(err.value), (dev, leaf)


def _p_worker(rank, world, port, precision, ret):
    """One of two ranks on the one GPU (gloo): its shard of the 37 windows on the fast route with the leaf BEFORE it joins the group, then on route "p" under
    ddp.flat_data_parallel without and with the leaf."""
    from morphsym_hgnn_amd import ddp
    os.environ["MSHGNN_DTYPE"] = precision
    case, spec, params, x_dict, eid, gout, B = _setup(shard=(rank, world))
    m = _model(case, spec, params, x_dict, eid, "cuda")
    _, _, gx_fast = _run(m, x_dict, eid, gout, True)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
    ddp.flat_data_parallel(m)
    _, g_plain, _ = _run(m, x_dict, eid, gout, False)
    _, g_leaf, gx_p = _run(m, x_dict, eid, gout, True)
    mine = torch.cat([g.flatten() for g in g_plain.values()])
    both = [torch.zeros_like(mine) for _ in range(world)]
    dist.all_gather(both, mine)
    ret[f"windows_{rank}"] = B
    ret[f"exchanged_{rank}"] = bool(torch.equal(both[0], both[1])) and bool(mine.abs().max() > 0)      # the flat exchange ran: both ranks hold one gradient
    ret[f"params_{rank}"] = _same(g_plain, g_leaf)
    ret[f"leaf_{rank}"] = bool(torch.equal(gx_p, gx_fast)) and bool(gx_p.abs().max() > 0)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["bf16", "x3"])
def test_route_p_under_two_ranks(precision):
    """Route "p" (parameters as autograd inputs under torch.distributed): the parameter gradients do not notice the input gradients, and the leaf's gradient
    is the one the fast route gave the same process -- input gradients are local, never exchanged."""
    world = 2
    mgr = mp.Manager()
    ret = mgr.dict()
    ctx = mp.spawn(_p_worker, args=(world, 37000 + (os.getpid() % 2000), precision, ret), nprocs=world, join=False)
    deadline = time.monotonic() + 150
    while not ctx.join(timeout=5):
        if time.monotonic() > deadline:
            for p in ctx.processes:
                p.kill()
            pytest.fail("the two ranks did not finish in time")
    assert ret["windows_0"] + ret["windows_1"] == 37 and ret["windows_0"] != ret["windows_1"]
    for rank in range(world):
        assert ret[f"exchanged_{rank}"] and ret[f"params_{rank}"] and ret[f"leaf_{rank}"], dict(ret)
