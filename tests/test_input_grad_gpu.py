"""Gradients with respect to the model's inputs on the fused engines (mshgnn_input_grad, Engine.input_grad, models._EngineFn): x_dict leaves that
require grad get the fp64 oracle's gradient (the reference's autograd through apply_symmetry and the encoder), in their own dtype / shape / device,
whatever the parameters do -- and the parameter gradients stay bit-identical to the same step without input gradients."""
import pytest
import torch

from tests import helpers
from tests.test_models import _build

TOL = {"f32": 1e-4, "x3": 1e-4, "bf16": 2e-2}


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-300))


def _loss(case, m, out, y, B):
    """The wrapper's loss on the module output (gnnLightning.py:633-648, 691)."""
    y_pred = torch.reshape(out.squeeze(), (B, out.numel() // B))
    if case["regression"]:
        return ((y_pred.flatten() - y.to(out.device).flatten()) ** 2).mean()
    return torch.nn.functional.cross_entropy(y_pred.reshape(-1, 2), y.to(out.device).flatten().long())


def _oracle_input_grads(case, spec, params, x_dict, ei, y, B, decisions=None, seed_sum=False):
    """The fp64 oracle's d loss / d x (or d out.sum() / d x), with the engine's relu decisions where it has them (helpers.run_engine_case)."""
    from oracle import ms_hgnn_oracle as orc
    cfg = helpers.oracle_config(spec)

    def relu_fn(key, h):
        if decisions is None or key not in decisions:
            return torch.relu(h)
        rows = helpers.row_live_mask(spec, key, B).view(-1, 1)
        return h * torch.where(rows, decisions[key], h.detach() > 0).to(h.dtype)
    xl = {k: v.detach().double().cpu().clone().requires_grad_(True) for k, v in x_dict.items()}
    o_out = orc.forward(cfg, {k: v.detach().double() for k, v in params.items()}, xl, ei, relu_fn=relu_fn)
    if seed_sum:
        loss = o_out.sum()
    else:
        yy, yp = orc.wrapper_outputs(cfg, o_out, y, B)
        loss = orc.mse_loss(yy, yp) if spec.regression else orc.cross_entropy_loss(yy, yp, B)
    loss.backward()
    return {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in xl.items()}


def _model(case, spec, x_dict, ei, params, precision, monkeypatch, dev="cuda"):
    monkeypatch.setenv("MSHGNN_DTYPE", precision)
    m = _build(case, spec).cuda()
    eid = {k: v.to(dev) for k, v in ei.items()}
    with torch.no_grad():
        m(x_dict={k: v.to(dev).clone() for k, v in x_dict.items()}, edge_index_dict=eid)
    m.load_state_dict(params)
    return m, eid


def _step(case, m, x_dict, eid, y, B, requires_grad, dev="cuda", dtype=torch.float64):
    xd = {k: v.detach().to(device=dev, dtype=dtype).clone().requires_grad_(requires_grad) for k, v in x_dict.items()}
    m.zero_grad()
    out = m(x_dict=xd, edge_index_dict=eid)
    _loss(case, m, out, y, B).backward()
    torch.cuda.synchronize()
    return xd, {k: p.grad.detach().clone() if p.grad is not None else None for k, p in m.named_parameters()}


CASES = ["a1c2_h128_L3_d3_B3", "a1c2_nosym_h128_L2_d3_B2", "a1c2_h128_L2_d3_B37", "mck4_cls_h128_L2_B3", "solok4com_h128_L3_B5",
         "mi_h128_L2_d3_B2", "synth8_mi_h256_L3_B3", "synth32_mi_h512_L6_B2"]


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["f32", "x3", "bf16"])
@pytest.mark.parametrize("name", CASES)
def test_module_input_gradients_match_the_oracle(name, precision, monkeypatch):
    torch.set_default_dtype(torch.float64)
    case, spec, fx, x_dict, y, params, ei = helpers.load_case(name)
    B = case["B"]
    m, eid = _model(case, spec, x_dict, ei, params, precision, monkeypatch)
    _, g_plain = _step(case, m, x_dict, eid, y, B, requires_grad=False)
    xd, g_in = _step(case, m, x_dict, eid, y, B, requires_grad=True)
    e = next(iter(m._engines.values()))
    decisions = helpers.engine_relu_decisions(e, spec, B)
    ref = _oracle_input_grads(case, spec, params, x_dict, ei, y, B, decisions)
    for t in spec.node_types:
        g = xd[t].grad
        assert g is not None and g.dtype == torch.float64 and g.shape == xd[t].shape and g.device == xd[t].device, t
        if float(ref[t].abs().max()) == 0.0:
            assert float(g.abs().max()) == 0.0, t
        else:
            assert _rel(g, ref[t]) < TOL[precision], (t, _rel(g, ref[t]))
    for k in g_plain:      # the parameter gradients do not notice the input gradients
        assert (g_plain[k] is None) == (g_in[k] is None), k
        if g_plain[k] is not None:
            assert torch.equal(g_plain[k], g_in[k]), k


@pytest.mark.gpu
@pytest.mark.parametrize("hidden,precision", [(96, "f32"), (96, "x3"), (200, "x3"), (200, "bf16")])
def test_padded_engine_input_gradients_match_the_oracle(hidden, precision, monkeypatch):
    from morphsym_hgnn_amd import engine as eng, synth
    torch.set_default_dtype(torch.float64)
    spec = helpers.make_spec("c2", "a1-c2", "a1-c2", hidden, 2)
    case = {"kind": "c2", "cfg": "a1-c2", "hidden": hidden, "layers": 2, "regression": True, "grf": 3}
    B = 5
    x_dict, y = synth.make_windows(4, B, spec.num_nodes, spec.widths, spec.out_channels * spec.num_nodes[spec.out_type])
    params = synth.make_params(4, spec.param_shapes())
    ei = spec.topology.edge_index_dict(B)
    m, eid = _model(case, spec, x_dict, ei, params, precision, monkeypatch)
    xd, _ = _step(case, m, x_dict, eid, y, B, requires_grad=True)
    e = next(iter(m._engines.values()))
    assert isinstance(e, eng.PaddedEngine)
    ref = _oracle_input_grads(case, spec, params, x_dict, ei, y.double(), B, helpers.engine_relu_decisions(e, spec, B))
    for t in spec.node_types:
        if float(ref[t].abs().max()) == 0.0:
            assert float(xd[t].grad.abs().max()) == 0.0, t
        else:
            assert _rel(xd[t].grad, ref[t]) < TOL[precision], (t, _rel(xd[t].grad, ref[t]))


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["f32", "x3", "bf16"])
def test_inputs_of_nodes_that_cannot_reach_the_output_get_exact_zeros(precision, monkeypatch):
    """A1-C2 at L = 3: the base nodes are four hops from the feet; the plan never computes them, their stash rows hold the workspace's poison
    (MSHGNN_POISON_WS=1) -- and their gradient is exactly 0, as in the oracle."""
    monkeypatch.setenv("MSHGNN_POISON_WS", "1")
    torch.set_default_dtype(torch.float64)
    case, spec, fx, x_dict, y, params, ei = helpers.load_case("a1c2_h128_L3_d3_B3")
    m, eid = _model(case, spec, x_dict, ei, params, precision, monkeypatch)
    xd, _ = _step(case, m, x_dict, eid, y, case["B"], requires_grad=True)
    ref = _oracle_input_grads(case, spec, params, x_dict, ei, y, case["B"])
    assert float(ref["base"].abs().max()) == 0.0
    assert torch.count_nonzero(xd["base"].grad) == 0 and bool(torch.isfinite(xd["joint"].grad).all())


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["x3", "bf16"])
def test_frozen_parameters_input_gradient_runs_no_weight_gradient_launch(precision, monkeypatch):
    torch.set_default_dtype(torch.float64)
    case, spec, fx, x_dict, y, params, ei = helpers.load_case("a1c2_h128_L3_d3_B3")
    B = case["B"]
    m, eid = _model(case, spec, x_dict, ei, params, precision, monkeypatch)
    m.requires_grad_(False)
    e = next(iter(m._engines.values()))
    xj = x_dict["joint"].cuda().clone().requires_grad_(True)
    xd = {k: (xj if k == "joint" else v.cuda()) for k, v in x_dict.items()}
    out = m(x_dict=xd, edge_index_dict=eid)
    assert out.requires_grad
    e.profile(True)
    (g,) = torch.autograd.grad(out.sum(), [xj])
    stats = e.profile_read()
    e.profile(False)
    ran = {s["name"]: s["launches"] for s in stats}
    assert ran.get("gradw", 0) == 0 and ran.get("finalize", 0) == 0, ran
    assert all(p.grad is None for p in m.parameters())
    ref = _oracle_input_grads(case, spec, params, x_dict, ei, y, B, helpers.engine_relu_decisions(e, spec, B), seed_sum=True)
    assert _rel(g, ref["joint"]) < TOL[precision]


@pytest.mark.gpu
def test_layouts_dtypes_devices_and_determinism(monkeypatch):
    from morphsym_hgnn_amd import engine as eng
    torch.set_default_dtype(torch.float64)
    case, spec, fx, x_dict, y, params, ei = helpers.load_case("a1c2_h128_L2_d3_B37")
    B = case["B"]
    m, eid = _model(case, spec, x_dict, ei, params, "x3", monkeypatch)
    ref = _oracle_input_grads(case, spec, params, x_dict, ei, y, B)
    # only one type requires grad; fp32 inputs give fp32 gradients
    xd = {k: v.cuda().float() for k, v in x_dict.items()}
    xd["foot"].requires_grad_(True)
    _loss(case, m, m(x_dict=xd, edge_index_dict=eid), y, B).backward()
    assert xd["foot"].grad.dtype == torch.float32 and xd["joint"].grad is None
    assert _rel(xd["foot"].grad, ref["foot"]) < 1e-4
    # rows already at the engine's pitch: a gradient of that shape, exact-zero pad columns
    P = eng.row_pitch(spec.widths["joint"], 4)
    xj = torch.zeros(B * spec.num_nodes["joint"], P, dtype=torch.float32, device="cuda")
    xj[:, :spec.widths["joint"]] = x_dict["joint"].float().cuda()
    xj.requires_grad_(True)
    xd = {k: (xj if k == "joint" else v.cuda().float()) for k, v in x_dict.items()}
    _loss(case, m, m(x_dict=xd, edge_index_dict=eid), y, B).backward()
    assert xj.grad.shape == xj.shape and torch.count_nonzero(xj.grad[:, spec.widths["joint"]:]) == 0
    assert _rel(xj.grad[:, :spec.widths["joint"]], ref["joint"]) < 1e-4
    # host inputs give host gradients
    xh = {k: v.clone().requires_grad_(True) for k, v in x_dict.items()}
    _loss(case, m, m(x_dict=xh, edge_index_dict=eid), y, B).backward()
    assert xh["joint"].grad.device.type == "cpu" and _rel(xh["joint"].grad, ref["joint"]) < 1e-4
    # a forward on other data between forward and backward raises
    xa = {k: v.cuda().clone().requires_grad_(True) for k, v in x_dict.items()}
    out = m(x_dict=xa, edge_index_dict=eid)
    m(x_dict={k: (v * 2).cuda().requires_grad_(True) for k, v in x_dict.items()}, edge_index_dict=eid)
    with pytest.raises(RuntimeError, match="overwritten"):
        _loss(case, m, out, y, B).backward()
    # two identical runs give identical bits
    g = []
    for _ in range(2):
        xr, _ = _step(case, m, x_dict, eid, y, B, requires_grad=True)
        g.append({k: v.grad.clone() for k, v in xr.items()})
    assert all(torch.equal(g[0][k], g[1][k]) for k in g[0])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,tol", [("f32", 1e-6), ("x3", 1e-4), ("bf16", 1e-2)])
def test_engine_input_grad_is_the_encoder_product_of_its_own_stash(dtype, tol):
    """Engine.input_grad after Engine.backward == (dY_enc @ W_enc) . mask rebuilt in torch from the engine's own dX_0 stash, at 1024 windows: per node
    within `tol` (relative to the node's largest element) of the product with the fp32 W, and per element within 2 n 2^-24 sum|terms| of the product
    with W in the plan's operand form (helpers.check_input_grad_against_own_operands)."""
    from morphsym_hgnn_amd import engine as eng
    spec = helpers.make_spec("c2", "a1-c2", "a1-c2", 128, 2)
    B = 1024
    x_dict, y, params = helpers.random_case(spec, B, 11)
    e = eng.Engine(spec, dtype, device="cuda:0")
    xs = e.cast_inputs(x_dict)
    flat = eng.flatten_params(spec, params, device=e.device)
    out = e.forward(xs, flat, B, training=True)
    gout = torch.randn(out.numel(), generator=torch.Generator().manual_seed(3)).float().cuda()
    e.backward(xs, flat, gout, B)
    got = e.input_grad(B, flat, dtype=torch.float64)
    dY = e.grad_hidden(B, 0).double()      # [B, NN, H]
    _, need = spec.node_liveness()
    masks = spec.input_masks()
    base = 0
    for t in spec.node_types:
        W = params[f"encoder.lins.{t}.weight"].double().cuda()      # [H, F]
        g = got[t].view(B, spec.num_nodes[t], -1)
        for i in range(spec.num_nodes[t]):
            if i in need[0][t]:
                ref = (dY[:, base + i] @ W) * masks[t][i].double().cuda()
                assert float((g[:, i] - ref).abs().max() / ref.abs().max()) < tol, (t, i)
            else:
                assert torch.count_nonzero(g[:, i]) == 0, (t, i)
        base += spec.num_nodes[t]
    for dt in (torch.float32, torch.float64):
        assert helpers.check_input_grad_against_own_operands(e, spec, params, B, e.input_grad(B, flat, dtype=dt)) <= 1.0
    with pytest.raises(RuntimeError, match="overwritten"):
        e.forward(xs, flat, B, training=True)
        e.input_grad(B, flat)


def _own_operands_case(spec, dtype, B, seed, dt=torch.float64):
    from morphsym_hgnn_amd import engine as eng
    x_dict, y, params = helpers.random_case(spec, B, seed)
    e = eng.make_engine(spec, dtype)
    xs = e.cast_inputs(x_dict)
    flat = eng.flatten_params(spec, params, device=e.device)
    out = e.forward(xs, flat, B, training=True)
    gout = (torch.randn(out.numel(), generator=torch.Generator().manual_seed(seed + 1)) * 1e-3).float().cuda()
    e.backward(xs, flat, gout, B)
    got = e.input_grad(B, flat, dtype=dt)
    torch.cuda.synchronize()
    return e, x_dict, params, gout, got


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["bf16", "x3"])
@pytest.mark.parametrize("hidden", [640, 1536, 2048])
def test_wide_input_grad_is_the_product_of_the_engines_own_operands(hidden, dtype):
    """The generic engine at hidden 640 (column chunks of 32 / 16), 1536 and 2048: every launch form of the kernel whose LDS exceeds 64 KB (bf16 at
    2048: 65 792 bytes; split at 1536 / 2048: 98 816 / 131 584), at 70 and 300 windows, held to the engine's own operands; at 70 windows also to the
    fp64 oracle under the engine's relu decisions (1e-4 split, 2e-2 bf16)."""
    from oracle import ms_hgnn_oracle as orc
    spec = helpers.make_spec("c2", "a1-c2", "a1-c2", hidden, 2)
    for B in (70, 300):
        e, x_dict, params, gout, got = _own_operands_case(spec, dtype, B, 5)
        assert e.generic
        assert helpers.check_input_grad_against_own_operands(e, spec, params, B, got) <= 1.0
        if B == 70:
            decisions = helpers.engine_relu_decisions(e, spec, B)

            def relu_fn(key, h):
                if key not in decisions:
                    return torch.relu(h)
                rows = helpers.row_live_mask(spec, key, B).view(-1, 1)
                return h * torch.where(rows, decisions[key], h.detach() > 0).to(h.dtype)
            xl = {k: v.clone().requires_grad_(True) for k, v in x_dict.items()}
            o = orc.forward(helpers.oracle_config(spec), {k: v.double() for k, v in params.items()}, xl, spec.topology.edge_index_dict(B), relu_fn=relu_fn)
            o.backward(gout.double().cpu().reshape(o.shape))
            for t in spec.node_types:
                ref = xl[t].grad if xl[t].grad is not None else torch.zeros_like(xl[t])
                if float(ref.abs().max()) == 0.0:
                    assert float(got[t].abs().max()) == 0.0, t
                else:
                    assert _rel(got[t], ref) < TOL[dtype], (t, _rel(got[t], ref))
        del e


@pytest.mark.gpu
def test_input_grad_at_65536_windows_is_the_product_of_the_engines_own_operands():
    """A1-C2 h128 split plan, two-call route (forward + backward: never chunked) at 65 536 windows: 64 row tiles per workgroup."""
    spec = helpers.make_spec("c2", "a1-c2", "a1-c2", 128, 3)
    e, _, params, _, got = _own_operands_case(spec, "x3", 65536, 7, dt=torch.float32)
    assert helpers.check_input_grad_against_own_operands(e, spec, params, 65536, got) <= 1.0


def _abi_setup(dtype="x3", B=37):
    from morphsym_hgnn_amd import engine as eng
    spec = helpers.make_spec("c2", "a1-c2", "a1-c2", 128, 4)
    x_dict, y, params = helpers.random_case(spec, B, 13)
    e = eng.Engine(spec, dtype, device="cuda:0")
    xs = e.cast_inputs(x_dict)
    flat = eng.flatten_params(spec, params, device=e.device)
    out = e.forward(xs, flat, B, training=True)
    e.backward(xs, flat, torch.randn(out.numel(), generator=torch.Generator().manual_seed(2)).float().cuda(), B)
    return spec, e, flat


def _abi_call(e, flat, B, bufs, pitches, dx_bytes, ws_B=None):
    """mshgnn_input_grad through ctypes: bufs / pitches per type (None: NULL), pitches=None: a NULL dx_pitch; the workspace of batch ws_B (default B)."""
    import ctypes as C
    n = len(e.types)
    ptrs = (C.c_void_p * n)(*[b if b is not None else None for b in bufs])
    pitch = None if pitches is None else (C.c_int64 * n)(*pitches)
    stream = torch.cuda.current_stream(e.device).cuda_stream
    rc = e.lib.mshgnn_input_grad(e._plan, flat.data_ptr(), ptrs, pitch, dx_bytes, e.workspace(ws_B or B, True).data_ptr(), B, stream)
    torch.cuda.synchronize()
    return rc


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [torch.float32, torch.float64])
def test_c_abi_layouts_write_every_element_of_the_callers_rows(dt):
    """NaN-filled buffers at pitches F, F + 1, F + 3 and ceil(F / 64) 64 + 5, base pointers one element off 16 bytes (no 16-byte stores), the last type
    alone (type 0 NULL) and a NULL dx_pitch: columns [0, F) are the dense result's bits, [F, pitch) are +0.0, no NaN is left."""
    B = 37
    spec, e, flat = _abi_setup()
    dense = e.input_grad(B, flat, dtype=dt)
    es = torch.empty(0, dtype=dt).element_size()
    types = list(e.types)
    F = [spec.widths[t] for t in types]
    rows = [B * spec.num_nodes[t] for t in types]

    def run(pitches, shift, only=None, null_pitch=False):
        store, ptrs = [], []
        for k, t in enumerate(types):
            if only is not None and k != only:
                store.append(None)
                ptrs.append(None)
                continue
            buf = torch.full((rows[k] * pitches[k] + shift + 8,), float("nan"), dtype=dt, device="cuda")
            store.append(buf)
            ptrs.append(buf.data_ptr() + shift * es)
        assert _abi_call(e, flat, B, ptrs, None if null_pitch else pitches, es) == 0, e.lib.mshgnn_last_error()
        for k, t in enumerate(types):
            if store[k] is None:
                continue
            buf = store[k]
            assert bool(torch.isnan(buf[:shift]).all()) and bool(torch.isnan(buf[shift + rows[k] * pitches[k]:]).all()), (t, "wrote outside its rows")
            v = buf[shift:shift + rows[k] * pitches[k]].view(rows[k], pitches[k])
            what = (t, pitches[k], shift)
            assert not bool(torch.isnan(v).any()), what
            assert torch.equal(v[:, :F[k]], dense[t]), what
            pad = v[:, F[k]:]
            assert torch.count_nonzero(pad) == 0 and not bool(torch.signbit(pad).any()), what

    for extra in (lambda f: f, lambda f: f + 1, lambda f: f + 3, lambda f: (f + 63) // 64 * 64 + 5):
        pitches = [extra(f) for f in F]
        for shift in (0, 1):
            run(pitches, shift)
    run(F, 0, only=len(types) - 1)
    run(F, 1, only=len(types) - 1)
    run(F, 0, null_pitch=True)


@pytest.mark.gpu
def test_c_abi_error_returns_launch_nothing():
    B = 37
    spec, e, flat = _abi_setup()
    types = list(e.types)
    F = [spec.widths[t] for t in types]
    bufs = [torch.full((B * spec.num_nodes[t] * F[k],), float("nan"), device="cuda") for k, t in enumerate(types)]
    ptrs = [b.data_ptr() for b in bufs]
    assert _abi_call(e, flat, B, ptrs, F, 2) == -2                                              # MSHGNN_EUNSUPPORTED
    assert _abi_call(e, flat, B, ptrs, [F[0], F[1] - 1, F[2]], 4) == -1                        # MSHGNN_EINVAL: pitch < F
    assert _abi_call(e, flat, 0, ptrs, F, 4, ws_B=B) == -1                                     # MSHGNN_EINVAL: batch 0
    assert _abi_call(e, flat, B, [None] * len(types), F, 4) == 0                              # nothing requested
    assert all(bool(torch.isnan(b).all()) for b in bufs), "an error return wrote"


@pytest.mark.gpu
def test_lds_attribute_holds_across_plans_of_different_modes_at_2048():
    """bf16, then split, then bf16 again at hidden 2048 in one process (65 792 and 131 584 bytes of LDS: the attribute is set once per instantiation)."""
    spec = helpers.make_spec("c2", "a1-c2", "a1-c2", 2048, 2)
    for dtype in ("bf16", "x3", "bf16"):
        e, _, params, _, got = _own_operands_case(spec, dtype, 40, 9)
        assert helpers.check_input_grad_against_own_operands(e, spec, params, 40, got) <= 1.0
        del e


@pytest.mark.gpu
def test_input_grad_at_8208_windows_is_deterministic():
    spec, e, flat = _abi_setup("bf16", 8208)
    a = e.input_grad(8208, flat, dtype=torch.float32)
    b = e.input_grad(8208, flat, dtype=torch.float32)
    assert all(torch.equal(a[t], b[t]) for t in a)


@pytest.mark.gpu
def test_wrapper_training_step_delivers_input_gradients(monkeypatch):
    from tests.test_wrappers import _batch, _wrapper
    monkeypatch.setenv("MSHGNN_DTYPE", "x3")
    torch.set_default_dtype(torch.float64)
    case, spec, fx, x_dict, y, params, ei = helpers.load_case("a1c2_h128_L3_d3_B3")
    B = case["B"]
    batch = _batch(x_dict, ei, y, B, torch.device("cuda"))
    w = _wrapper(case, spec, batch).to("cuda")
    w.model.load_state_dict(params)
    w.training_step(batch, 0)
    assert w.model._gpend_id == 1      # no input requires grad: the one-call step
    batch.x_dict = {k: v.clone().requires_grad_(True) for k, v in batch.x_dict.items()}
    loss = w.training_step(batch, 1)
    assert w.model._gpend_id == 1      # inputs require grad: the two-call route
    w.model.zero_grad()
    loss.backward()
    ref = _oracle_input_grads(case, spec, params, x_dict, ei, y, B)
    assert _rel(batch.x_dict["joint"].grad, ref["joint"]) < 1e-4
    assert all(p.grad is not None for p in w.model.parameters())
