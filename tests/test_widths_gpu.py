"""GPU parity sweep over hidden widths (the reference takes any hidden_channels, hgnn_c2.py:11; its scripts expose it as --hidden_size).

Two routes serve a width: the generic-width engine (mshgnn_gen.hip) for every multiple of 128 up to 2048, whose job kernels are chosen per launch from
NCT = hidden / 128, the batch and the storage (g_launch_jobs, and the weight-gradient launch after it), and engine.PaddedEngine for every other width
(zero rows / columns up to the next multiple of 128).  Every case compares the HIP engine with the fp64 oracle evaluated with the engine's own relu
decisions (tests/helpers.py): x3 / f32 every stage within 1e-4, bf16 within 3e-2 with decisions within 3e-2 of zero; reference gradients that are
exactly zero must come back exactly zero."""
import pytest
import torch

from tests import helpers

pytestmark = pytest.mark.gpu
RTOL = 1e-4          # x3 / f32 (as tests/test_generic_gpu.py)
BF16_TOL = 3e-2      # bf16 (as test_generic_bf16_arithmetic_is_within_bf16_distance_of_the_oracle)


def mi_spec(hidden, limbs=1, layers=2):
    """The MI graph of a robot of `limbs` three-joint limbs, narrow inputs: the host oracle stays cheap at any width."""
    from morphsym_hgnn_amd import topology
    from morphsym_hgnn_amd.spec import ModelSpec
    return ModelSpec(kind="mi", topology=topology.synthetic_limbs(limbs), hidden=hidden, num_layers=layers, widths={"base": 24, "joint": 9, "foot": 5},
                     regression=True, grf_dimension=1, group=None, num_timesteps=3)


def k4_cls_spec(hidden):
    return helpers.make_spec("k4", "mini_cheetah-k4", "mini_cheetah-k4", hidden, 2, regression=False)


def _tol(dtype):
    return (BF16_TOL, {"decision_tol": BF16_TOL}) if dtype == "bf16" else (RTOL, {})


def _assert_parity(errs, ref, tol, what):
    bad = {k: v for k, v in errs.items() if v > tol}
    assert not bad, f"{what}: stages above {tol}: {bad}"
    assert errs["relu_decisions_outside_tolerance"] == 0.0, what
    for k, g in ref["grads"].items():
        if float(g.abs().max()) == 0.0:
            assert errs["grad:" + k] == 0.0, f"{what}: {k} has an exact-zero reference gradient, the engine's is {errs['grad:' + k]:.3e}"


def _engine_case(spec, e, dtype, B, seed, what):
    """forward (training) + MSE / CE seed + backward of `e` against the oracle: every hidden state, the output, the loss, every gradient."""
    x_dict, y, params = helpers.random_case(spec, B, seed)
    tol, kw = _tol(dtype)
    errs, out, loss, grads = helpers.run_engine_case(spec, x_dict, y, params, spec.topology.edge_index_dict(B), B, dtype=dtype, engine=e, **kw)
    _assert_parity(errs, helpers.run_engine_case.last_reference, tol, what)
    return x_dict, y, params, out, grads


def _step_case(spec, e, dtype, B, seed, what):
    """The one-call step (step_mse / step_ce) of `e` against the oracle."""
    x_dict, y, params = helpers.random_case(spec, B, seed)
    tol, kw = _tol(dtype)
    errs, out, loss, grads = helpers.run_step_case(spec, x_dict, y, params, B, dtype=dtype, engine=e, **kw)
    _assert_parity(errs, helpers.run_step_case.last_reference, tol, what)
    return x_dict, y, params, out, loss, grads


def _generic(spec, dtype):
    from morphsym_hgnn_amd import engine as eng
    e = eng.Engine(spec, dtype)
    assert e.generic and e.info.kernel_sets == 4
    assert e.storage == ("bf16" if dtype == "bf16" else "x3")
    return e


# ---------------------------------------------------------------------------------------------------
# 1. the generic-width engine across NCT = hidden / 128
# ---------------------------------------------------------------------------------------------------
# (hidden, limbs, layers, dtype, B).  The dispatch each row is there for:
#   bf16, odd NCT (128 forced generic, 384, 640, 1152): k_gstep<false,4,4> for every job launch (tile mode 3 below 256 windows, 8 from 256: no k_gstep5 at an odd
#     NCT, not even the RAW encoder) and the OS=1 weight-gradient super-units k_ggradw<false,1,8,true> (su_os is 2 only for an even NCT);
#   x3 / f32, odd NCT: k_gstep<true,4,4> with 1, 3, 5, 9 column groups, k_ggradw<true,1,8,true>;
#   x3, NCT = 6 (768): k_gstep<true,4,8> on three column groups, k_ggradw<true,2,...>; bf16 at 768: k_gstep<false,4,8> / the 4-wave k_gstep5 (half_only);
#   NCT > 8 (1152, 1536, 2048): every kernel with up to 16 column tiles, k_gdec_fwd / k_gdec_bwd over 9-16 column groups, the decoder slab SF = 8 Hd + 16;
#   B < 256 (70, 33): tile mode 3 on bf16; B = 300: three 128-window tiles, the last one ragged (mode 8); B = 1: one window in a 64 / 128-window tile.
GENERIC_CASES = (
    [(128, 3, 2, dt, B) for dt in ("bf16", "x3") for B in (1, 70, 300)]
    + [(384, 3, 2, dt, B) for dt in ("bf16", "x3", "f32") for B in (1, 70, 300)]
    + [(640, 2, 3, dt, B) for dt in ("bf16", "x3") for B in (70, 300)]
    + [(768, 3, 2, dt, B) for dt in ("bf16", "x3") for B in (1, 70, 300)]
    + [(1152, 2, 2, dt, B) for dt in ("bf16", "x3") for B in (70, 300)]
    + [(1536, 1, 2, dt, B) for dt in ("bf16", "x3") for B in (1, 70, 300)]
    + [(2048, 1, 2, "bf16", 70), (2048, 1, 2, "x3", 70), (2048, 1, 2, "f32", 33)]
)


@pytest.mark.parametrize("hidden,limbs,layers,dtype,B", GENERIC_CASES)
def test_generic_width_matches_the_oracle(hidden, limbs, layers, dtype, B, monkeypatch):
    """forward + backward at NCT = 1, 3, 5, 6, 9, 12 and 16 (hidden 128 .. 2048, the advertised maximum) on both storages (f32 requests run the split
    arithmetic): every hidden state, the output, the loss and every gradient against the oracle."""
    if hidden == 128:
        monkeypatch.setenv("MSHGNN_ENGINE", "generic")      # (the LDS-resident kernels take this model otherwise)
    spec = mi_spec(hidden, limbs, layers)
    e = _generic(spec, dtype)
    _engine_case(spec, e, dtype, B, 1000 + hidden + B, f"h{hidden} {dtype} B={B}")


@pytest.mark.parametrize("dtype", ["bf16", "x3"])
@pytest.mark.parametrize("B", [256, 1100])
def test_generic_step_on_both_sides_of_the_pipelined_kernels_wave_switch(B, dtype):
    """hidden 512 (NCT % 4 == 0) on a 16-limb robot: the default dispatch of the bf16 plan runs k_gstep5 at 8 waves while a launch has at most as many
    (job, 128-window tile) pairs as the GPU has CUs and at 4 waves (two workgroups per CU) above that -- the RAW encoder launch the same way.  256 windows:
    at most 48 jobs x 2 tiles, every launch 8-wave; 1100 windows (9 tiles, the last ragged): the 48-job encoder and the 32-job first layer switch to 4 waves,
    the 16-job last layer stays at 8.  The split plan runs k_gstep5<true> at both.  One-call step against the oracle."""
    spec = mi_spec(512, 16, 2)
    e = _generic(spec, dtype)
    _step_case(spec, e, dtype, B, 77 + B, f"h512 {dtype} B={B}")


@pytest.mark.parametrize("dtype", ["bf16", "x3"])
@pytest.mark.parametrize("hidden", [384, 512])
@pytest.mark.parametrize("mode", ["0", "1", "2", "3", "6", "8", "9"])
def test_forced_tile_modes_match_the_oracle(mode, hidden, dtype, monkeypatch):
    """MSHGNN_GEN_TILE (read per launch) forces each job-kernel form at an odd (384) and an even (512) NCT on 300 windows: 0 -> k_gstep<*,4,4>;
    1 -> k_gstep<*,8,8> (128-window tiles, even NCT) / <*,4,4> (odd); 2 -> k_gstep<*,4,8> / <*,4,4>; 3 -> the widest k_gstep the NCT allows;
    6 -> k_gstep4 (NCT % 4 == 0); 8 -> k_gstep5 at 8 waves (the RAW encoder too, bf16); 9 -> k_gstep5 at 4 waves -- each against the oracle under its own
    decisions (the split forms are not bit-identical to each other: tests/test_generic_gpu.py, test_job_kernels_of_the_generic_engine_agree_bit_for_bit).
    Tolerances over whole tensors here; the same table of modes meets the oracle bit for bit, on rounding-free data, in tests/test_exact_generic_gpu.py."""
    monkeypatch.setenv("MSHGNN_GEN_TILE", mode)
    spec = mi_spec(hidden, 2, 2)
    e = _generic(spec, dtype)
    _engine_case(spec, e, dtype, 300, 500 + hidden, f"mode {mode} h{hidden} {dtype}")


@pytest.mark.parametrize("dtype", ["bf16", "x3"])
@pytest.mark.parametrize("hidden", [384, 1024])
def test_generic_classification_matches_the_oracle(hidden, dtype):
    """Cross entropy over the per-foot logit pairs (the CE branch of k_gdec_bwd) at NCT = 3 and 8 on the K4 classification model: the one-call step_ce
    against the oracle, then forward + backward_ce on the same engine gives the same bits (the generic step is that pair of calls)."""
    spec = k4_cls_spec(hidden)
    e = _generic(spec, dtype)
    B = 37
    x_dict, y, params, out, loss, grads = _step_case(spec, e, dtype, B, 3 + hidden, f"ce h{hidden} {dtype}")
    from morphsym_hgnn_amd import engine as eng
    xs = e.cast_inputs(x_dict)
    flat = eng.flatten_params(spec, params, e.device)
    lab = y.reshape(B, -1).to(e.device, torch.int32).contiguous()
    out2 = e.forward(xs, flat, B, training=True)
    loss2, g2 = e.backward_ce(xs, flat, out2, lab, B)
    torch.cuda.synchronize()
    assert torch.equal(out2.cpu(), out) and torch.equal(loss2.cpu(), loss)
    assert all(torch.equal(g, grads[k]) for k, g in eng.unflatten(spec, g2.cpu()).items())


def test_dense_bf16_inputs_leave_the_raw_encoder_with_the_same_bits():
    """bf16 inputs at their dense width (cast_inputs(pad=False): 9- and 5-element rows, no whole 16-byte chunks) fail g_raw_ok, so the encoder launch of a
    300-window step at NCT = 6 drops from k_gstep5<RAW> to the plain job kernel: same bits as the padded-pitch inputs, and within bf16 distance of the oracle."""
    from morphsym_hgnn_amd import engine as eng
    spec = mi_spec(768, 2, 2)
    e = _generic(spec, "bf16")
    B = 300
    x_dict, y, params, out, loss, grads = _step_case(spec, e, "bf16", B, 91, "h768 padded-pitch")
    flat = eng.flatten_params(spec, params, e.device)
    yd = y.reshape(-1).to(e.device, torch.float32)
    xs = e.cast_inputs(x_dict, pad=False)
    assert [x.shape[1] for x in xs] == [spec.widths[t] for t in spec.node_types]
    o2, l2, g2 = e.step_mse(xs, flat, yd, B)
    torch.cuda.synchronize()
    assert torch.equal(o2.cpu(), out) and torch.equal(l2.cpu(), loss)
    assert all(torch.equal(g, grads[k]) for k, g in eng.unflatten(spec, g2.cpu()).items())


@pytest.mark.parametrize("dtype", ["bf16", "x3"])
def test_generic_odd_width_step_is_deterministic_and_equals_the_two_call_sequence(dtype):
    """NCT = 5 (hidden 640) on 300 windows: the one-call step equals forward + backward_mse bit for bit, and a repeat gives the same bits (fixed-order slab
    sums, no float atomics) -- as test_generic_ragged_batches_and_step_equals_two_call_sequence does at 256."""
    from morphsym_hgnn_amd import engine as eng
    spec = mi_spec(640, 2, 2)
    e = _generic(spec, dtype)
    B = 300
    x_dict, y, params = helpers.random_case(spec, B, 17)
    xs = e.cast_inputs(x_dict); yd = y.reshape(-1).to(e.device, torch.float32)
    flat = eng.flatten_params(spec, params, e.device)
    out_a = e.forward(xs, flat, B).clone()
    loss_a, g_a = e.backward_mse(xs, flat, out_a, yd, B)
    loss_a, g_a = loss_a.clone(), g_a.clone()
    res = []
    for _ in range(2):
        o, l_, g = e.step_mse(xs, flat, yd, B)
        res.append((o.clone(), l_.clone(), g.clone()))
    torch.cuda.synchronize()
    for o, l_, g in res:
        assert torch.equal(o, out_a) and torch.equal(l_, loss_a) and torch.equal(g, g_a)


def test_two_phase_step_is_refused_on_the_generic_engine():
    """The generic plan has no two-phase gradient split (info.grad_split = -1): mshgnn_step_mse_phase answers EUNSUPPORTED, and the caller's gradient
    buffer is left as it was."""
    from morphsym_hgnn_amd import engine as eng
    spec = mi_spec(384, 1, 2)
    e = _generic(spec, "x3")
    assert int(e.info.grad_split) == -1
    B = 5
    x_dict, y, params = helpers.random_case(spec, B, 2)
    xs = e.cast_inputs(x_dict); yd = y.reshape(-1).to(e.device, torch.float32)
    flat = eng.flatten_params(spec, params, e.device)
    out = torch.empty(B * e.n_out, spec.out_channels, device=e.device); loss = torch.empty(1, device=e.device)
    g = torch.full((spec.flat_size(),), 7.0, device=e.device)
    for phase in (0, 1):
        with pytest.raises(eng.MshgnnError, match="two-phase"):
            e.step_mse_phase(phase, xs, flat, yd, B, out, g, loss)
    torch.cuda.synchronize()
    assert bool((g == 7.0).all())


# ---------------------------------------------------------------------------------------------------
# 2. engine.PaddedEngine: widths off the 128 grid
# ---------------------------------------------------------------------------------------------------
def _padded(spec, dtype):
    from morphsym_hgnn_amd import engine as eng
    e = eng.make_engine(spec, dtype)
    assert isinstance(e, eng.PaddedEngine) and e.inner_spec.hidden == (spec.hidden + 127) // 128 * 128
    assert e.info is not e.inner.info
    return e


def _pad_columns_are_zero(e, spec, B, layers, what):
    """The inner engine's hidden states are exactly 0.0 in every padded feature column (of the nodes its plan computes: the others are never written)."""
    sl = helpers.node_slices(spec)
    liv, need = spec.node_liveness()
    for l in layers:
        x = e.inner.hidden_state(B, l)
        nodes = need[0] if l == 0 else liv[l - 1]
        idx = torch.tensor([n + sl[t].start for t in spec.node_types for n in nodes[t]])
        pad = x[:, idx.to(x.device), spec.hidden:]
        assert bool((pad == 0).all()), f"{what}: X{l} has non-zero padded columns (max {float(pad.abs().max()):.3e})"


def _pgrad_outside_is_zero(e, what):
    """The padded gradient buffer is exactly 0.0 at every position that is not a true parameter's twin (the rows / columns the padding added)."""
    outside = torch.ones(e._pgrad.numel(), dtype=torch.bool, device=e.device)
    outside[e._pad_pos] = False
    bad = e._pgrad[outside]
    assert bool((bad == 0).all()), f"{what}: {int((bad != 0).sum())} padded gradient entries are not zero"


def _grads_zero_where_the_oracle_is(grads, ref, what):
    for k, g in ref["grads"].items():
        z = g == 0
        if bool(z.any()):
            assert bool((grads[k][z] == 0).all()), f"{what}: {k} is non-zero where the oracle's gradient is exactly zero"


def _close(got, ref, tol):
    got, ref = got.detach().double().cpu().reshape(-1), ref.detach().double().cpu().reshape(-1)
    return float((got - ref).abs().max()) <= tol * max(float(ref.abs().max()), 1e-300)


def _grads_close(grads, ref, tol, what):
    for k, g in ref["grads"].items():
        if float(g.abs().max()) == 0.0:
            assert float(grads[k].abs().max()) == 0.0, (what, k)
        else:
            assert _close(grads[k], g, tol), (what, k)


# (hidden, dtype): 1 / 64 / 127 -> the LDS-resident kernels at 128 (f32, bf16; x3 where the split tile fits), 129 / 255 -> 256, 257 / 300 -> 384 (an odd
# NCT, generic), 2000 -> 2048 (the maximum).  (Not bf16 at hidden 1: every weight gradient is then ONE sum of bf16 products that cancels -- a max-abs bound
# relative to that one element measures its conditioning, not the kernel; the padding invariants of the 128-wide bf16 plan are checked at 64 and 127.)
PADDED_CASES = ([(1, "f32"), (1, "x3")] + [(h, dt) for h in (64, 127) for dt in ("f32", "bf16", "x3")]
                + [(129, "x3"), (129, "bf16"), (255, "f32"), (255, "bf16"), (257, "bf16"), (257, "x3"), (300, "x3"), (300, "f32"),
                   (2000, "bf16"), (2000, "x3")])


@pytest.mark.parametrize("hidden,dtype", PADDED_CASES)
def test_padded_width_entry_points_match_the_oracle_at_the_true_width(hidden, dtype):
    """make_engine at a width off the 128 grid, against the oracle of the TRUE-width model: forward (training) + backward, every hidden state (truncated to
    the true width), forward(training=False) == the training forward, backward_mse on the same forward, the one-call step_mse; after each, the padding's
    exact-zero invariants: the inner engine's padded feature columns are 0.0, the padded gradient buffer is 0.0 outside the true parameters' twins, the
    true-layout gradient is 0.0 wherever the oracle's is."""
    from morphsym_hgnn_amd import engine as eng
    spec = mi_spec(hidden, 1, 2)
    e = _padded(spec, dtype)
    if hidden < 128 and dtype != "x3":
        assert not e.generic
    if hidden > 128:
        assert e.generic
    B = 21 if hidden < 1000 else 9
    tol = _tol(dtype)[0]
    what = f"padded h{hidden} {dtype}"
    x_dict, y, params, out, grads = _engine_case(spec, e, dtype, B, 40 + hidden, what)
    ref = helpers.run_engine_case.last_reference
    _pad_columns_are_zero(e, spec, B, range(spec.num_layers + 1), what + " forward")
    _pgrad_outside_is_zero(e, what + " backward")
    _grads_zero_where_the_oracle_is(grads, ref, what + " backward")
    assert e.hidden_state(B, 0).shape[-1] == hidden and e.grad_hidden(B, spec.num_layers).shape[-1] == hidden
    xs = e.cast_inputs(x_dict)
    flat = eng.flatten_params(spec, params, e.device)
    out_inf = e.forward(xs, flat, B, training=False).clone()
    out_tr = e.forward(xs, flat, B, training=True)
    assert torch.equal(out_inf.cpu(), out) and torch.equal(out_tr.cpu(), out)
    yd = y.reshape(-1).to(e.device, torch.float32)
    e._pgrad.fill_(float("nan"))      # (whatever the inner backward does not write would show)
    loss_m, g_m = e.backward_mse(xs, flat, out_tr, yd, B)
    torch.cuda.synchronize()
    assert _close(loss_m, ref["loss"].reshape(1), tol), what
    g_m = eng.unflatten(spec, g_m.cpu())
    _grads_close(g_m, ref, tol, what + " backward_mse")
    _pgrad_outside_is_zero(e, what + " backward_mse")
    _grads_zero_where_the_oracle_is(g_m, ref, what + " backward_mse")
    # the one-call step (its own decisions, its own oracle evaluation)
    x_dict, y, params, out_s, loss_s, g_s = _step_case(spec, e, dtype, B, 40 + hidden, what + " step_mse")
    _pad_columns_are_zero(e, spec, B, range(spec.num_layers), what + " step_mse")
    _pgrad_outside_is_zero(e, what + " step_mse")
    _grads_zero_where_the_oracle_is(g_s, helpers.run_step_case.last_reference, what + " step_mse")


@pytest.mark.parametrize("hidden,dtype", [(96, "f32"), (96, "bf16"), (96, "x3"), (200, "x3"), (200, "bf16")])
def test_padded_classification_matches_the_oracle(hidden, dtype):
    """The K4 classification model at a width off the grid (96 -> 128, 200 -> 256): forward + backward_ce and the one-call step_ce against the oracle at the
    true width; the padded gradient stays 0.0 outside the true parameters' twins."""
    from morphsym_hgnn_amd import engine as eng
    spec = k4_cls_spec(hidden)
    e = _padded(spec, dtype)
    B = 13
    tol = _tol(dtype)[0]
    what = f"padded ce h{hidden} {dtype}"
    x_dict, y, params, out, grads = _engine_case(spec, e, dtype, B, 60 + hidden, what)
    ref = helpers.run_engine_case.last_reference
    xs = e.cast_inputs(x_dict)
    flat = eng.flatten_params(spec, params, e.device)
    out_tr = e.forward(xs, flat, B, training=True)
    loss_c, g_c = e.backward_ce(xs, flat, out_tr, y.reshape(B, -1).to(e.device, torch.int32).contiguous(), B)
    torch.cuda.synchronize()
    assert torch.equal(out_tr.cpu(), out)
    assert _close(loss_c, ref["loss"].reshape(1), tol), what
    g_c = eng.unflatten(spec, g_c.cpu())
    _grads_close(g_c, ref, tol, what + " backward_ce")
    _pgrad_outside_is_zero(e, what + " backward_ce")
    _grads_zero_where_the_oracle_is(g_c, ref, what + " backward_ce")
    _, _, _, _, _, g_s = _step_case(spec, e, dtype, B, 60 + hidden, what + " step_ce")
    _pgrad_outside_is_zero(e, what + " step_ce")
    _grads_zero_where_the_oracle_is(g_s, helpers.run_step_case.last_reference, what + " step_ce")


@pytest.mark.parametrize("hidden,dtype", [(64, "f32"), (300, "x3")])
@pytest.mark.parametrize("B", [1, 17, 333])
def test_padded_ragged_batches_match_the_oracle(hidden, dtype, B):
    """Ragged batches (one window, a 16-window tile and one more, 333: 64- / 128-window tiles with a ragged last one) on a padded LDS-resident width
    (64 -> 128) and a padded generic width (300 -> 384).  (Three limbs: three outputs per window -- one window of a one-foot robot has a single output,
    whose max-abs relative error is that of one cancelling sum.)"""
    spec = mi_spec(hidden, 3, 2)
    e = _padded(spec, dtype)
    _engine_case(spec, e, dtype, B, 7 + B, f"padded h{hidden} {dtype} B={B}")
    _pgrad_outside_is_zero(e, f"padded h{hidden} B={B}")


def test_padded_adam_step_matches_torch_adam():
    """PaddedEngine.adam_step runs on the caller's true-size buffers: three steps of the engine's own gradients against torch.optim.Adam (fp64, CPU), as
    test_adam_step_matches_torch_adam does for Engine."""
    from morphsym_hgnn_amd import engine as eng
    spec = mi_spec(96, 1, 2)
    e = _padded(spec, "f32")
    B = 5
    x_dict, y, params = helpers.random_case(spec, B, 3)
    xs = e.cast_inputs(x_dict)
    flat = eng.flatten_params(spec, params, e.device)
    assert flat.numel() == spec.flat_size()
    m = torch.zeros_like(flat); v = torch.zeros_like(flat)
    ref = flat.detach().cpu().double().clone().requires_grad_(True)
    opt = torch.optim.Adam([ref], lr=1e-3)
    yd = y.reshape(-1).to(e.device, torch.float32)
    for step in range(1, 4):
        out = e.forward(xs, flat, B)
        _, g = e.backward_mse(xs, flat, out, yd, B)
        ref.grad = g.detach().cpu().double()
        opt.step()
        e.adam_step(flat, g, m, v, step, lr=1e-3)
        torch.cuda.synchronize()
        delta = float((ref.detach() - flat.cpu().double()).abs().max())
        assert delta < 2e-6, (step, delta)


def test_width_above_the_generic_range_is_refused_before_anything_runs():
    """hidden 2049 pads to 2176, which no engine takes: make_engine fails loudly, naming the accepted range, and allocates nothing on the device."""
    from morphsym_hgnn_amd import engine as eng
    spec = mi_spec(2049, 1, 2)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    with pytest.raises(eng.MshgnnError, match=r"128\.\.2048"):
        eng.make_engine(spec, "bf16")
    assert torch.cuda.memory_allocated() == before


# ---------------------------------------------------------------------------------------------------
# 3. PaddedEngine.step_mse_phase: the two-phase contract in the true layout
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "f32", "x3"])
def test_padded_two_phase_step_keeps_the_contract(dtype):
    """A1-C2 at hidden 96 (-> 128, the plans with a two-phase step): info.grad_split is the TRUE layout's first non-encoder offset; after phase 0
    grad_flat[split:], the loss and the output equal the one-call step bit for bit and grad_flat[:split] is untouched; what the caller writes into
    grad_flat[split:] between the phases (its all-reduce) survives phase 1; with that write undone the whole buffer equals the one-call step."""
    from morphsym_hgnn_amd import engine as eng, synth
    spec = helpers.make_spec("c2", "a1-c2", "a1-c2", 96, 3)
    e = eng.make_engine(spec, dtype)
    assert isinstance(e, eng.PaddedEngine) and not e.generic
    offs = spec.param_offsets()
    split = min(o for k, (o, n) in offs.items() if not k.startswith("encoder."))
    assert split == offs["convs.0.convs.<base___front_bj___joint>.lin_rel.weight"][0]
    B = 333
    x_dict, y = synth.make_windows(5, B, spec.num_nodes, spec.widths, 12)
    xs = e.cast_inputs(x_dict)
    yd = y.reshape(-1).to(e.device, torch.float32)
    flat = eng.flatten_params(spec, synth.make_params(5, spec.param_shapes()), e.device)
    out_a, loss_a, g_a = e.step_mse(xs, flat, yd, B)
    out_a, loss_a, g_a = out_a.clone(), loss_a.clone(), g_a.clone()
    out_b = torch.empty_like(out_a); loss_b = torch.empty(1, device=e.device); g_b = torch.full_like(g_a, float("nan"))
    e.step_mse_phase(0, xs, flat, yd, B, out_b, g_b, loss_b)
    torch.cuda.synchronize()
    assert torch.equal(g_b[split:], g_a[split:]) and torch.equal(loss_b, loss_a) and torch.equal(out_b, out_a)
    assert bool(torch.isnan(g_b[:split]).all())           # the encoder's slice is untouched until phase 1
    reduced = g_b[split:] * 0.5 + 1.0                      # (stands in for the all-reduce of the first region)
    g_b[split:] = reduced
    e.step_mse_phase(1, xs, flat, yd, B, out_b, g_b, loss_b)
    torch.cuda.synchronize()
    assert torch.equal(g_b[split:], reduced)
    g_b[split:] = g_a[split:]
    assert torch.equal(g_b, g_a)
    # where callers read the split: info in the TRUE layout, a copy of the inner plan's summary (whose split is in padded coordinates)
    assert int(e.info.grad_split) == split and e.info is not e.inner.info and int(e.inner.info.grad_split) > split
