"""Evaluation straight from a resident sequence (mshgnn_forward_series, Engine.forward_series, models.forward_windows, the wrappers' evaluation steps):
every comparison is torch.equal against the yardstick `store.assemble(starts)` + `Engine.forward(..., training=False)`, both pinned to the oracle and the
reference by tests/test_windows.py and the golden cases.  Standardised recipes (normalize=True) included: the encoder standardises the fp32 series itself
with the assembly kernel's own arithmetic (one shared device function).

The Solo centroidal-momentum recipes are left out: their windows are 1 (or 5) steps long with several runs per node row, and the series encoders take a
chunk's 8 elements from at most two runs -- mshgnn_forward_series refuses such recipes (checked below), the wrappers assemble them as before."""
import types

import numpy as np
import pytest
import torch

from oracle import window_oracle as wo
from tests import helpers
from tests import test_windows as tw

pytestmark = pytest.mark.gpu
T = tw.T
CONST_ROWS = (100, 300)      # rows over which one column per series below is constant: windows starting in [100, 150] see a constant run
CONST_START = 120


def _sequence(name, constant=False):
    """The synthetic sequences of tests/test_windows.py; constant=True: a copy with one joint column and one base column constant over CONST_ROWS."""
    if name.startswith("a1c2"):
        seq, n = {k: np.array(v) for k, v in tw.SEQ.items()}, tw.N
    else:
        seq, n = {k: np.array(v) for k, v in tw.SEQ4.items()}, int(tw.FX4["N"])
    if constant:
        seq["q"][CONST_ROWS[0]:CONST_ROWS[1], 4] = 0.515625
        seq["imu_omega"][CONST_ROWS[0]:CONST_ROWS[1], 1] = -3.0
    return seq, n


def _model(name, normalize=False):
    from morphsym_hgnn_amd.windows import quadsdk_a1_c2_recipe, minicheetah_k4_recipe
    if name == "a1c2_L3":        # compile-time program A1C2_L3; body-frame labels: label_rotate and the quaternion by-product
        return quadsdk_a1_c2_recipe(tw.JP, tw.FP, T, 3, body_frame_labels=True, normalize=normalize), helpers.make_spec("c2", "a1-c2", "a1-c2", 128, 3)
    if name == "a1c2_L2":        # interpreted
        return quadsdk_a1_c2_recipe(tw.JP, tw.FP, T, 3, normalize=normalize), helpers.make_spec("c2", "a1-c2", "a1-c2", 128, 2)
    return minicheetah_k4_recipe(tw.JP, tw.FP, T, normalize), helpers.make_spec("k4", "mini_cheetah-k4", "mini_cheetah-k4", 128, 3, regression=False)


def _starts(n, B, force=()):
    st = torch.randint(0, n - T + 1, (B,), generator=torch.Generator().manual_seed(B))
    st[0], st[-1] = 0, n - T
    for i, s in enumerate(force):
        st[1 + i] = s
    return st.cuda()


def _setup(name, plan, normalize=False, constant=False):
    from morphsym_hgnn_amd import engine as eng, synth
    from morphsym_hgnn_amd.windows import SequenceStore
    recipe, spec = _model(name, normalize)
    seq, n = _sequence(name, constant)
    store = SequenceStore(seq, recipe, dtype=plan)
    e = eng.Engine(spec, plan)
    assert not e.generic
    flat = eng.flatten_params(spec, synth.make_params(8, spec.param_shapes()), e.device)
    return recipe, spec, seq, n, store, e, flat


def _yardstick(store, e, flat, starts):
    B = int(starts.numel())
    xs, y, q = store.assemble(starts)
    out = e.forward(xs, flat, B, training=False).clone()
    return xs, (y.clone() if y is not None else None), (q.clone() if q is not None else None), out


CASES = [(m, B) for m in ("a1c2_L3", "a1c2_L2", "mck4_cls") for B in (3, 130, 1000)] + [("a1c2_L3", 8192), ("a1c2_L2", 8192)]


@pytest.mark.parametrize("plan", ["bf16", "x3"])
@pytest.mark.parametrize("name,B", CASES)
def test_forward_series_is_bit_identical_to_assemble_then_forward(name, B, plan):
    recipe, spec, seq, n, store, e, flat = _setup(name, plan)
    if name == "a1c2_L3" and plan == "bf16":
        assert e.specialised == "A1C2_L3"   # the stack launch runs the compile-time program, as mshgnn_forward(training = 0) does
    if name == "a1c2_L2":
        assert e.specialised == ""
    starts = _starts(n, B)
    _, y_a, q_a, out_a = _yardstick(store, e, flat, starts)
    n_ws = len(e._ws)
    y, q, li, out = e.forward_series(store, starts, flat)
    torch.cuda.synchronize()
    assert (B, 0) in e._ws and (B, 1) not in e._ws and len(e._ws) == n_ws      # the evaluation workspace, no other
    assert B not in store._cache                                               # ... and no window buffers
    assert torch.equal(out, out_a) and torch.equal(y, y_a)
    if recipe.quat_series:
        assert torch.equal(q, q_a)
    else:
        assert q is None
    if spec.regression:
        assert li is None
    else:
        assert li.dtype == torch.int32 and torch.equal(li, (y_a != 0).to(torch.int32).reshape(B, 4))
        assert 0 < int(li.sum()) < li.numel()
    # a sequence without labels: no by-products, the same output
    out_a2 = out.clone()
    y2, q2, li2, out2 = e.forward_series(store, starts, flat, labels=False)
    torch.cuda.synchronize()
    assert y2 is None and q2 is None and li2 is None and torch.equal(out2, out_a2)
    assert store.desc.run_ptrs_ready == 1      # later calls on the same stream vouch for the run pointers


@pytest.mark.parametrize("plan", ["bf16", "x3"])
@pytest.mark.parametrize("name", ["a1c2_L3", "mck4_cls"])
@pytest.mark.parametrize("B", [3, 130, 1000])
def test_standardised_forward_series_is_bit_identical_to_assemble_then_forward(name, B, plan):
    """normalize=True: the encoder standardises every run over its window.  Not vacuous: the series hold a column that is constant over a sampled
    window (checked on the CPU with the oracle's window function first), the assembled windows hold the zeros of the NaN -> 0 branch, and the
    standardised output differs from the unstandardised one."""
    seq, n = _sequence(name, constant=True)
    if name.startswith("a1c2"):
        w = wo.a1_c2_window(seq, CONST_START, T, tw.JP, tw.FP, 3, False, True)
    else:
        w = wo.minicheetah_k4_window(seq, CONST_START, T, tw.JP, tw.FP, True)
    jrow = int(np.where(np.asarray(tw.JP) == 4)[0][0])      # the joint node that reads column 4 of q; its first run is q
    assert not np.asarray(w[1])[jrow, :T].any() and np.asarray(w[1])[jrow, T:2 * T].any()
    assert not np.asarray(w[0])[0, 4 * T:5 * T].any()       # imu_omega column 1 of the base rows
    recipe, spec, seq, n, store, e, flat = _setup(name, plan, normalize=True, constant=True)
    starts = _starts(n, B, force=(CONST_START,))
    xs, y_a, q_a, out_a = _yardstick(store, e, flat, starts)
    nj = recipe.num_nodes["joint"]
    assert not xs[1][1 * nj + jrow, :T].float().any() and xs[1][1 * nj + jrow, T:2 * T].float().any()      # window 1 = CONST_START: the zeros are there
    y, q, li, out = e.forward_series(store, starts, flat)
    torch.cuda.synchronize()
    assert torch.equal(out, out_a) and torch.equal(y, y_a)
    assert torch.isfinite(out).all()
    # the same starts, unstandardised: another output
    _, _, _, _, store_u, e_u, _ = _setup(name, plan, normalize=False, constant=True)
    out_u = e_u.forward_series(store_u, starts, flat)[3]
    assert not torch.equal(out_u, out)


@pytest.mark.parametrize("plan", ["bf16", "x3"])
def test_forward_series_leaves_a_pending_training_stash_alone(plan):
    """A training forward, then forward_series (on the evaluation workspace), then the backward of the first: the first's gradients."""
    recipe, spec, seq, n, store, e, flat = _setup("a1c2_L3", plan)
    B = 130
    starts = _starts(n, B)
    xs, _, _ = store.assemble(starts)
    xs = [x.clone() for x in xs]
    gout = torch.randn(B * e.n_out, spec.out_channels, generator=torch.Generator().manual_seed(1)).cuda()
    e.forward(xs, flat, B, training=True)
    g_ref = e.backward(xs, flat, gout, B).clone()
    e.forward(xs, flat, B, training=True)
    other = _starts(n, B).flip(0).contiguous()
    out = e.forward_series(store, other, flat)[3]
    g = e.backward(xs, flat, gout, B)
    torch.cuda.synchronize()
    assert torch.equal(g, g_ref)
    assert torch.equal(out, _yardstick(store, e, flat, other)[3])


def test_forward_series_refuses_what_it_cannot_run(monkeypatch):
    from morphsym_hgnn_amd import engine as eng, synth
    from morphsym_hgnn_amd.windows import SequenceStore, quadsdk_a1_c2_recipe, minicheetah_k4_recipe, solo_com_recipe, solo_com_arrays
    spec = helpers.make_spec("c2", "a1-c2", "a1-c2", 128, 2)
    starts = torch.tensor([0, 5, 9], dtype=torch.int64).cuda()
    for dtype, seq, recipe, match in (("f32", tw.SEQ, quadsdk_a1_c2_recipe(tw.JP, tw.FP, T, 3), "bf16 plan"),
                                      ("bf16", tw.SEQ, quadsdk_a1_c2_recipe(tw.JP, tw.FP, T, 1), "label count"),
                                      ("x3", tw.SEQ, quadsdk_a1_c2_recipe(tw.JP, tw.FP, T, 1), "label count"),
                                      ("bf16", tw.SEQ4, minicheetah_k4_recipe(tw.JP, tw.FP, T), "node type"),
                                      ("bf16", tw.SEQ, quadsdk_a1_c2_recipe(tw.JP, tw.FP, 1, 3, normalize=True), "history must be >= 2"),
                                      ("x3", tw.SEQ, quadsdk_a1_c2_recipe(tw.JP, tw.FP, 1, 3, normalize=True), "history must be >= 2")):
        e = eng.Engine(spec, dtype)
        store = SequenceStore(seq, recipe, dtype=dtype)
        flat = eng.flatten_params(spec, synth.make_params(1, spec.param_shapes()), e.device)
        with pytest.raises(eng.MshgnnError, match=match):
            e.forward_series(store, starts, flat)
    # windows shorter than a chunk with several runs per node row (the Solo centroidal-momentum recipes): refused, not gathered wrongly
    cspec = helpers.make_spec("k4_com", "solo-k4-com", "solo-k4", 128, 2)
    e = eng.Engine(cspec, "bf16")
    store = SequenceStore(solo_com_arrays(tw.SEQS["X"], tw.SEQS["Y"]), solo_com_recipe("k4_com", tw.JP, 1), dtype="bf16")
    with pytest.raises(eng.MshgnnError, match="history >= 8"):
        e.forward_series(store, starts, eng.flatten_params(cspec, synth.make_params(1, cspec.param_shapes()), e.device))
    # the training entry point keeps refusing standardised recipes (tests/test_windows.py pins it; restated here)
    e = eng.Engine(spec, "bf16")
    store = SequenceStore(tw.SEQ, quadsdk_a1_c2_recipe(tw.JP, tw.FP, T, 3, normalize=True), dtype="bf16")
    flat = eng.flatten_params(spec, synth.make_params(1, spec.param_shapes()), e.device)
    with pytest.raises(eng.MshgnnError, match="unstandardised"):
        e.step_mse_series(store, starts, flat)
    # the generic-width engine
    monkeypatch.setenv("MSHGNN_ENGINE", "generic")
    e = eng.Engine(spec, "bf16")
    assert e.generic
    store = SequenceStore(tw.SEQ, quadsdk_a1_c2_recipe(tw.JP, tw.FP, T, 3), dtype="bf16")
    with pytest.raises(eng.MshgnnError, match="bf16 plan"):
        e.forward_series(store, starts, flat)


@pytest.mark.parametrize("normalize", [False, True])
def test_forward_series_in_a_hip_graph_replays_on_new_starts(normalize):
    """One call captured and replayed on new `starts` contents gives the eager result: no host-side state changes per call but run_ptrs_ready."""
    recipe, spec, seq, n, store, e, flat = _setup("a1c2_L3", "bf16", normalize=normalize, constant=normalize)
    B = 130
    st_a, st_b = _starts(n, B, force=(CONST_START,)), _starts(n, B).flip(0).contiguous()
    want_a, want_b = _yardstick(store, e, flat, st_a)[3], _yardstick(store, e, flat, st_b)[3]
    static = st_a.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = e.forward_series(store, static, flat)[3]      # warm-up on the capture stream: buffers, workspace
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            e.forward_series(store, static, flat, out=out)
    torch.cuda.current_stream().wait_stream(side)
    g.replay(); torch.cuda.synchronize()
    assert torch.equal(out, want_a)
    static.copy_(st_b)
    g.replay(); torch.cuda.synchronize()
    assert torch.equal(out, want_b)


def _wrapper(kind, plan, normalize):
    import os
    from morphsym_hgnn_amd import wrappers
    from morphsym_hgnn_amd.windows import SequenceStore, quadsdk_a1_c2_recipe, minicheetah_k4_recipe
    dev = torch.device("cuda")
    torch.set_default_dtype(torch.float32)
    if kind == "a1c2_regression":
        (seq, n), recipe = _sequence("a1c2", normalize), quadsdk_a1_c2_recipe(tw.JP, tw.FP, T, 3, normalize=normalize)
        spec = helpers.make_spec("c2", "a1-c2", "a1-c2", 128, 2)
        _, cfg = helpers.load_group("a1-c2")
        make = lambda dummy: wrappers.HGNN_C2_Lightning_Reg(128, 2, spec.topology.metadata(), dummy, symmetry_mode="MorphSym", group_operator_path=cfg)
    else:
        (seq, n), recipe = _sequence("mck4", normalize), minicheetah_k4_recipe(tw.JP, tw.FP, T, normalize)
        spec = helpers.make_spec("k4", "mini_cheetah-k4", "mini_cheetah-k4", 128, 2, regression=False)
        _, cfg = helpers.load_group("mini_cheetah-k4")
        make = lambda dummy: wrappers.HGNN_K4_Lightning(128, 2, spec.topology.metadata(), dummy, regression=False, symmetry_mode="MorphSym",
                                                        group_operator_path=cfg)
    store = SequenceStore(seq, recipe, dtype=plan)
    xs, _, _ = store.assemble([0, 1])
    dummy = types.SimpleNamespace(edge_index_dict=spec.topology.edge_index_dict(2, device=dev),
                                  x_dict={t: x[:, :recipe.width(t)].float().contiguous() for t, x in zip(recipe.node_types, xs)})
    prev = os.environ.get("MSHGNN_DTYPE")
    os.environ["MSHGNN_DTYPE"] = plan
    try:
        torch.manual_seed(3)
        w = make(dummy).to(dev)
    finally:
        os.environ.pop("MSHGNN_DTYPE", None) if prev is None else os.environ.__setitem__("MSHGNN_DTYPE", prev)
    return w, store, spec, n, dev


@pytest.mark.parametrize("kind,plan,normalize", [("a1c2_regression", "bf16", False), ("a1c2_regression", "x3", True), ("mck4_classification", "bf16", True),
                                                 ("mck4_classification", "x3", False)])
def test_wrapper_evaluation_epochs_match_the_assembled_route(kind, plan, normalize):
    """A validation and a test epoch over WindowBatches (two full batches and a ragged one): metric sums and logged values are the bits of the same
    epochs with fused_evaluation_step = False; after a fused step the batch holds no materialised windows, and batch.y is there."""
    w, store, spec, n, dev = _wrapper(kind, plan, normalize)
    all_starts = _starts(n, 96 + 96 + 37, force=(CONST_START,))
    batches = [all_starts[0:96], all_starts[96:192], all_starts[192:]]
    eis = {B: spec.topology.edge_index_dict(B, device=dev) for B in (96, 37)}

    def epoch(which, fused):
        w.fused_evaluation_step = fused
        state = []
        with torch.no_grad():
            getattr(w, f"on_{which}_epoch_start")()
            for i, st in enumerate(batches):
                wb = store.batch(st, eis[int(st.numel())])
                loss = getattr(w, f"{which}_step")(wb, i)
                assert (wb._x is None) == fused          # fused: nothing was assembled
                y_ref = store.assemble(st)[1]
                assert torch.equal(wb.y, y_ref)
                state.append(loss.detach().clone())
            getattr(w, f"on_{which}_epoch_end")()
        torch.cuda.synchronize()
        return state, {k: torch.as_tensor(v).detach().clone() for k, v in w.logged.items() if k.startswith(which[:3]) and v is not None}

    for which in ("validation", "test"):
        losses_f, logged_f = epoch(which, True)
        losses_a, logged_a = epoch(which, False)
        assert len(logged_f) > 0 and logged_f.keys() == logged_a.keys()
        for a, b in zip(losses_f, losses_a):
            assert torch.equal(a, b)
        for k in logged_f:
            assert torch.equal(logged_f[k], logged_a[k]), k


@pytest.mark.parametrize("normalize", [False, True])
def test_evaluate_sequence_equals_stacked_yardstick_outputs(normalize):
    from morphsym_hgnn_amd import wrappers
    w, store, spec, n, dev = _wrapper("a1c2_regression", "bf16", normalize)
    ei1 = spec.topology.edge_index_dict(1, device=dev)
    stride, bs = 3, 32
    pred = wrappers.evaluate_sequence(w, store, ei1, bs, stride=stride)
    starts = torch.arange(0, len(store), stride, device=dev)
    assert pred.shape[0] == starts.numel() and starts.numel() % bs != 0      # a ragged last batch
    e = next(iter(w.model._engines.values()))
    flat = w.model._flat_params(dev)
    want = torch.cat([_yardstick(store, e, flat, starts[lo:lo + bs])[3].reshape(-1, 12) for lo in range(0, starts.numel(), bs)])
    assert torch.equal(pred, want)
    assert any(k.startswith("test_") for k in w.logged)
