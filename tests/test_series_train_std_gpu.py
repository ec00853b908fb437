"""Training straight from a resident sequence on STANDARDISED windows (mshgnn_step_mse_series_std / mshgnn_step_ce_series_std, Engine.step_mse_series_std /
step_ce_series_std, models.fused_training_step_windows on a normalize=True recipe): every comparison is torch.equal against the yardstick
`store.assemble(starts)` + `Engine.step_mse` / `step_ce`, which tests/test_windows.py and the golden cases pin to the oracle and the reference.

The sequences are those of tests/test_windows.py with one joint column and one base column held constant over a stretch (tests/test_series_eval_gpu.py,
constant=True), so that a sampled window meets the sd = 0 -> 0 branch of the standardisation."""
import ctypes as C
import types

import pytest
import torch

from tests import helpers
from tests import test_series_eval_gpu as se
from tests import test_windows as tw

pytestmark = pytest.mark.gpu
T = tw.T
CONST_START = se.CONST_START


def _model(name, normalize):
    from morphsym_hgnn_amd.windows import quadsdk_a1_c2_recipe, minicheetah_k4_recipe
    if name.startswith("a1c2"):
        return (quadsdk_a1_c2_recipe(tw.JP, tw.FP, T, 3, body_frame_labels=name.endswith("body"), normalize=normalize),
                helpers.make_spec("c2", "a1-c2", "a1-c2", 128, 3))
    return minicheetah_k4_recipe(tw.JP, tw.FP, T, normalize), helpers.make_spec("k4", "mini_cheetah-k4", "mini_cheetah-k4", 128, 2, regression=False)


def _setup(name, plan, normalize=True):
    from morphsym_hgnn_amd import engine as eng, synth
    from morphsym_hgnn_amd.windows import SequenceStore
    recipe, spec = _model(name, normalize)
    seq, n = se._sequence(name, constant=True)
    store = SequenceStore(seq, recipe, dtype=plan)
    e = eng.Engine(spec, plan)
    assert not e.generic
    flat = eng.flatten_params(spec, synth.make_params(8, spec.param_shapes()), e.device)
    return recipe, spec, n, store, e, flat


def _yardstick(store, e, spec, flat, starts):
    """assemble + step_mse / step_ce on fresh tensors: (xs, y, q, labels | None, out, loss, grad), all the caller's own copies"""
    B = int(starts.numel())
    xs, y, q = store.assemble(starts)
    xs = [x.clone() for x in xs]; y = y.clone(); q = q.clone() if q is not None else None
    if spec.regression:
        lab = None
        out, loss, g = e.step_mse(xs, flat, y.reshape(-1), B)
    else:
        lab = (y != 0).to(torch.int32).reshape(B, 4).contiguous()
        out, loss, g = e.step_ce(xs, flat, lab, B)
    return xs, y, q, lab, out.clone(), loss.clone(), g.clone()


def _poison(store, B):
    """NaN in every feature column of the store's window buffers, zero in the pad columns: the fused step rewrites the former and leaves the latter zero"""
    for x, t in zip(store._buffers(B)[0], store.recipe.node_types):
        x.fill_(float("nan"))
        x[:, store.recipe.width(t):] = 0


def _check_step(store, e, spec, starts, want, got):
    B = int(starts.numel())
    xs_a, y_a, q_a, lab_a, out_a, loss_a, g_a = want
    xs, second, out, loss, g = got
    torch.cuda.synchronize()
    assert len(xs) == len(xs_a)
    for a, b in zip(xs_a, xs):
        assert torch.equal(a, b)
    _, y, q = store._buffers(B)
    assert torch.equal(y, y_a)
    if spec.regression:
        assert second is y
        if store.recipe.quat_series:
            assert torch.equal(q, q_a)
    else:
        assert second.dtype == torch.int32 and torch.equal(second, lab_a) and 0 < int(lab_a.sum()) < lab_a.numel()
    assert torch.equal(out, out_a) and torch.equal(loss, loss_a) and torch.equal(g, g_a)
    assert torch.isfinite(out).all() and torch.isfinite(g).all()


CASES = [("a1c2", B) for B in (3, 37, 1000)] + [("a1c2_body", 64)] + [("mck4_cls", B) for B in (3, 130)]


@pytest.mark.parametrize("plan", ["bf16", "x3"])
@pytest.mark.parametrize("name,B", CASES)
def test_standardised_series_step_is_bit_identical_to_assemble_then_step(name, B, plan):
    """The materialised windows, labels / contact flags / quaternion, outputs, loss and the whole flat gradient are the bits of assembly + step.  Not vacuous:
    window 1 starts at CONST_START, its constant runs are the zeros of the sd = 0 branch, and the unstandardised step on the same starts gives other bits."""
    recipe, spec, n, store, e, flat = _setup(name, plan)
    starts = se._starts(n, B, force=(CONST_START,))
    assert int(starts[0]) == 0 and int(starts[-1]) == n - T
    want = _yardstick(store, e, spec, flat, starts)
    nj = recipe.num_nodes["joint"]
    jrow = int((torch.as_tensor(tw.JP) == 4).nonzero()[0, 0])      # the joint node that reads column 4 of q; its first run is q
    assert not want[0][1][1 * nj + jrow, :T].float().any() and want[0][1][1 * nj + jrow, T:2 * T].float().any()
    _poison(store, B)
    step = e.step_mse_series_std if spec.regression else e.step_ce_series_std
    got = step(store, starts, flat)
    assert store.desc.run_ptrs_ready == 0      # the first step of a store resolves the runs' column pointers
    _check_step(store, e, spec, starts, want, got)
    # the same starts, unstandardised: other windows, another output, another gradient
    _, _, _, store_u, e_u, _ = _setup(name, plan, normalize=False)
    xs_u, _, out_u, _, g_u = (e_u.step_mse_series if spec.regression else e_u.step_ce_series)(store_u, starts, flat)
    torch.cuda.synchronize()
    assert not torch.equal(xs_u[1], want[0][1]) and not torch.equal(out_u, want[4]) and not torch.equal(g_u, want[6])


@pytest.mark.parametrize("plan", ["bf16", "x3"])
@pytest.mark.parametrize("name", ["a1c2", "mck4_cls"])
def test_second_standardised_step_vouches_for_the_run_pointers(name, plan):
    """A second step on the same store and stream, other starts, run_ptrs_ready == 1 (no pointer launch): the bits of its own assembled yardstick."""
    recipe, spec, n, store, e, flat = _setup(name, plan)
    B = 130
    st_a, st_b = se._starts(n, B, force=(CONST_START,)), se._starts(n, B, force=(CONST_START + 7,)).flip(0).contiguous()
    want_a, want_b = _yardstick(store, e, spec, flat, st_a), _yardstick(store, e, spec, flat, st_b)
    assert not torch.equal(want_a[4], want_b[4])
    step = e.step_mse_series_std if spec.regression else e.step_ce_series_std
    _poison(store, B)
    got = step(store, st_a, flat)
    assert store.desc.run_ptrs_ready == 0
    _check_step(store, e, spec, st_a, want_a, got)
    _poison(store, B)
    got = step(store, st_b, flat)
    assert store.desc.run_ptrs_ready == 1
    _check_step(store, e, spec, st_b, want_b, got)


@pytest.mark.parametrize("plan", ["bf16", "x3"])
def test_standardised_series_step_in_a_hip_graph_replays_on_new_starts(plan):
    """One step captured and replayed on new `starts` contents gives the eager step: no host-side state changes per call but run_ptrs_ready."""
    recipe, spec, n, store, e, flat = _setup("a1c2", plan)
    B = 130
    st_a, st_b = se._starts(n, B, force=(CONST_START,)), se._starts(n, B).flip(0).contiguous()
    want_a, want_b = _yardstick(store, e, spec, flat, st_a), _yardstick(store, e, spec, flat, st_b)
    static = st_a.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        xs, y, out, loss, g = e.step_mse_series_std(store, static, flat)      # warm-up on the capture stream: buffers, workspace, run pointers
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            e.step_mse_series_std(store, static, flat, out=out, grad_flat=g, loss=loss)
    torch.cuda.current_stream().wait_stream(side)
    for st, want in ((st_a, want_a), (st_b, want_b)):
        static.copy_(st)
        _poison(store, B)
        out.fill_(float("nan")); g.fill_(float("nan")); loss.fill_(float("nan"))
        graph.replay()
        _check_step(store, e, spec, st, want, (xs, y, out, loss, g))


@pytest.mark.parametrize("kind,plan", [("mck4_classification", "bf16"), ("mck4_classification", "x3"), ("a1c2_regression", "x3"), ("a1c2_regression", "bf16")])
def test_wrapper_training_step_on_standardised_windows_matches_the_assembled_batch(kind, plan, monkeypatch):
    """HGNN_K4_Lightning (classification) and HGNN_C2_Lightning_Reg on normalize=True recipes: training_step(WindowBatch) + backward() = the same on the
    assembled plain batch (loss, every parameter gradient, batch.y).  The fused route is proven by making store.assemble raise during the call; with
    fused_training_step = False the batch is assembled and the results are those of the plain batch under the same setting."""
    w, store, spec, n, dev = se._wrapper(kind, plan, True)
    recipe = store.recipe
    assert recipe.normalize
    B = 96
    starts = se._starts(n, B, force=(CONST_START,))
    ei = spec.topology.edge_index_dict(B, device=dev)
    xs, y, _ = store.assemble(starts)
    plain = types.SimpleNamespace(x_dict={t: x.clone() for t, x in zip(recipe.node_types, xs)}, edge_index_dict=ei, y=y.clone(), batch_size=B)
    params = list(w.model.parameters())

    def run(batch, i):
        w.model.zero_grad()
        loss = w.training_step(batch, i)
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach().clone(), w.model._gflat.clone(), [p.grad.clone() for p in params]

    loss_a, flat_a, grads_a = run(plain, 0)
    assert bool(flat_a.any()) and any(bool(g.any()) for g in grads_a)

    def same(got):
        assert torch.equal(got[0], loss_a) and torch.equal(got[1], flat_a)
        assert len(got[2]) == len(grads_a) and all(torch.equal(a, b) for a, b in zip(got[2], grads_a))

    real_assemble = store.assemble

    def refuse(*a, **k):
        raise AssertionError("the fused route assembles nothing")
    monkeypatch.setattr(store, "assemble", refuse)
    wb = store.batch(starts, ei)
    assert wb._x is None
    got = run(wb, 1)
    assert wb._x is not None and torch.equal(wb.y, y)      # the step left the standardised windows and the labels on the batch
    for t in recipe.node_types:
        assert torch.equal(wb.x_dict[t], plain.x_dict[t])
    same(got)
    # fused_training_step = False switches the whole route off: the batch is assembled
    calls = []
    monkeypatch.setattr(store, "assemble", lambda *a, **k: (calls.append(1), real_assemble(*a, **k))[1])
    w.fused_training_step = False
    wb = store.batch(starts, ei)
    got = run(wb, 2)
    assert calls and torch.equal(wb.y, y)
    loss_a, flat_a, grads_a = run(plain, 3)      # (the two-call route takes its loss from torch: its own yardstick on the plain batch)
    same(got)


def _sentinels(store, e, B):
    """Distinct values in everything a launch of the step would write: window buffers, labels, statistics, outputs, loss, gradient"""
    xs, y, q = store._buffers(B)
    out, g, loss = e._results(B, None, None, None)
    bufs = list(xs) + [y, out, g, loss] + ([q] if q is not None else [])
    stats = store._stats_buffer(B)
    if stats is not None:
        bufs.append(stats)
    for b in bufs:
        b.fill_(-7.0)
    torch.cuda.synchronize()
    return bufs, out, g, loss


def test_standardised_series_steps_refuse_what_they_cannot_run(monkeypatch):
    """Every refusal of the new entry points, made before anything is launched: nothing the step writes has changed afterwards."""
    from morphsym_hgnn_amd import engine as eng, synth, topology
    from morphsym_hgnn_amd.spec import ModelSpec
    from morphsym_hgnn_amd.windows import SequenceStore, quadsdk_a1_c2_recipe, minicheetah_k4_recipe
    spec = helpers.make_spec("c2", "a1-c2", "a1-c2", 128, 2)
    starts = torch.tensor([0, 5, 9], dtype=torch.int64).cuda()
    B = 3

    def refused(e, store, code, match, ce=False):
        flat = eng.flatten_params(e.spec, synth.make_params(1, e.spec.param_shapes()), e.device)
        bufs, out, g, loss = _sentinels(store, e, B)
        with pytest.raises(eng.MshgnnError, match=match) as err:
            (e.step_ce_series_std if ce else e.step_mse_series_std)(store, starts, flat, out=out, grad_flat=g, loss=loss)
        assert f"failed ({code})" in str(err.value)
        torch.cuda.synchronize()
        for b in bufs:
            assert bool((b == -7.0).all())

    a1 = lambda **k: quadsdk_a1_c2_recipe(tw.JP, tw.FP, k.pop("history", T), k.pop("grf", 3), **k)
    EINVAL, EUNSUPPORTED = -1, -2
    e16, e3 = eng.Engine(spec, "bf16"), eng.Engine(spec, "x3")
    for e, plan in ((e16, "bf16"), (e3, "x3")):
        # an unstandardised descriptor: the plain entry points are named
        refused(e, SequenceStore(tw.SEQ, a1(), dtype=plan), EINVAL, "unstandardised; use mshgnn_step_mse_series / mshgnn_step_ce_series")
        refused(e, SequenceStore(tw.SEQ, a1(history=1, normalize=True), dtype=plan), EINVAL, "history must be >= 2")
        refused(e, SequenceStore(tw.SEQ, a1(history=257, normalize=True), dtype=plan), EUNSUPPORTED, "longer than 256")
        refused(e, SequenceStore(tw.SEQ, a1(grf=1, normalize=True), dtype=plan), EINVAL, "label count")
        # the stats scratch: missing, misaligned
        store = SequenceStore(tw.SEQ, a1(normalize=True), dtype=plan)
        whole = torch.empty(2 * int(store.desc.n_runs) * B + 2, dtype=torch.float64, device="cuda")
        for stats, match in ((None, "needs the stats scratch"), (whole[1:], "16-byte aligned")):
            assert stats is None or stats.data_ptr() % 16 == 8
            with monkeypatch.context() as m:
                m.setattr(store, "_stats_buffer", lambda B_, s=stats: s)
                refused(e, store, EINVAL, match)
    # the label description, as the plain entry points check it: rotation needs a quaternion source
    r = a1(normalize=True, body_frame_labels=True)
    r.quat_series = None
    refused(e16, SequenceStore(tw.SEQ, r, dtype="bf16"), EINVAL, "label rotation")
    # the fp32 plan and the generic-width engine
    refused(eng.Engine(spec, "f32"), SequenceStore(tw.SEQ, a1(normalize=True), dtype="f32"), EUNSUPPORTED, "bf16 plan")
    with monkeypatch.context() as m:
        m.setenv("MSHGNN_ENGINE", "generic")
        eg = eng.Engine(spec, "bf16")
        assert eg.generic
        refused(eg, SequenceStore(tw.SEQ, a1(normalize=True), dtype="bf16"), EUNSUPPORTED, "bf16 plan")
    # windows shorter than a chunk with node rows of several runs (5 steps; the base row has 6 runs)
    r5 = a1(history=5, normalize=True, n_base=1)
    spec5 = ModelSpec(kind="mi", topology=topology.TOPOLOGIES["quadruped-mi"](), hidden=128, num_layers=2, widths={t: r5.width(t) for t in r5.node_types},
                      regression=True, grf_dimension=3, group=None, num_timesteps=5)
    for plan in ("bf16", "x3"):
        store5 = SequenceStore(tw.SEQ, r5, dtype=plan)
        assert store5.desc.n_runs > store5.desc.n_rows
        refused(eng.Engine(spec5, plan), store5, EUNSUPPORTED, "history >= 8")
    # the classification entry point on a regression plan (one value per foot, so the label count fits: it is the logit pair that is missing)
    seq4 = dict(tw.SEQ4)
    seq4["F"] = tw.SEQ["F"][:int(tw.FX4["N"]), :4]
    rk = minicheetah_k4_recipe(tw.JP, tw.FP, T, True)
    rk.label_series, rk.label_cols = "F", [0, 1, 2, 3]
    kspec = helpers.make_spec("k4", "mini_cheetah-k4", "mini_cheetah-k4", 128, 2, grf=1)
    refused(eng.Engine(kspec, "bf16"), SequenceStore(seq4, rk, dtype="bf16"), EINVAL, "two logits", ce=True)
    # ... and the regression entry point on the classification plan
    kcls = helpers.make_spec("k4", "mini_cheetah-k4", "mini_cheetah-k4", 128, 2, regression=False)
    refused(eng.Engine(kcls, "x3"), SequenceStore(dict(tw.SEQ4), minicheetah_k4_recipe(tw.JP, tw.FP, T, True), dtype="x3"), EINVAL, "label count")


def test_a_standardised_step_needs_the_window_buffers():
    """The weight-gradient pass reads the materialised standardised windows and nothing else: x_out == NULL is MSHGNN_EUNSUPPORTED on both plans."""
    from morphsym_hgnn_amd import engine as eng
    for plan in ("bf16", "x3"):
        recipe, spec, n, store, e, flat = _setup("a1c2", plan)
        B = 3
        starts = se._starts(n, B)
        bufs, out, g, loss = _sentinels(store, e, B)
        _, y, q = store._buffers(B)
        _, run_ptrs = store.series_step_args(bf16=False)
        store.desc.run_ptrs_ready = 0
        rc = e.lib.mshgnn_step_mse_series_std(e._plan, C.byref(store.desc), store._src, None, store._pitch, store._rows, starts.data_ptr(), B, None, None,
                                              y.data_ptr(), q.data_ptr(), run_ptrs.data_ptr(), store._stats_buffer(B).data_ptr(), flat.data_ptr(), out.data_ptr(),
                                              loss.data_ptr(), g.data_ptr(), e.workspace(B, True).data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == -2 and b"materialised" in e.lib.mshgnn_last_error()      # MSHGNN_EUNSUPPORTED
        torch.cuda.synchronize()
        for b in bufs:
            assert bool((b == -7.0).all())
        assert not bool(run_ptrs.any())
