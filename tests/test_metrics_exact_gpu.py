"""The numbers a run publishes -- MSE / RMSE / L1, cross entropy, 16-class accuracy, per-leg F1, the centroidal-momentum MSEs and cosine similarities, the
world-frame GRF -- VALUE BY VALUE through the C ABI (ctypes on engine.load_library()): mshgnn_metrics_regression[_step], mshgnn_metrics_classification[_step],
mshgnn_metrics_com_step and mshgnn_grf_body_to_world (csrc/mshgnn_train_ops.hip: k_metrics_reg, k_metrics_cls, k_metrics_com, k_grf_to_world) against the
fp64 references of tests/metrics_reference.py.  tests/test_metrics_reference.py shows on the host, for every case run here, that the checkers accept the
reference and reject: a dropped last element, a dropped workgroup partial, a stale partial of an earlier and larger call, n - 1, squares in the abs column,
a batch state accumulated, an epoch state overwritten, labels read as == 1, the last maximum winning, foot 0 as the low bit of the class, fp / fn swapped, a
kept F1 NaN, batch_ce[2] without its float rounding, the lin / ang halves swapped, the cosine on base node 1, on the standardised values, without the eps
clamp, R instead of R^T, a scalar-first quaternion, an unnormalised quaternion, and sums / rotation formed in fp32.

What the earlier tests (tests/test_metrics.py: a 3 x 4 and an 8-window known answer, one random batch each at 1e-12 / 1e-6 / 1e-5, the accumulating entry
points against the step ones only) left unreached: the ticket scheme over 1 .. 64 workgroups, its scratch across calls of different sizes and inside a
replayed graph, every nullable argument, the published slots beside the sums, the tie rules, `label != 0`, the eps clamp, and the direction of the rotation.

Matrix
  regression step       n in {1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8193, 262143, 262144, 262145, 266245} x {integers, binade values}: batch[0..7] and
                        epoch[0..2] are the order mirror's bits; a second call on other data (batch overwritten, epoch added); batch only, epoch only; grad_out
                        given and NULL; the inputs unchanged
  regression (adding)   n in {1, 1023, 1024, 1025, 5000} x the same data, two calls into one state: the bits of the 1024-thread mirror
  classification step   B in {1, 63, 64, 65, 255, 256, 257, 513, 16383, 16384, 16385, 16643}: the 18 counters of batch and epoch, batch_ce[1] and [3..7]
                        exact, [0] within the bound, [2] == float32([0]) / (4 B) from the call's own [0]; two runs, the same bits; each pair alone
  classification (adding)  B in {1, 1023, 1025, 3000}, two calls into one state
  COM step              B in {1, 64, 257, 16385} x n_bases in {1, 4}: exact data, all eight slots bit for bit; binade data, [0] [1] by the mirror's bits,
                        [2] [3] [6] [7] exact, [4] [5] within the counted bound; a second call; either state alone
  scratch               one zeroed-once scratch through calls of 64, 1, 2 and 64 workgroups on different data (each result exact), and the step captured in a
                        graph on one stream and replayed twice on new contents (= the eager call's bits)
  rotation              B in {1, 255, 256, 257, 1000}: signed-permutation quaternions bit for bit, random ones within 0.5 ulp32 + the fp64 budget; q and -q
  refusals              every documented argument of the six entry points, the 8-byte rule of the states and the scratch included (`ptr + 4`)
64 sentinel elements stand behind every output, state and scratch; every state and the scratch are compared at their full documented size.

Measured once on an MI355X, against the numpy references (never against another device run):
  * cross-entropy sum, |device - fsum| / (gamma_(4 B + 4) sum |terms|): at most 0.001 in the twelve step cases (the saturated
    terms of 1e4 dominate sum |terms|), 0.331 in the adding entry at B = 1, below 0.001 at B = 1023, 1025, 3000.  All below 1: the gamma bound is kept as it
    is, with no allowance for exp / log (metrics_reference.CE_K = 0; the smallest integer K the measurement needs is 0)
  * cosine sums of the binade COM cases, error / (sum of the windows' bounds + gamma_(B + 4) B): at most 0.081 (B = 1, n_bases = 4);
    0.003 and less from B = 64 on
  * rotation, random quaternions: worst error / bound 0.998 .. 1.000 -- the one rounding to fp32 uses its half ulp, the fp64 budget beside it is 2^-24 of that

Not covered, and why:
  * NaN / inf logits: fmax, exp and the comparisons have defined results for them, but the reference has no stated behaviour to pin them to.
  * a zero quaternion: 0 / 0 in the normalisation; scipy raises on it, the kernel returns NaN; nothing publishes such a value.
  * n >= 2^31: the kernels index with int64; buffers of that size (2 x 8 GiB) do not fit a quick test.
  * the exactness of half-turn quaternions of the (1, 1, 0, 0) kind: their norm is sqrt(2), so the unit components round; they run in the random cases.
  * logit gaps that underflow exp gradually (708 < gap < 745): the bound has no subnormal term; gaps here are <= ~25 or 1e4.
  * f1_nan_kept at even B, fp32 sums on integer data, a stale partial after a full grid, a dropped partial of one workgroup: the case cannot show the
    defect by construction (tests/metrics_reference.py: `damaged` returns None and says why); the other cases of the same family do.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from morphsym_hgnn_amd import engine as eng
from tests import metrics_reference as mr

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINELS = 64
EINVAL = -1
SENT_F, SENT_I, GRAD_FILL = -123.25, -77, -7.5
SCRATCH_WORDS = 16384 // 8                       # MSHGNN_METRICS_SCRATCH_BYTES


def _require_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (there is no CPU fallback to fall through to)")


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _lib():
    _require_gpu()
    return eng.load_library()


def _f64(values):
    return torch.tensor(list(np.asarray(values, dtype=np.float64)) + [SENT_F] * SENTINELS, dtype=torch.float64, device=DEV)


def _i64(values):
    return torch.tensor([int(v) for v in values] + [SENT_I] * SENTINELS, dtype=torch.int64, device=DEV)


def _scratch():
    s = torch.zeros(SCRATCH_WORDS + SENTINELS, dtype=torch.int64, device=DEV)
    s[SCRATCH_WORDS:] = SENT_I
    return s


def _grad(n):
    return torch.full((n + SENTINELS,), GRAD_FILL, dtype=torch.float32, device=DEV)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _read(t, n):
    """The first n words of a framed state on the host, after checking the frame."""
    h = t.cpu()
    fill = SENT_F if t.dtype == torch.float64 else SENT_I
    assert h.numel() == n + SENTINELS and bool((h[n:] == fill).all()), "wrote past the end of a state"
    return h[:n].numpy().copy()


def _scratch_settled(s):
    h = s.cpu()
    assert bool((h[SCRATCH_WORDS:] == SENT_I).all()), "wrote past the scratch"
    assert int(h[0]) & 0xFFFFFFFF == 0, "the ticket was not reset"


def _grad_intact(g, n):
    assert bool((g[n:] == GRAD_FILL).all()), "wrote past grad_out"


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _ok(lib, rc):
    torch.cuda.synchronize()
    assert rc == 0, lib.mshgnn_last_error()


# ---------------------------------------------------------------------------------------------------
# regression
# ---------------------------------------------------------------------------------------------------
def _reg_step(lib, case, p, y, batch, epoch, grad, scratch):
    rc = lib.mshgnn_metrics_regression_step(p.data_ptr(), y.data_ptr(), case["n"], batch.data_ptr() if batch is not None else None,
                                            epoch.data_ptr() if epoch is not None else None, grad.data_ptr() if grad is not None else None,
                                            scratch.data_ptr(), _stream())
    _ok(lib, rc)
    _scratch_settled(scratch)
    d = mr.reg_check(case, _read(batch, 8) if batch is not None else None, _read(epoch, 3) if epoch is not None else None)
    assert d is None, d


@pytest.mark.parametrize("n", mr.REG_N)
@pytest.mark.parametrize("maker", ["exact_reg", "binade_reg"])
def test_regression_step_is_the_order_mirror_bit_for_bit(maker, n):
    lib = _lib()
    case = getattr(mr, maker)(n)
    p, y = _dev(case["pred"]), _dev(case["y"])
    p0, y0 = p.clone(), y.clone()
    batch, epoch, scratch, grad = _f64([mr.BATCH_FILL] * 8), _f64(case["epoch0"]), _scratch(), _grad(n)
    _reg_step(lib, case, p, y, batch, epoch, grad, scratch)
    _grad_intact(grad, n)
    want_g = ((2.0 / n) * (case["pred"].astype(np.float64) - case["y"])).astype(np.float32)
    assert _same_bits(grad[:n].cpu(), torch.from_numpy(want_g)), "grad_out is not float32(fp64(2 / n) (pred - y))"
    assert _same_bits(p, p0) and _same_bits(y, y0), "the inputs changed"
    # a second call on other data, into the same states and scratch, without grad_out: batch overwritten, epoch added
    second = getattr(mr, maker)(n, seed=1, epoch0=mr.reg_expected(case)["epoch"])
    p2, y2 = _dev(second["pred"]), _dev(second["y"])
    _reg_step(lib, second, p2, y2, batch, epoch, None, scratch)
    # either state alone
    only_b, only_e = _f64([mr.BATCH_FILL] * 8), _f64(case["epoch0"])
    _reg_step(lib, case, p, y, only_b, None, None, scratch)
    _reg_step(lib, case, p, y, None, only_e, grad, scratch)
    _grad_intact(grad, n)


@pytest.mark.parametrize("n", mr.REG_ACC_N)
@pytest.mark.parametrize("maker", ["exact_reg", "binade_reg"])
def test_regression_accumulating_entry_is_the_1024_thread_mirror(maker, n):
    lib = _lib()
    case = getattr(mr, maker)(n, entry="acc")
    second = getattr(mr, maker)(n, entry="acc", seed=1, epoch0=mr.reg_expected(case)["epoch"])
    state = _f64(case["epoch0"])
    for c in (case, second):
        p, y = _dev(c["pred"]), _dev(c["y"])
        _ok(lib, lib.mshgnn_metrics_regression(p.data_ptr(), y.data_ptr(), n, state.data_ptr(), _stream()))
        d = mr.reg_check(c, None, _read(state, 3))
        assert d is None, d


# ---------------------------------------------------------------------------------------------------
# classification
# ---------------------------------------------------------------------------------------------------
def _cls_step(lib, case, lg, lab, ce_b, cnt_b, ce_e, cnt_e, grad, scratch):
    ptr = lambda t: t.data_ptr() if t is not None else None
    rc = lib.mshgnn_metrics_classification_step(lg.data_ptr(), lab.data_ptr(), case["B"], ptr(ce_b), ptr(cnt_b), ptr(ce_e), ptr(cnt_e), ptr(grad),
                                                scratch.data_ptr(), _stream())
    _ok(lib, rc)
    _scratch_settled(scratch)
    got = [_read(ce_b, 8) if ce_b is not None else None, _read(cnt_b, mr.N_COUNTS) if cnt_b is not None else None,
           _read(ce_e, 2) if ce_e is not None else None, _read(cnt_e, mr.N_COUNTS) if cnt_e is not None else None]
    d = mr.cls_check(case, *got, mr.CE_K)
    assert d is None, d
    return got


def _cls_states(case):
    return _f64([mr.BATCH_FILL] * 8), _i64([7] * mr.N_COUNTS), _f64(case["ce0"]), _i64(case["counts0"])


@pytest.mark.parametrize("B", mr.CLS_B)
def test_classification_step_counters_exact_and_the_cross_entropy_within_its_bound(B):
    lib = _lib()
    case = mr.cls_case(B)
    lg, lab = _dev(case["logits"]), _dev(case["labels"])
    assert lab.dtype == torch.int32
    lg0, lab0 = lg.clone(), lab.clone()
    scratch, grad = _scratch(), _grad(B * 8)
    runs = []
    for g in (grad, None):                       # two runs on fresh states: the same bits
        runs.append(_cls_step(lib, case, lg, lab, *_cls_states(case), g, scratch))
    _grad_intact(grad, B * 8)
    print(f"CE B {B}: error / bound {mr.ce_ratio(case, runs[0][0][0]):.3f}")
    for a, b in zip(*runs):
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), "two runs of the same step differ"
    assert _same_bits(lg, lg0) and torch.equal(lab, lab0), "the inputs changed"
    ce_b, cnt_b, ce_e, cnt_e = _cls_states(case)
    _cls_step(lib, case, lg, lab, ce_b, cnt_b, None, None, None, scratch)
    _cls_step(lib, case, lg, lab, None, None, ce_e, cnt_e, None, scratch)
    # a second step on other data into the epoch pair: added
    second = mr.cls_case(B, seed=1)
    second["ce0"], second["counts0"] = _read(ce_e, 2), _read(cnt_e, mr.N_COUNTS)
    _cls_step(lib, second, _dev(second["logits"]), _dev(second["labels"]), ce_b, cnt_b, ce_e, cnt_e, None, scratch)


@pytest.mark.parametrize("B", mr.CLS_ACC_B)
def test_classification_accumulating_entry_adds_exact_counters(B):
    lib = _lib()
    case, second = mr.cls_case(B, entry="acc"), mr.cls_case(B, entry="acc", seed=1)
    ce, cnt = _f64(case["ce0"]), _i64(case["counts0"])
    for c in (case, second):
        lg, lab = _dev(c["logits"]), _dev(c["labels"])
        _ok(lib, lib.mshgnn_metrics_classification(lg.data_ptr(), lab.data_ptr(), B, ce.data_ptr(), cnt.data_ptr(), _stream()))
        got_ce, got_c = _read(ce, 2), _read(cnt, mr.N_COUNTS)
        d = mr.cls_check(c, None, None, got_ce, got_c, mr.CE_K)
        assert d is None, d
        print(f"CE (adding) B {B}: error / bound {abs(got_ce[0] - c['ce0'][0] - mr.cls_expected(c)['ce']) / mr.ce_bound(mr.cls_expected(c), 0):.3f}")
        second["ce0"], second["counts0"] = got_ce, got_c


# ---------------------------------------------------------------------------------------------------
# centroidal momentum
# ---------------------------------------------------------------------------------------------------
def _vec6(a):
    return (C.c_double * 6)(*[float(v) for v in a])


def _com_step(lib, case, p, y, batch, epoch, scratch):
    rc = lib.mshgnn_metrics_com_step(p.data_ptr(), y.data_ptr(), case["B"], case["nb"], _vec6(case["mean"]), _vec6(case["std"]),
                                     batch.data_ptr() if batch is not None else None, epoch.data_ptr() if epoch is not None else None, scratch.data_ptr(), _stream())
    _ok(lib, rc)
    _scratch_settled(scratch)
    got = (_read(batch, 8) if batch is not None else None, _read(epoch, 8) if epoch is not None else None)
    d = mr.com_check(case, *got)
    assert d is None, d
    return got


@pytest.mark.parametrize("nb", mr.COM_NB)
@pytest.mark.parametrize("B", mr.COM_B)
@pytest.mark.parametrize("maker", ["com_exact", "com_random"])
def test_com_step_sums_and_cosines(maker, B, nb):
    lib = _lib()
    case = getattr(mr, maker)(B, nb)
    p, y = _dev(case["pred"]), _dev(case["y"])
    p0, y0 = p.clone(), y.clone()
    batch, epoch, scratch = _f64([mr.BATCH_FILL] * 8), _f64(case["epoch0"]), _scratch()
    got_b, got_e = _com_step(lib, case, p, y, batch, epoch, scratch)
    if maker == "com_random":
        print(f"COM B {B} nb {nb}: cosine error / bound {mr.com_ratio(case, got_b):.3f}")
    assert _same_bits(p, p0) and _same_bits(y, y0), "the inputs changed"
    second = getattr(mr, maker)(B, nb, seed=1)
    second["epoch0"] = got_e
    _com_step(lib, second, _dev(second["pred"]), _dev(second["y"]), batch, epoch, scratch)
    _com_step(lib, case, p, y, _f64([mr.BATCH_FILL] * 8), None, scratch)
    _com_step(lib, case, p, y, None, _f64(case["epoch0"]), scratch)


# ---------------------------------------------------------------------------------------------------
# the scratch across calls, and inside a graph
# ---------------------------------------------------------------------------------------------------
def test_one_scratch_serves_regression_calls_of_64_1_2_and_64_workgroups():
    lib = _lib()
    scratch, epoch = _scratch(), _f64(mr.REG_EPOCH0)
    epoch0 = mr.REG_EPOCH0
    for k, n in enumerate(mr.SCRATCH_SEQUENCE["reg"]):
        case = mr.exact_reg(n, seed=10 + k, epoch0=epoch0)
        _reg_step(lib, case, _dev(case["pred"]), _dev(case["y"]), _f64([mr.BATCH_FILL] * 8), epoch, None, scratch)
        epoch0 = mr.reg_expected(case)["epoch"]


def test_one_scratch_serves_classification_calls_of_64_1_2_and_64_workgroups():
    lib = _lib()
    scratch = _scratch()
    for k, B in enumerate(mr.SCRATCH_SEQUENCE["cls"]):
        case = mr.cls_case(B, seed=20 + k)
        _cls_step(lib, case, _dev(case["logits"]), _dev(case["labels"]), *_cls_states(case), None, scratch)


def test_one_scratch_serves_com_calls_of_64_1_2_and_64_workgroups():
    lib = _lib()
    scratch = _scratch()
    for k, B in enumerate(mr.SCRATCH_SEQUENCE["com"]):
        case = mr.com_exact(B, mr.SCRATCH_COM_NB, seed=10 + k)
        _com_step(lib, case, _dev(case["pred"]), _dev(case["y"]), _f64([mr.BATCH_FILL] * 8), _f64(case["epoch0"]), scratch)


def _captured(call):
    """`call` once eagerly (the kernel's first launch stays outside the capture), then captured on the capture stream."""
    call()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    return graph


def test_regression_step_replays_in_a_graph_on_new_contents():
    lib = _lib()
    n = mr.GRAPH_ITEMS["reg"]
    cases = [mr.exact_reg(n, seed=14 + k) for k in range(3)]
    p, y = _dev(cases[0]["pred"]), _dev(cases[0]["y"])
    batch, epoch, scratch = _f64([mr.BATCH_FILL] * 8), _f64(mr.REG_EPOCH0), _scratch()
    state = {"rc": 0}

    def call():
        state["rc"] |= lib.mshgnn_metrics_regression_step(p.data_ptr(), y.data_ptr(), n, batch.data_ptr(), epoch.data_ptr(), None, scratch.data_ptr(), _stream())
    graph = _captured(call)
    assert state["rc"] == 0, lib.mshgnn_last_error()
    epoch0 = mr.reg_expected(cases[0])["epoch"]                      # (the eager call before the capture ran the step once)
    d = mr.reg_check(cases[0], _read(batch, 8), _read(epoch, 3))
    assert d is None, f"capturing must not run the step: {d}"
    for case in cases[1:]:
        case["epoch0"] = epoch0
        p.copy_(_dev(case["pred"])); y.copy_(_dev(case["y"]))
        graph.replay()
        torch.cuda.synchronize()
        _scratch_settled(scratch)
        got_b, got_e = _read(batch, 8), _read(epoch, 3)
        d = mr.reg_check(case, got_b, got_e)
        assert d is None, d
        eb, ee = _f64([mr.BATCH_FILL] * 8), _f64(epoch0)
        _reg_step(lib, case, p, y, eb, ee, None, _scratch())
        assert np.array_equal(_read(eb, 8).view(np.uint64), got_b.view(np.uint64)) and np.array_equal(_read(ee, 3).view(np.uint64), got_e.view(np.uint64))
        epoch0 = mr.reg_expected(case)["epoch"]


def test_classification_step_replays_in_a_graph_on_new_contents():
    lib = _lib()
    B = mr.GRAPH_ITEMS["cls"]
    cases = [mr.cls_case(B, seed=24 + k) for k in range(3)]
    lg, lab = _dev(cases[0]["logits"]), _dev(cases[0]["labels"])
    ce_b, cnt_b, ce_e, cnt_e = _cls_states(cases[0])
    scratch = _scratch()
    state = {"rc": 0}

    def call():
        state["rc"] |= lib.mshgnn_metrics_classification_step(lg.data_ptr(), lab.data_ptr(), B, ce_b.data_ptr(), cnt_b.data_ptr(), ce_e.data_ptr(), cnt_e.data_ptr(),
                                                             None, scratch.data_ptr(), _stream())
    graph = _captured(call)
    assert state["rc"] == 0, lib.mshgnn_last_error()
    d = mr.cls_check(cases[0], _read(ce_b, 8), _read(cnt_b, mr.N_COUNTS), _read(ce_e, 2), _read(cnt_e, mr.N_COUNTS), mr.CE_K)
    assert d is None, f"capturing must not run the step: {d}"
    for case in cases[1:]:
        case["ce0"], case["counts0"] = _read(ce_e, 2), _read(cnt_e, mr.N_COUNTS)
        lg.copy_(_dev(case["logits"])); lab.copy_(_dev(case["labels"]))
        graph.replay()
        torch.cuda.synchronize()
        _scratch_settled(scratch)
        got = [_read(ce_b, 8), _read(cnt_b, mr.N_COUNTS), _read(ce_e, 2), _read(cnt_e, mr.N_COUNTS)]
        d = mr.cls_check(case, *got, mr.CE_K)
        assert d is None, d
        eager = _cls_step(lib, case, lg, lab, _f64([mr.BATCH_FILL] * 8), _i64([7] * mr.N_COUNTS), _f64(case["ce0"]), _i64(case["counts0"]), None, _scratch())
        for a, b in zip(got, eager):
            assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), "the replay differs from the eager call"


def test_com_step_replays_in_a_graph_on_new_contents():
    lib = _lib()
    B, nb = mr.GRAPH_ITEMS["com"], mr.SCRATCH_COM_NB
    cases = [mr.com_exact(B, nb, seed=14 + k) for k in range(3)]
    p, y = _dev(cases[0]["pred"]), _dev(cases[0]["y"])
    batch, epoch, scratch = _f64([mr.BATCH_FILL] * 8), _f64(cases[0]["epoch0"]), _scratch()
    mean, std = _vec6(cases[0]["mean"]), _vec6(cases[0]["std"])
    state = {"rc": 0}

    def call():
        state["rc"] |= lib.mshgnn_metrics_com_step(p.data_ptr(), y.data_ptr(), B, nb, mean, std, batch.data_ptr(), epoch.data_ptr(), scratch.data_ptr(), _stream())
    graph = _captured(call)
    assert state["rc"] == 0, lib.mshgnn_last_error()
    d = mr.com_check(cases[0], _read(batch, 8), _read(epoch, 8))
    assert d is None, f"capturing must not run the step: {d}"
    for case in cases[1:]:
        case["epoch0"] = _read(epoch, 8)
        p.copy_(_dev(case["pred"])); y.copy_(_dev(case["y"]))
        graph.replay()
        torch.cuda.synchronize()
        _scratch_settled(scratch)
        got_b, got_e = _read(batch, 8), _read(epoch, 8)
        d = mr.com_check(case, got_b, got_e)
        assert d is None, d
        eb, ee = _com_step(lib, case, p, y, _f64([mr.BATCH_FILL] * 8), _f64(case["epoch0"]), _scratch())
        assert np.array_equal(eb.view(np.uint64), got_b.view(np.uint64)) and np.array_equal(ee.view(np.uint64), got_e.view(np.uint64))


# ---------------------------------------------------------------------------------------------------
# rotation
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", mr.GRF_B)
@pytest.mark.parametrize("maker", ["grf_exact", "grf_random"])
def test_grf_rotation_is_the_inverse_of_the_scalar_last_quaternion(maker, B):
    lib = _lib()
    case = getattr(mr, maker)(B)
    q, f = _dev(case["quat"]), _dev(case["body"])
    q0, f0 = q.clone(), f.clone()
    outs = []
    for quat in (q, -q):
        out = _grad(B * 12)
        _ok(lib, lib.mshgnn_grf_body_to_world(quat.data_ptr(), f.data_ptr(), out.data_ptr(), B, _stream()))
        _grad_intact(out, B * 12)
        outs.append(out[:B * 12].cpu())
    d = mr.grf_check(case, outs[0].numpy())
    assert d is None, d
    if maker == "grf_random":
        err = np.abs(outs[0].numpy().reshape(B, 12).astype(mr.EXT) - case["want"]).astype(np.float64)
        print(f"GRF B {B}: worst error / bound {float((err / mr.grf_bound(case)).max()):.3f}")
    assert _same_bits(outs[0], outs[1]), "q and -q give different bits"
    assert _same_bits(q, q0) and _same_bits(f, f0), "the inputs changed"


# ---------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------
def _refused(lib, name, good, bad_sets):
    fn = getattr(lib, name)
    for changes in bad_sets:
        args = list(good)
        for pos, bad in changes:
            args[pos] = bad
        assert fn(*args) == EINVAL, (name, changes)
        assert name.encode() in lib.mshgnn_last_error(), (name, changes, lib.mshgnn_last_error())


def test_every_entry_point_refuses_its_bad_arguments_before_any_launch():
    lib = _lib()
    B, nb = 65, 2
    x = torch.ones(B * nb * 6 + SENTINELS, dtype=torch.float32, device=DEV)          # serves as pred, y, logits (B * 8), quat, body and world
    lab = torch.ones(B * 4, dtype=torch.int32, device=DEV)
    f = [_f64([5.0] * 8) for _ in range(4)]
    c = [_i64([5] * mr.N_COUNTS) for _ in range(2)]
    scratch = _scratch()
    mean, std = _vec6(np.zeros(6)), _vec6(np.ones(6))
    X, L, S, N = x.data_ptr(), lab.data_ptr(), scratch.data_ptr(), None
    F, Cn = [t.data_ptr() for t in f], [t.data_ptr() for t in c]
    _refused(lib, "mshgnn_metrics_regression", [X, X, B, F[0], N],
             [[(0, N)], [(1, N)], [(3, N)], [(2, 0)], [(2, -1)], [(3, F[0] + 4)]])
    _refused(lib, "mshgnn_metrics_regression_step", [X, X, B, F[0], F[1], N, S, N],
             [[(0, N)], [(1, N)], [(2, 0)], [(2, -5)], [(3, N), (4, N)], [(6, N)], [(6, S + 4)], [(3, F[0] + 4)], [(4, F[1] + 4)], [(3, N), (4, F[1] + 4)]])
    _refused(lib, "mshgnn_metrics_classification", [X, L, B, F[0], Cn[0], N],
             [[(0, N)], [(1, N)], [(3, N)], [(4, N)], [(2, 0)], [(3, F[0] + 4)], [(4, Cn[0] + 4)]])
    _refused(lib, "mshgnn_metrics_classification_step", [X, L, B, F[0], Cn[0], F[1], Cn[1], N, S, N],
             [[(0, N)], [(1, N)], [(2, 0)], [(8, N)], [(3, N)], [(4, N)], [(5, N)], [(6, N)], [(3, N), (4, N), (5, N), (6, N)],
              [(8, S + 4)], [(3, F[0] + 4)], [(4, Cn[0] + 4)], [(5, F[1] + 4)], [(6, Cn[1] + 4)]])
    _refused(lib, "mshgnn_metrics_com_step", [X, X, B, nb, mean, std, F[2], F[3], S, N],
             [[(0, N)], [(1, N)], [(4, N)], [(5, N)], [(2, 0)], [(3, 0)], [(3, -1)], [(6, N), (7, N)], [(8, N)], [(8, S + 4)], [(6, F[2] + 4)], [(7, F[3] + 4)]])
    _refused(lib, "mshgnn_grf_body_to_world", [X, X, X, B, N], [[(0, N)], [(1, N)], [(2, N)], [(3, 0)], [(3, -2)]])
    torch.cuda.synchronize()
    for t in f:
        assert bool((_read(t, 8) == 5.0).all())
    for t in c:
        assert bool((_read(t, mr.N_COUNTS) == 5).all())
    h = scratch.cpu()
    assert not bool(h[:SCRATCH_WORDS].any()) and bool((h[SCRATCH_WORDS:] == SENT_I).all()) and bool((x == 1).all()) and bool((lab == 1).all())
