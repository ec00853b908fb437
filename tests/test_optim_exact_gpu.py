"""The flat optimizers and gradient clipping (csrc/mshgnn_train_ops.hip: k_sgd, k_adamw, k_grad_norm, k_grad_clip) ELEMENT BY ELEMENT through the C ABI
(ctypes on engine.load_library()), against the fp64 references of tests/optim_reference.py: exact data bit for bit, random data under per-element bounds
counted rounding by rounding.  tests/test_optim_reference.py shows on the host that these checkers accept an fp32 emulation of every kernel path and reject,
for every case run here, dampening on the first step, nesterov without its momentum term, weight decay behind the momentum update, AdamW's decay without lr,
coupled decay for decoupled and the reverse, an untouched tail or second sweep, a clip coefficient without its 1e-6 or without its clamp and a dropped partial
of the norm -- and that the references are torch's own optimizers to 1e-12.

Matrix: n in {1 .. 9, 1023, 1024, 1025, S, S + 3} (S = 2 097 152, the cap of the sweep's grid) x t in {1, 2, 1000} x three hyperparameter sets per optimizer
(SGD: plain with momentum_buf == NULL; nesterov + weight decay + grad_scale 1/3; momentum + dampening; a fourth with all of them at three n), the exact cases
at n in {5, 1027, S + 3}.  Every case is ONE step from the state the case gives, run three times from that state: host step + lr, device step count + lr,
host step + lr_dev; the first is held to the checker, the other two to the first one's bits.  64 sentinel elements behind every buffer; on a first step the
momentum buffer holds NaN (it must only be written).  Norm: n in {1, 3, 4, 5, 255 .. 257, one workgroup's share (1024) +- 1, one round of the full grid
(262 144) +- 1, S + 3}, random data within n 2^-53 of math.fsum, integers and a single 1.0 at the first / a middle / the last element bit for bit, every call
twice on one scratch.

Not covered, and why: n >= 2^31 (the kernels index with int64; buffers of 4 x 8 GiB do not fit a quick test); a NaN or infinite norm in the clip
(error_if_nonfinite is out of scope)."""
import ctypes as C

import pytest
import torch

from morphsym_hgnn_amd import engine as eng
from tests import optim_reference as orf
from tests import train_ops_reference as tr

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINELS = 64
FILL = (1.25, -2.5, 3.75, -5.0)


def _require_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (there is no CPU fallback to fall through to)")


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


class Buffers:
    """The case's tensors (names: keys of the case) on the device, each followed by its own sentinels; the second one is the gradient."""

    def __init__(self, case, names, poison=()):
        self.n, self.names = case["n"], names
        self.bufs = [torch.cat([case[k].to(torch.float32), torch.full((SENTINELS,), f, dtype=torch.float32)]).to(DEV) for k, f in zip(names, FILL)]
        for k in poison:
            self.bufs[names.index(k)][:self.n] = float("nan")
        self.g0 = self.bufs[1].clone()

    def ptrs(self):
        return [b.data_ptr() for b in self.bufs]

    def host(self):
        return [b[:self.n].cpu() for b in self.bufs]

    def intact(self, what):
        for b, f, name in zip(self.bufs, FILL, self.names):
            assert bool((b[self.n:] == f).all()), f"{what}: wrote past n in {name}"
        assert _same_bits(self.bufs[1], self.g0), f"{what}: the gradient buffer changed"

    def same_as(self, other, what):
        for x, y, name in zip(self.bufs, other.bufs, self.names):
            assert _same_bits(x, y), f"{what}: {name} differs in {int((x != y).sum())} elements"


def _count(t):
    return torch.tensor([t - 1, -77], dtype=torch.int64, device=DEV)


def _lr(lr):
    return torch.tensor([lr, 7.5], dtype=torch.float32, device=DEV)


def _ok(lib, rc):
    torch.cuda.synchronize()
    assert rc == 0, lib.mshgnn_last_error()


# ---------------------------------------------------------------------------------------------------
# SGD
# ---------------------------------------------------------------------------------------------------
def _sgd_call(lib, b, case, step, count, lr_dev):
    lr, mom, damp, wd, nesterov, s = case["hp"]
    p, g = b.ptrs()[:2]
    buf = b.ptrs()[2] if mom != 0 else None
    _ok(lib, lib.mshgnn_sgd_step(p, g, buf, case["n"], step, count.data_ptr() if count is not None else None, lr if lr_dev is None else -1.0,
                                 lr_dev.data_ptr() if lr_dev is not None else None, mom, damp, wd, int(nesterov), s, _stream()))


@pytest.mark.parametrize("key", orf.all_sgd_cases(), ids=lambda k: "-".join(str(v) for v in k))
def test_sgd_step_every_case(key):
    _require_gpu()
    lib = eng.load_library()
    case = orf.build_sgd_case(key)
    mom, t = case["hp"][1], case["t"]
    names = ("p", "g", "buf") if mom != 0 else ("p", "g")
    poison = ("buf",) if mom != 0 and case["first"] else ()
    a = Buffers(case, names, poison)
    _sgd_call(lib, a, case, t, None, None)
    a.intact(f"mshgnn_sgd_step {key}")
    got = a.host()
    d = orf.sgd_check(case, got[0], got[2] if mom != 0 else None)
    assert d is None, f"mshgnn_sgd_step {key}: {d}"
    b, count = Buffers(case, names, poison), _count(t)
    _sgd_call(lib, b, case, 77 if case["first"] else 1, count, None)      # (`step` is not read when the count is given: it names the other answer here)
    b.intact(f"device step count {key}")
    assert count.tolist() == [t, -77], f"the count after a step from {t - 1}"
    b.same_as(a, f"{key}: host step against device step count")
    c, lr_dev = Buffers(case, names, poison), _lr(case["hp"][0])
    _sgd_call(lib, c, case, t, None, lr_dev)      # (the lr argument is -1 here: it must not be read)
    c.intact(f"lr_dev {key}")
    assert lr_dev.tolist() == [tr.f32(case["hp"][0]), 7.5]
    c.same_as(a, f"{key}: lr against lr_dev")


def test_sgd_counts_its_steps_on_the_device_and_writes_the_buffer_first():
    """Three calls on one stream from count 0 and a NaN momentum buffer: the first only writes the buffer, the count ends at 3, and every step is within the
    checker from the state the step before left."""
    _require_gpu()
    lib = eng.load_library()
    case = orf.sgd_case(1025, 1, 3)
    b, count, lr_dev = Buffers(case, ("p", "g", "buf"), ("buf",)), _count(1), _lr(case["hp"][0])
    for k in (1, 2, 3):
        before = b.host()
        _sgd_call(lib, b, case, 99, count, lr_dev)
        assert count.tolist() == [k, -77]
        b.intact(f"call {k}")
        got = b.host()
        d = orf.sgd_check(dict(case, p=before[0], buf=before[2], first=k == 1, t=k), got[0], got[2])
        assert d is None, f"call {k}: {d}"


# ---------------------------------------------------------------------------------------------------
# Adam with weight decay
# ---------------------------------------------------------------------------------------------------
def _adamw_call(lib, b, case, step, count, lr_dev, hp=None):
    b1, b2, eps, s, lr, wd, decoupled = hp or case["hp"]
    _ok(lib, lib.mshgnn_adamw_step(*b.ptrs(), case["n"], step, count.data_ptr() if count is not None else None, lr if lr_dev is None else -1.0,
                                   lr_dev.data_ptr() if lr_dev is not None else None, b1, b2, eps, wd, int(decoupled), s, _stream()))


@pytest.mark.parametrize("key", orf.all_adamw_cases(), ids=lambda k: "-".join(str(v) for v in k))
def test_adamw_step_every_case(key):
    _require_gpu()
    lib = eng.load_library()
    case = orf.build_adamw_case(key)
    t = case["t"]
    a = Buffers(case, "pgmv")
    _adamw_call(lib, a, case, t, None, None)
    a.intact(f"mshgnn_adamw_step {key}")
    p, _, m, v = a.host()
    d = orf.adamw_check(case, p, m, v)
    assert d is None, f"mshgnn_adamw_step {key}: {d}"
    b, count = Buffers(case, "pgmv"), _count(t)
    _adamw_call(lib, b, case, 0, count, None)
    b.intact(f"device step count {key}")
    assert count.tolist() == [t, -77], f"the count after a step from {t - 1}"
    b.same_as(a, f"{key}: host step against device step count")
    c, lr_dev = Buffers(case, "pgmv"), _lr(case["hp"][4])
    _adamw_call(lib, c, case, t, None, lr_dev)
    c.intact(f"lr_dev {key}")
    c.same_as(a, f"{key}: lr against lr_dev")


@pytest.mark.parametrize("n,t,hp_i", [(5, 1, 0), (7, 2, 1), (1025, 1000, 2), (orf.S + 3, 2, 0)])
@pytest.mark.parametrize("decoupled", [0, 1])
def test_adamw_without_decay_is_adam_bit_for_bit(n, t, hp_i, decoupled):
    """mshgnn_adamw_step(weight_decay = 0) == mshgnn_adam_step (host step) and == mshgnn_adam_step_counted (device step count), with lr and with lr_dev, on
    the Adam table's own cases (decoupled with no decay multiplies p by 1: the same bits too)."""
    _require_gpu()
    lib = eng.load_library()
    case = tr.adam_case(n, t, hp_i)
    b1, b2, eps, s, lr = case["hp"]
    hp = (b1, b2, eps, s, lr, 0.0, decoupled)
    ref = Buffers(case, "pgmv")
    _ok(lib, lib.mshgnn_adam_step(*ref.ptrs(), n, t, lr, b1, b2, eps, s, _stream()))
    assert tr.adam_check(case, *[ref.host()[k] for k in (0, 2, 3)]) is None
    for lr_dev in (None, _lr(lr)):
        x = Buffers(case, "pgmv")
        _adamw_call(lib, x, case, t, None, lr_dev, hp)
        x.intact("mshgnn_adamw_step")
        x.same_as(ref, f"mshgnn_adamw_step against mshgnn_adam_step (lr_dev: {lr_dev is not None})")
    ref, count = Buffers(case, "pgmv"), _count(t)
    _ok(lib, lib.mshgnn_adam_step_counted(*ref.ptrs(), n, count.data_ptr(), lr, b1, b2, eps, s, _stream()))
    for lr_dev in (None, _lr(lr)):
        x, count = Buffers(case, "pgmv"), _count(t)
        _adamw_call(lib, x, case, 0, count, lr_dev, hp)
        assert count.tolist() == [t, -77]
        x.same_as(ref, f"mshgnn_adamw_step against mshgnn_adam_step_counted (lr_dev: {lr_dev is not None})")


def test_adamw_counts_its_steps_on_the_device():
    _require_gpu()
    lib = eng.load_library()
    case = orf.adamw_case(1025, 1, 0)
    b, count, lr_dev = Buffers(case, "pgmv"), _count(1), _lr(case["hp"][4])
    for k in (1, 2, 3):
        before = b.host()
        _adamw_call(lib, b, case, 0, count, lr_dev)
        assert count.tolist() == [k, -77]
        p, _, m, v = b.host()
        d = orf.adamw_check(dict(case, p=before[0], m=before[2], v=before[3], t=k), p, m, v)
        assert d is None, f"call {k}: {d}"


def test_refused_calls_write_nothing():
    _require_gpu()
    lib = eng.load_library()
    x = torch.ones(16 + 4, device=DEV)
    c = torch.zeros(1, dtype=torch.int64, device=DEV)
    nrm = torch.full((1,), 4.0, dtype=torch.float64, device=DEV)
    sc = torch.zeros(512, dtype=torch.int64, device=DEV)
    p, st = x.data_ptr(), _stream()
    assert lib.mshgnn_sgd_step(p, p, None, 8, 1, c.data_ptr(), 1e-2, None, 0.9, 0.0, 0.0, 0, 1.0, st) == -1            # momentum without a buffer
    assert lib.mshgnn_sgd_step(p, p, p, 8, 1, c.data_ptr(), 1e-2, None, 0.9, 0.1, 0.0, 1, 1.0, st) == -1               # nesterov with dampening
    assert lib.mshgnn_sgd_step(p + 4, p, None, 8, 1, c.data_ptr(), 1e-2, None, 0.0, 0.0, 0.0, 0, 1.0, st) == -1        # not 16-byte aligned
    assert lib.mshgnn_sgd_step(p, p, None, 8, 0, None, 1e-2, None, 0.0, 0.0, 0.0, 0, 1.0, st) == -1                    # step < 1
    assert lib.mshgnn_adamw_step(p, p, p, p, 8, 1, c.data_ptr(), 1e-3, None, 0.9, 0.999, 1e-8, -1.0, 1, 1.0, st) == -1
    assert lib.mshgnn_adamw_step(p, p, p, p + 4, 8, 1, c.data_ptr(), 1e-3, None, 0.9, 0.999, 1e-8, 0.0, 1, 1.0, st) == -1
    assert lib.mshgnn_adamw_step(p, p, p, p, 0, 1, c.data_ptr(), 1e-3, None, 0.9, 0.999, 1e-8, 0.0, 1, 1.0, st) == -1
    assert lib.mshgnn_grad_norm(p + 4, 8, nrm.data_ptr(), sc.data_ptr(), st) == -1
    assert lib.mshgnn_grad_norm(p, 8, nrm.data_ptr(), sc.data_ptr() + 8, st) == -1
    assert lib.mshgnn_grad_norm(p, 0, nrm.data_ptr(), sc.data_ptr(), st) == -1
    assert lib.mshgnn_grad_clip(p, 8, nrm.data_ptr(), -1.0, st) == -1
    assert lib.mshgnn_grad_clip(p + 4, 8, nrm.data_ptr(), 1.0, st) == -1
    torch.cuda.synchronize()
    assert bool((x == 1).all()) and int(c.item()) == 0 and float(nrm.item()) == 4.0 and not bool(sc.any())


# ---------------------------------------------------------------------------------------------------
# the gradient norm and the clipping sweep
# ---------------------------------------------------------------------------------------------------
def _norm_buffers(lib, n):
    words = lib.mshgnn_grad_norm_scratch_bytes(n) // 8
    scratch = torch.cat([torch.zeros(words, dtype=torch.int64), torch.full((SENTINELS,), -77, dtype=torch.int64)]).to(DEV)
    out = torch.tensor([-7.5, 1.25], dtype=torch.float64, device=DEV)
    return out, scratch, words


@pytest.mark.parametrize("n,kind", orf.all_norm_cases(), ids=lambda v: str(v))
def test_grad_norm_every_case(n, kind):
    """Two calls on one scratch: both by the case's checker (exact data bit for bit, random data within n 2^-53 of math.fsum), the same bits both times, the
    ticket back at 0, nothing written past the scratch, the norm's neighbour or into the gradient."""
    _require_gpu()
    lib = eng.load_library()
    case = orf.norm_case(n, kind)
    g = torch.cat([case["g"], torch.full((SENTINELS,), 1e30)]).to(DEV)      # (sentinels that would wreck the sum if they were read)
    g0 = g.clone()
    out, scratch, words = _norm_buffers(lib, n)
    assert words * 8 == 16 + (8 * orf.norm_blocks(n) + 15) // 16 * 16
    got = []
    for call in (1, 2):
        out[0] = -7.5
        _ok(lib, lib.mshgnn_grad_norm(g.data_ptr(), n, out.data_ptr(), scratch.data_ptr(), _stream()))
        assert float(out[1]) == 1.25 and bool((scratch[words:] == -77).all()) and _same_bits(g, g0), f"call {call}: wrote where it must not"
        assert int(scratch[0].item()) & 0xffffffff == 0, f"call {call}: the ticket is not back at 0"
        d = orf.norm_check(case, float(out[0]))
        assert d is None, f"norm {n} {kind}, call {call}: {d}"
        got.append(out[:1].clone())
    assert torch.equal(got[0].view(torch.int64), got[1].view(torch.int64)), "two runs of the same call differ"


@pytest.mark.parametrize("n", orf.CLIP_N)
@pytest.mark.parametrize("above", [False, True], ids=["below", "above"])
def test_grad_clip_every_case(n, above):
    """A norm below max_norm leaves every bit (the sign of a zero too); above it every element is within gamma_2 |ref| of g min(1, max_norm / (norm + 1e-6))."""
    _require_gpu()
    lib = eng.load_library()
    case = orf.clip_case(n, above)
    g = torch.cat([case["g"], torch.full((SENTINELS,), 1.25)]).to(DEV)
    norm = torch.tensor([case["norm"], -7.5], dtype=torch.float64, device=DEV)
    _ok(lib, lib.mshgnn_grad_clip(g.data_ptr(), n, norm.data_ptr(), case["max_norm"], _stream()))
    assert bool((g[n:] == 1.25).all()) and norm.tolist() == [case["norm"], -7.5]
    d = orf.clip_check(case, g[:n])
    assert d is None, f"clip {n} above={above}: {d}"


def test_norm_then_clip_on_one_stream_clips_to_max_norm():
    """The two launches as optim.clip_grad_norm_ issues them: the clip reads the norm the launch before it wrote; the clipped gradient's norm is max_norm."""
    _require_gpu()
    lib = eng.load_library()
    n = orf.NORM_SHARE + 5
    case = orf.clip_case(n, True)
    g = case["g"].to(DEV)
    out, scratch, _ = _norm_buffers(lib, n)
    assert lib.mshgnn_grad_norm(g.data_ptr(), n, out.data_ptr(), scratch.data_ptr(), _stream()) == 0
    _ok(lib, lib.mshgnn_grad_clip(g.data_ptr(), n, out.data_ptr(), case["max_norm"], _stream()))
    assert orf.norm_check(dict(case, exact=False), float(out[0])) is None
    d = orf.clip_check(dict(case, norm=float(out[0])), g)
    assert d is None, d
    after = orf.norm_reference(g.cpu())
    assert abs(after - case["max_norm"]) <= 1e-5 * case["max_norm"]
