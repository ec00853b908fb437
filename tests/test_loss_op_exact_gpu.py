"""mshgnn_regression_loss (the stand-alone MSE / L1 / Huber operator of the two-call routes) element by element.

Per kind and element count n -- around the vector width (4), the workgroup's span (256 threads x 4 = 1024 elements), the full grid (256 workgroups) and one
large n with a tail -- on random data with the special elements d == 0, |d| == delta and saturated ones of both signs:
  * the gradient is the fp32 host mirror's BITS (tests/loss_reference.py mirror32: the kernel's expressions, every operation rounded on its own);
  * the loss is within gamma_(n+6) * sum|terms| / n of the fp64 loss of the same fp32 inputs -- the derived bound of tests/ops_reference.py: at most n - 1
    additions and the two roundings of the mean (fl32(1 / n), the product) in any summation order, plus at most five roundings inside a term (d, and up to
    four operations on it), each of which moves the sum by at most u sum|terms|;
  * a sentinel behind every buffer is untouched, on 16-byte aligned pointers (the vector kernel) and on pointers off by one element (the scalar kernel);
  * two runs give identical bits (no floating-point atomic; the scratch is ready for the next call);
  * one NaN element gives a NaN loss and a NaN gradient at that element only.
"""
import numpy as np
import pytest
import torch

from morphsym_hgnn_amd import engine as eng
from tests import loss_reference as lr
from tests import ops_reference as opr

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 3, 4, 5, 7, 8, 9, 255, 256, 257, 1023, 1024, 1025, 1027, 2049, 262144, 262147, 786435]
SENTINEL = -123456.75
DELTA = 0.4
PAD = 8


def _data(n, seed, delta):
    g = torch.Generator().manual_seed(seed)
    out = torch.randn(n, generator=g, dtype=torch.float32)
    y = torch.randn(n, generator=g, dtype=torch.float32)
    k = torch.arange(n)
    y[k % 7 == 0] = out[k % 7 == 0]                                   # d == 0
    z = k % 11 == 3
    out[z] = 0.0
    y[z] = torch.where((k[z] // 11) % 2 == 0, -delta, delta).float()       # |d| == delta exactly, both signs
    s = k % 13 == 5
    y[s] = out[s] + torch.where((k[s] // 13) % 2 == 0, 3.0, -3.0).float()  # saturated, both signs
    return out, y


def _guarded(t, off, dev):
    """A device copy of `t` inside a sentinel-filled buffer, starting `off` elements behind a 16-byte boundary."""
    buf = torch.full((t.numel() + 2 * PAD,), SENTINEL, dtype=torch.float32, device=dev)
    view = buf[4 + off:4 + off + t.numel()]
    view.copy_(t)
    return buf, view


def _intact(buf, off, n):
    return bool((buf[:4 + off] == SENTINEL).all()) and bool((buf[4 + off + n:] == SENTINEL).all())


@pytest.mark.parametrize("kind", ["mse", "l1", "huber"])
def test_regression_loss_operator(kind):
    lib, dev = eng.load_library(), torch.device("cuda:0")
    delta = float(np.float32(DELTA))
    bad = []
    scratch = torch.zeros(lib.mshgnn_regression_loss_scratch_bytes(1) // 8 + 1, dtype=torch.int64, device=dev)      # zeroed once, reused by every call below
    for n in SIZES:
        out, y = _data(n, n, delta)
        gm, _ = lr.mirror32(kind, out.numpy(), y.numpy(), delta=delta)
        t64 = lr.terms64(kind, out, y, delta)
        want, bound = float(t64.sum()) / n, float(opr.gamma(n + 6)) * float(t64.abs().sum()) / n
        for off in (0, 1):      # aligned: the vector kernel; off by one element: the scalar kernel
            bo, o = _guarded(out, off, dev)
            by, t = _guarded(y, off, dev)
            bg, g = _guarded(torch.full((n,), SENTINEL), off, dev)
            bl, l = _guarded(torch.full((1,), SENTINEL), 0, dev)
            assert (o.data_ptr() % 16 == 0) == (off == 0)
            runs = []
            for _ in range(2):
                loss, grad = eng.regression_loss(lib, dev, o, t, kind, delta, scratch=scratch)
                runs.append((loss.clone(), grad.clone()))
            # into guarded buffers, straight through the C-ABI
            rc = lib.mshgnn_regression_loss(o.data_ptr(), t.data_ptr(), n, lr.KINDS[kind], delta, l.data_ptr(), g.data_ptr(), scratch.data_ptr(),
                                            torch.cuda.current_stream(dev).cuda_stream)
            assert rc == 0, lib.mshgnn_last_error()
            torch.cuda.synchronize()
            what = f"{kind} n={n} off={off}"
            if not (_intact(bo, off, n) and _intact(by, off, n) and _intact(bg, off, n) and _intact(bl, 0, 1)):
                bad.append(f"{what}: a sentinel was overwritten")
            if not (torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]) and torch.equal(l, runs[0][0]) and torch.equal(g, runs[0][1])):
                bad.append(f"{what}: two runs differ")
            got = g.cpu().numpy()
            if not np.array_equal(got.view(np.uint32), gm.view(np.uint32)):
                i = int(np.nonzero(got.view(np.uint32) != gm.view(np.uint32))[0][0])
                bad.append(f"{what}: gradient[{i}] = {got[i]!r}, the mirror has {gm[i]!r} (out {float(out[i])!r}, y {float(y[i])!r})")
            err = abs(float(l) - want)
            if not err <= bound:
                bad.append(f"{what}: loss {float(l)!r}, fp64 {want!r}: off by {err:.3e}, bound {bound:.3e}")
            # loss only
            l2, none = eng.regression_loss(lib, dev, o, t, kind, delta, want_grad=False, scratch=scratch)
            if none is not None or not torch.equal(l2, runs[0][0]):
                bad.append(f"{what}: the loss-only call differs")
    assert int(scratch[0]) == 0, "the ticket is not ready for the next call"
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("kind", ["mse", "l1", "huber"])
def test_one_nan_poisons_the_loss_and_its_own_gradient_only(kind):
    lib, dev = eng.load_library(), torch.device("cuda:0")
    n, at = 1029, 517
    out, y = _data(n, 5, DELTA)
    clean = eng.regression_loss(lib, dev, out.to(dev), y.to(dev), kind, DELTA)[1]
    out[at] = float("nan")
    loss, g = eng.regression_loss(lib, dev, out.to(dev), y.to(dev), kind, DELTA)
    assert bool(torch.isnan(loss).all())
    nan = torch.isnan(g)
    assert bool(nan[at]) and int(nan.sum()) == 1
    keep = torch.arange(n, device=dev) != at
    assert torch.equal(g[keep], clean[keep])
