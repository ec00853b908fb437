"""Host tests of tests/optim_reference.py (no GPU): the fp64 references agree with torch's own optimizers and clip_grad_norm_, every checker of every case
of the GPU tables accepts the fp32 emulation of its kernel path and rejects every damaged variant that exists for the case, the exact cases close, and the
library's five new entry points -- loaded without a device -- are declared, exported, bound and refuse bad arguments with a message before any launch."""
import ctypes as C
import math
import os
import re

import pytest
import torch

from morphsym_hgnn_amd import engine
from tests import optim_reference as orf
from tests.ops_reference import DoesNotClose

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TORCH_RTOL = 1e-12      # oracle == reference, the figure of oracle/gen_golden.py
SMALL = 1027            # the host controls run every (t, set) of the tables at the sizes up to this one, and one key of each kind at the large ones


def _close(a, b, what):
    err = (a - b).abs()
    assert bool((err <= TORCH_RTOL * b.abs()).all()), f"{what}: {float((err / b.abs().clamp_min(1e-300)).max()):.3e} relative"


def _fixed(n=64, steps=3, seed=11):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(n, generator=gen, dtype=torch.float64).float(), [torch.randn(n, generator=gen, dtype=torch.float64).float() for _ in range(steps)]


# ---------------------------------------------------------------------------------------------------
# the references are torch's semantics
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hp", orf.SGD_HP + orf.SGD_EXACT_HP, ids=str)
def test_sgd_reference_is_torch_sgd(hp):
    hp = orf._hp(hp)
    lr, mom, damp, wd, nesterov, s = hp
    p0, grads = _fixed()
    q = torch.nn.Parameter(p0.double().clone())
    opt = torch.optim.SGD([q], lr=lr, momentum=mom, dampening=damp, weight_decay=wd, nesterov=nesterov)
    p, buf = p0.double(), None
    for t, g in enumerate(grads, 1):
        q.grad = g.double() * s
        opt.step()
        p, buf = orf.sgd_reference(p, g, buf, t == 1, hp)
        _close(p, q.detach(), f"step {t}: p")
        if mom != 0:
            _close(buf, opt.state[q]["momentum_buffer"], f"step {t}: momentum_buffer")
        else:
            assert buf is None and "momentum_buffer" not in opt.state[q]


@pytest.mark.parametrize("hp", orf.ADAMW_HP + [orf.ADAMW_EXACT_HP], ids=str)
def test_adamw_reference_is_torch_adam_and_adamw(hp):
    hp = orf._hp(hp)
    b1, b2, eps, s, lr, wd, decoupled = hp
    p0, grads = _fixed()
    q = torch.nn.Parameter(p0.double().clone())
    opt = (torch.optim.AdamW if decoupled else torch.optim.Adam)([q], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    p, m, v = p0.double(), torch.zeros(64, dtype=torch.float64), torch.zeros(64, dtype=torch.float64)
    for t, g in enumerate(grads, 1):
        q.grad = g.double() * s
        opt.step()
        p, m, v = orf.adamw_reference(p, g, m, v, t, hp)
        _close(p, q.detach(), f"step {t}: p")
        _close(m, opt.state[q]["exp_avg"], f"step {t}: exp_avg")
        _close(v, opt.state[q]["exp_avg_sq"], f"step {t}: exp_avg_sq")


@pytest.mark.parametrize("max_norm", [0.5, 3.0, 1e3])
def test_norm_and_clip_references_are_torch_clip_grad_norm(max_norm):
    _, grads = _fixed(n=96)
    qs = [torch.nn.Parameter(torch.zeros(32, dtype=torch.float64)) for _ in range(3)]
    flat = grads[0]
    for k, q in enumerate(qs):
        q.grad = flat[32 * k:32 * k + 32].double().clone()
    total = torch.nn.utils.clip_grad_norm_(qs, max_norm)
    norm = orf.norm_reference(flat)
    assert abs(float(total) - norm) <= TORCH_RTOL * norm
    _close(orf.clip_reference(flat, norm, max_norm), torch.cat([q.grad for q in qs]), "clipped gradient")
    assert (orf.clip_coefficient(norm, max_norm) == 1.0) == (max_norm == 1e3)


# ---------------------------------------------------------------------------------------------------
# the checkers: the emulation passes, every damage is rejected
# ---------------------------------------------------------------------------------------------------
def _host_keys(keys):
    """Every key up to SMALL elements, and of the large sizes the first key of every (kind, n, hyperparameter set)."""
    out, seen = [], set()
    for k in keys:
        if k[1] <= SMALL:
            out.append(k)
        elif (k[0], k[1], k[-1]) not in seen:
            seen.add((k[0], k[1], k[-1]))
            out.append(k)
    return out


def test_sgd_checkers_accept_the_emulation_and_reject_every_damage():
    seen = {k: 0 for k in orf.SGD_DAMAGES}
    for key in _host_keys(orf.all_sgd_cases()):
        case = orf.build_sgd_case(key)
        good = orf.sgd_emulation(case["p"], case["g"], case["buf"], case["first"], case["hp"])
        assert orf.sgd_check(case, *good) is None, (key, orf.sgd_check(case, *good))
        for kind in orf.SGD_DAMAGES:
            bad = orf.damaged_sgd(case, kind)
            if bad is not None:
                seen[kind] += 1
                assert orf.sgd_check(case, *bad) is not None, f"{key}: the checker accepts '{kind}'"
    assert all(seen.values()), seen


def test_adamw_checkers_accept_the_emulation_and_reject_every_damage():
    seen = {k: 0 for k in orf.ADAMW_DAMAGES}
    for key in _host_keys(orf.all_adamw_cases()):
        case = orf.build_adamw_case(key)
        good = orf.adamw_emulation(case["p"], case["g"], case["m"], case["v"], case["t"], case["hp"])
        assert orf.adamw_check(case, *good) is None, (key, orf.adamw_check(case, *good))
        for kind in orf.ADAMW_DAMAGES:
            bad = orf.damaged_adamw(case, kind)
            if bad is not None:
                seen[kind] += 1
                assert orf.adamw_check(case, *bad) is not None, f"{key}: the checker accepts '{kind}'"
        if case["hp"][5] != 0 and not case["exact"]:      # wherever a decay is asked for, both decay damages exist: the data shows the decay at every n
            assert orf.damaged_adamw(case, "other_decay") is not None, key
    assert all(seen.values()), seen


def test_norm_checker_accepts_the_kernel_order_and_rejects_a_dropped_partial():
    dropped = 0
    for n, kind in orf.all_norm_cases():
        case = orf.norm_case(n, kind)
        assert orf.norm_check(case, orf.norm_emulation(case["g"])) is None, (n, kind)
        bad = orf.damaged_norm(case)
        assert bad is not None
        dropped += 1
        assert orf.norm_check(case, bad) is not None, f"norm {n} {kind}: the checker accepts a dropped partial"
    assert dropped == len(orf.all_norm_cases())
    assert [orf.norm_blocks(n) for n in (1, 4, 5, 1024, 1025, orf.NORM_ROUND, orf.NORM_ROUND + 1, 10 ** 9)] == [1, 1, 1, 1, 2, 256, 256, 256]


def test_clip_checker_accepts_the_emulation_and_rejects_every_damage():
    seen = {k: 0 for k in orf.CLIP_DAMAGES}
    for n in orf.CLIP_N:
        for above in (False, True):
            case = orf.clip_case(n, above)
            assert (orf.clip_coefficient(case["norm"], case["max_norm"]) < 1.0) == above
            assert orf.clip_check(case, orf.clip_emulation(case["g"], case["norm"], case["max_norm"])) is None, (n, above)
            for kind in orf.CLIP_DAMAGES:
                bad = orf.damaged_clip(case, kind)
                if bad is not None:
                    seen[kind] += 1
                    assert orf.clip_check(case, bad) is not None, f"clip {n} above={above}: the checker accepts '{kind}'"
            assert orf.damaged_clip(case, "no_eps" if above else "not_clamped") is not None
            flipped = orf.clip_emulation(case["g"], case["norm"], case["max_norm"]).clone()
            if not above and n >= 2:          # the sign of a zero is a bit too
                assert bool((case["g"] == 0).any())
                z = int((case["g"] == 0).nonzero()[0])
                flipped[z] = -flipped[z]
                assert orf.clip_check(case, flipped) is not None
    assert all(seen.values()), seen


def test_exact_cases_refuse_data_that_does_not_close(monkeypatch):
    monkeypatch.setattr(orf, "SGD_EXACT_HP", [(0.1, 0.5, 0.5, 0.25, False, 1.0)])
    with pytest.raises(DoesNotClose):
        orf.sgd_exact_case.__wrapped__(5, 2, 0)
    monkeypatch.setattr(orf, "ADAMW_EXACT_HP", (0.5, 0.75, 2.0 ** -10, 1.0, 2.0 ** -10, 0.1, 1))
    with pytest.raises(DoesNotClose):
        orf.adamw_exact_case.__wrapped__(5)
    with pytest.raises(DoesNotClose):
        monkeypatch.setattr(orf, "norm_reference", lambda g: 2.0)
        orf.norm_case.__wrapped__(7, "one@0")


# ---------------------------------------------------------------------------------------------------
# the library, loaded without a device
# ---------------------------------------------------------------------------------------------------
NEW = ("mshgnn_sgd_step", "mshgnn_adamw_step", "mshgnn_grad_norm_scratch_bytes", "mshgnn_grad_norm", "mshgnn_grad_clip")


def test_the_five_entry_points_are_declared_exported_and_bound():
    lib = engine.load_library()
    hdr = open(os.path.join(ROOT, "include", "mshgnn.h")).read()
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", hdr), f"include/mshgnn.h does not declare {name}"
        assert name in engine.EXPORTS and hasattr(lib, name) and getattr(lib, name).argtypes is not None, name
    assert int(re.search(r"#define MSHGNN_ABI_VERSION (\d+)", hdr).group(1)) == engine.ABI_VERSION == 6
    assert lib.mshgnn_grad_norm_scratch_bytes(0) == 0
    sizes = [lib.mshgnn_grad_norm_scratch_bytes(n) for n in (1, 1024, 1025, orf.NORM_ROUND, 10 ** 9)]
    assert sizes == [16 + 16, 16 + 16, 16 + 16, 16 + 8 * 256, 16 + 8 * 256] and all(s % 16 == 0 for s in sizes)


def test_every_argument_check_returns_its_code_with_a_message():
    """None of these calls reaches a launch: the pointers are made-up addresses that are never dereferenced."""
    lib = engine.load_library()
    A, odd, n = 0x10000, 0x10004, 8          # an aligned and a misaligned address
    nan = float("nan")

    def refused(rc, text):
        assert rc == -1, text
        msg = lib.mshgnn_last_error().decode()
        assert text in msg, (text, msg)

    def sgd(p=A, g=A, buf=None, n=n, step=1, count=None, lr=1e-2, lr_dev=None, mom=0.0, damp=0.0, wd=0.0, nesterov=0, s=1.0):
        return lib.mshgnn_sgd_step(p, g, buf, n, step, count, lr, lr_dev, mom, damp, wd, nesterov, s, None)
    refused(sgd(p=None), "bad argument to mshgnn_sgd_step")
    refused(sgd(g=None), "bad argument to mshgnn_sgd_step")
    refused(sgd(n=0), "bad argument to mshgnn_sgd_step")
    refused(sgd(mom=0.9), "momentum_buf must be given exactly when momentum != 0")
    refused(sgd(buf=A), "momentum_buf must be given exactly when momentum != 0")
    refused(sgd(mom=-0.5, buf=A), "must be >= 0")
    refused(sgd(wd=-1.0), "must be >= 0")
    refused(sgd(wd=nan), "must be >= 0")
    refused(sgd(nesterov=1), "nesterov needs momentum > 0 and dampening == 0")
    refused(sgd(nesterov=1, mom=0.9, buf=A, damp=0.1), "nesterov needs momentum > 0 and dampening == 0")
    refused(sgd(p=odd), "16-byte aligned")
    refused(sgd(g=odd), "16-byte aligned")
    refused(sgd(mom=0.9, buf=odd), "16-byte aligned")
    refused(sgd(step=0), "step must be >= 1")
    refused(sgd(step=0, count=odd), "step_count must be 8-byte aligned")
    refused(sgd(lr_dev=A + 2), "lr_dev must be 4-byte aligned")
    refused(sgd(lr=-1.0), "lr must be >= 0")
    refused(sgd(lr=nan), "lr must be >= 0")

    def adamw(p=A, g=A, m=A, v=A, n=n, step=1, count=None, lr=1e-3, lr_dev=None, wd=1e-2, decoupled=1):
        return lib.mshgnn_adamw_step(p, g, m, v, n, step, count, lr, lr_dev, 0.9, 0.999, 1e-8, wd, decoupled, 1.0, None)
    for k in "pgmv":
        refused(adamw(**{k: None}), "bad argument to mshgnn_adamw_step")
        refused(adamw(**{k: odd}), "16-byte aligned")
    refused(adamw(n=-1), "bad argument to mshgnn_adamw_step")
    refused(adamw(wd=-1e-2), "weight_decay must be >= 0")
    refused(adamw(step=0), "step must be >= 1")
    refused(adamw(count=odd), "step_count must be 8-byte aligned")
    refused(adamw(lr_dev=A + 1), "lr_dev must be 4-byte aligned")
    refused(adamw(lr=-1e-3), "lr must be >= 0")

    refused(lib.mshgnn_grad_norm(None, n, A, A, None), "bad argument to mshgnn_grad_norm")
    refused(lib.mshgnn_grad_norm(A, n, None, A, None), "bad argument to mshgnn_grad_norm")
    refused(lib.mshgnn_grad_norm(A, n, A, None, None), "bad argument to mshgnn_grad_norm")
    refused(lib.mshgnn_grad_norm(A, 0, A, A, None), "bad argument to mshgnn_grad_norm")
    refused(lib.mshgnn_grad_norm(odd, n, A, A, None), "16-byte aligned")
    refused(lib.mshgnn_grad_norm(A, n, A, A + 8, None), "16-byte aligned")
    refused(lib.mshgnn_grad_norm(A, n, odd, A, None), "norm_out must be 8-byte aligned")
    refused(lib.mshgnn_grad_clip(None, n, A, 1.0, None), "bad argument to mshgnn_grad_clip")
    refused(lib.mshgnn_grad_clip(A, n, None, 1.0, None), "bad argument to mshgnn_grad_clip")
    refused(lib.mshgnn_grad_clip(A, 0, A, 1.0, None), "bad argument to mshgnn_grad_clip")
    refused(lib.mshgnn_grad_clip(A, n, A, -1.0, None), "max_norm must be >= 0")
    refused(lib.mshgnn_grad_clip(A, n, A, nan, None), "max_norm must be >= 0")
    refused(lib.mshgnn_grad_clip(odd, n, A, 1.0, None), "grads must be 16-byte aligned")
    refused(lib.mshgnn_grad_clip(A, n, odd, 1.0, None), "norm must be 8-byte aligned")
    assert math.isnan(nan) and C.sizeof(C.c_void_p) == 8
