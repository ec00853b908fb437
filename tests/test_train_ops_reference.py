"""tests/train_ops_reference.py polices itself on the host (no GPU): the fp64 references agree with torch's own Adam and cross entropy in fp64, the
exact cases close, the positive-control emulations pass every checker of every case of the GPU tables -- and every deliberately damaged result is
REJECTED by every one of them (no share of cases left out: a case whose checker cannot see a damage has to be an exact-data or sparse-data case)."""
import math

import numpy as np
import pytest
import torch

from tests import train_ops_reference as tr

CE_K = 4.0          # the host controls use a generous ULP figure for expf / logf: a damage the checker rejects at K = 4 is rejected at any smaller K


@pytest.mark.parametrize("hp_i", range(len(tr.ADAM_HP)))
def test_adam_reference_is_torch_adam_in_fp64(hp_i):
    """Five steps of torch.optim.Adam on fp64 tensors with the same fp32-valued hyperparameters (the gradient pre-multiplied by grad_scale in fp64)."""
    b1, b2, eps, s, lr = hp = tr.hp32(tr.ADAM_HP[hp_i])
    gen = torch.Generator().manual_seed(hp_i)
    p = torch.randn(300, generator=gen)
    q = p.double().clone().requires_grad_(True)
    opt = torch.optim.Adam([q], lr=lr, betas=(b1, b2), eps=eps)
    p64, m64, v64 = p.double(), torch.zeros(300, dtype=torch.float64), torch.zeros(300, dtype=torch.float64)
    for t in range(1, 6):
        g = torch.randn(300, generator=gen)
        g[::5] = 0.0
        q.grad = g.double() * s
        opt.step()
        p64, m64, v64 = tr.adam_reference(p64, g, m64, v64, t, hp)      # (fp64 state carried from step to step: the reference widens, it never rounds)
        st = opt.state[q]
        assert float((p64 - q.detach()).abs().max()) <= 1e-13 * float(q.detach().abs().max()), t
        assert float((m64 - st["exp_avg"]).abs().max()) <= 1e-15 and float((v64 - st["exp_avg_sq"]).abs().max()) <= 1e-15, t
    assert int(opt.state[q]["step"]) == 5 and bool((m64[::5] == 0).all()) and torch.equal(p64[::5], p.double()[::5])      # zero gradients: nothing moves


def test_ce_and_mse_references_are_torch_in_fp64():
    for rows in (1, 7, 300):
        case = tr.ce_case(rows, "random")
        l = case["logits"].double().requires_grad_(True)
        lab = (case["labels"] != 0).long()
        loss = torch.nn.functional.cross_entropy(l, lab, reduction="sum") / rows
        loss.backward()
        assert abs(float(loss.detach()) - case["loss"]) <= 1e-14 * max(1.0, case["loss"]) and float((l.grad - case["grad"]).abs().max()) <= 1e-15
        assert set(case["labels"].tolist()) <= {0, 1, -1, 7}
    case = tr.mse_case(257, "random")
    o = case["out"].double().requires_grad_(True)
    loss = torch.nn.functional.mse_loss(o, case["y"].double())
    loss.backward()
    assert abs(float(loss.detach()) - case["loss"]) <= 1e-15 * case["loss"] and float((o.grad - case["grad"]).abs().max()) <= 1e-17


def test_exact_adam_case_closes_and_refuses_data_that_does_not():
    for n in tr.ADAM_EXACT_N:
        case = tr.adam_exact_case(n)
        live = case["g"] != 0
        assert bool(live.any()) and bool((~live).any())
        assert torch.equal(case["ref_m"], case["g"].double() / 2) and torch.equal(case["ref_v"], case["g"].double() ** 2 / 4)
        got = tr.adam_emulation(case["p"], case["g"], case["m"], case["v"], 1, case["hp"])
        assert tr.adam_check(case, *got) is None
        for how in ("fp32", "fp64"):      # at t = 1 both ways of forming the corrections give the same factors
            assert tr._factors(0.5, 0.75, 1, how) == (0.5, 0.5)
    assert not tr._is_f32(torch.tensor([1.0 + 2.0 ** -30], dtype=torch.float64))
    with pytest.raises(tr.DoesNotClose):
        tr.mse_case(262145, "exact")
    with pytest.raises(tr.DoesNotClose):
        tr.ce_case(6, "exact_equal")


def test_fp32_bias_corrections_are_the_defect_the_bounds_see():
    """1 - powf(0.999f, 2) keeps 17 bits: 1 / sqrt(bc2) is off by tens of u, and the checker rejects the result at the first probe."""
    dev = tr.bc_deviation(tr.hp32(tr.ADAM_HP[0]), 2, "fp32")
    assert dev > 30, dev
    case = tr.adam_case(1, 2, 0)
    assert tr.damaged_adam(case, "bc_fp32") is not None
    assert tr.bc_deviation(tr.hp32(tr.ADAM_HP[0]), 1, "fp32") == 0.0 and tr.bc_deviation(tr.hp32(tr.ADAM_HP[0]), 100000, "fp32") == 0.0


@pytest.mark.parametrize("key", tr.all_adam_cases(), ids=lambda k: "-".join(str(v) for v in k))
def test_adam_checker_accepts_the_control_and_rejects_every_damage(key):
    case = tr.build_adam_case(key)
    n = case["n"]
    if not case["exact"]:      # the data is what the docstring says
        b1, b2, eps, s, lr = case["hp"]
        for x in ((case["g"].double() * s).abs(), case["m"].double().abs(), case["v"].double().sqrt()):
            nz = x[x != 0]
            assert nz.numel() == 0 or (float(nz.min()) >= 1e-12 and float(nz.max()) <= 1e3)
        z = case["zero"]
        assert not bool((case["g"][z] != 0).any() | (case["m"][z] != 0).any() | (case["v"][z] != 0).any()) and (n < 4 or bool(z.any()))
    good = tr.adam_emulation(case["p"], case["g"], case["m"], case["v"], case["t"], case["hp"])
    d = tr.adam_check(case, *good)
    assert d is None, f"the fp32 emulation with fp64-formed bias corrections fails: {d}"
    ref = tr.adam_reference(case["p"], case["g"], case["m"], case["v"], case["t"], case["hp"])
    assert tr.adam_check(case, *(x.float() for x in ref)) is None, "the rounded reference fails its own checker"
    if not case["exact"]:
        em, ev, ep = tr.adam_error_units(case, *good)
        assert em <= 5 and ev <= 8 and ep <= 8, (em, ev, ep)
    seen = []
    for kind in tr.ADAM_DAMAGES:
        bad = tr.damaged_adam(case, kind)
        if bad is None:
            continue
        seen.append(kind)
        assert tr.adam_check(case, *bad) is not None, f"{kind} passes the checker of {key}"
    # the damages that must exist for this case do
    want = {"eps_inside_sqrt"}
    if n % 4:
        want.add("tail_untouched")
    if n > tr.SWEEP:
        want.add("second_sweep_untouched")
    if n >= 2:
        want.add("neighbour_gradient")
    if n >= 4:
        want.add("zero_element_moved")
    if case["hp"][3] != 1.0:
        want.add("grad_scale_ignored")
    if key[0] == "random" and key[2] == 2 and key[3] == 0:
        want.add("bc_fp32")
    if key[0] == "exact" or key[2] in (2, 3, 10):
        want.add("bc_dropped")
    assert want <= set(seen), (want - set(seen), key)


def test_adam_tables_hold_what_the_issue_names():
    keys = tr.all_adam_cases()
    assert {k[1] for k in keys if k[0] == "random"} >= set(tr.ADAM_N) and tr.ADAM_N[8:] == [tr.S, tr.S + 1, tr.S + 4, tr.S + 1027, 2 * tr.S + 5] and tr.S == 2097152
    for n in tr.ADAM_T_AT:
        assert {(k[2], k[3]) for k in keys if k[0] == "random" and k[1] == n} >= {(t, h) for t in tr.ADAM_T for h in range(3)}
    assert [n for n, _ in tr.MSE_CASES] == [1, 63, 64, 65, 255, 256, 257, 262145, 2 ** 18, 2 ** 19]
    assert {n for n, _ in tr.CE_CASES} >= {1, 63, 64, 65, 255, 256, 257, 262145, 2 ** 18, 2 ** 19}


@pytest.mark.parametrize("n,kind", tr.MSE_CASES)
def test_mse_checker_accepts_the_control_and_rejects_every_damage(n, kind):
    case = tr.mse_case(n, kind)
    d32 = case["out"] - case["y"]
    inv = np.float32(1.0) / np.float32(n)
    good = (float(np.float32(float((d32 * d32).double().sum())) * inv), d32 * 2.0 * float(inv))      # fp32 operations; the sum in any order: fp64, rounded once
    assert tr.mse_check(case, *good) is None and tr.mse_check(case, good[0], None) is None
    assert tr.mse_check(case, f32r(case["loss"]), case["grad"].float()) is None
    seen = []
    for dmg in tr.LOSS_DAMAGES:
        bad = tr.damaged_mse(case, dmg)
        if bad is None:
            continue
        seen.append(dmg)
        assert tr.mse_check(case, bad[0], bad[1].float()) is not None, f"{dmg} passes the checker of MSE {n} {kind}"
    assert set(seen) >= {"drop_one_term", "one_over_n_minus_1"} | ({"swap_gradient_pair"} if n >= 2 else set()), seen
    assert tr.order_bound(case) == 0.0 if (n <= 256 or case["exact"]) else tr.order_bound(case) > 0.0


def f32r(x):
    return float(np.float32(x))


@pytest.mark.parametrize("rows,kind", tr.CE_CASES)
def test_ce_checker_accepts_the_control_and_rejects_every_damage(rows, kind):
    case = tr.ce_case(rows, kind)
    good = tr.ce_emulation(case["logits"], case["labels"])
    for K in (1.0, CE_K):
        d = tr.ce_check(case, *good, K)
        assert d is None, d
    assert tr.ce_check(case, good[0], None, CE_K) is None
    assert tr.ce_needed_ulp(case, *good) <= 1.0
    if kind != "random":
        t = case["terms"]
        nz = t != 0
        assert int(nz.sum()) == (tr.SPARSE_TERMS if rows >= 32 else (rows + 1) // 2)
        assert bool((t[nz] == tr.GAP).all()) if kind != "exact_equal" else bool(((t[nz] - math.log(2.0)).abs() < 1e-15).all())
        g = case["grad"][nz]
        assert bool((g.abs() == (1.0 if kind != "exact_equal" else 0.5) / rows).all()) and bool((case["grad"][~nz] == 0).all())
    seen = []
    for dmg in tr.LOSS_DAMAGES:
        bad = tr.damaged_ce(case, dmg)
        if bad is None:
            continue
        seen.append(dmg)
        assert tr.ce_check(case, bad[0], bad[1].float(), CE_K) is not None, f"{dmg} passes the checker of CE {rows} {kind}"
    want = {"drop_one_term", "one_over_n_minus_1", "swap_gradient_pair"}
    if float(case["logits"].max()) > 88.0:
        assert kind != "random"
        want.add("no_max_subtraction")
    if rows >= 63:
        want.add("label_equals_1")
    assert want <= set(seen), (want - set(seen), rows, kind)
