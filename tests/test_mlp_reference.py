"""CPU: the host-side proofs behind tests/test_mlp_exact_gpu.py, per (shape, batch) of its matrix and the seed it uses (tests/mlp_reference.py):
closure (every activation and activation gradient is a bf16 value, every accumulation fits 2^24 units of its finest grid, the emulation with and without
rounding equals the fp64 reference bit for bit), coverage (every input column meets a non-zero weight and a non-zero dW_1 entry, every 32-column slice of
every hidden activation is non-zero, every layer has exact-zero pre-activations, every parameter tensor has a non-zero gradient) and that every damaged
variant -- a dropped K chunk, a dropped row tile, a transposed weight, a skipped bias -- is caught by the checker.
One seed closes every row of the matrix: no row is omitted.
For the cross-entropy cases of tests/test_exact_ce_gpu.py (mlp_reference.CE_MATRIX: the last layer times 2^7, so that every logit pair is a tie or saturated and
the loss tail's fp32 softmax gradient is exact) the same closure and coverage with that gradient, and the coverage of labels and regimes of check_exact_ce."""
import pytest
import torch

from tests import mlp_reference as mr

CASES = [(row[:5], B) for row in mr.EXACT_MATRIX for B in row[5]]


@pytest.mark.parametrize("shape,B", CASES, ids=[f"in{s[0]}_T{s[1]}_h{s[2]}_L{s[3]}_o{s[4]}_B{B}" for s, B in CASES])
def test_exact_case_is_closed_covered_and_its_damaged_variants_are_caught(shape, B):
    case = mr.exact_case(*shape, B)
    assert int(case["starts"][0]) == 0 and int(case["starts"][-1]) == case["series"].shape[0] - shape[1]      # row 0 and the last valid row
    for key in ("gout_mse", "gout"):      # (ref: the last one, for gout)
        ref = mr.check_exact(case, key)
    good = mr.emulate(case["params"], case["x"], gout=case["gout"])
    assert mr.compare(ref, good["out"], good["acts"][0], good["grads"]) == []
    names = []
    for name, res in mr.damaged_variants(case):
        assert mr.compare(ref, res["out"], res["acts"][0], res["grads"]), f"the checker does not see the damaged variant '{name}'"
        names.append(name)
    assert {"k_chunk", "row_tile", "skip_bias"} <= set(names) and ("transpose" in names) == (shape[3] > 2)


def test_mse_targets_give_the_dyadic_gradient_the_fused_tail_computes():
    case = mr.exact_case(35, 7, 128, 3, 4, 17)
    out = mr.reference(case["params"], case["x"])["out"].float()
    inv = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(out.numel()), dtype=torch.float32)
    g = (torch.tensor(2.0) * (out - case["y"].float()) * inv).double()
    assert torch.equal(g, case["gout_mse"]) and bool((case["gout_mse"] != 0).any())


def test_emulation_rounds_on_random_data_and_stays_near_fp64():
    c = mr.random_case(450, 128, 8, 3, 64, seed=2)
    ref, em, em0 = mr.reference(c["params"], c["x"], loss="mse", target=c["y"]), mr.emulate(c["params"], c["x"], loss="mse", target=c["y"]), \
        mr.emulate(c["params"], c["x"], loss="mse", target=c["y"], quant=False)
    assert mr.rel_max(em0["out"], ref["out"]) < 1e-12 and abs(float(em0["loss"]) - float(ref["loss"])) < 1e-12 * float(ref["loss"])
    for (a, b), (ra, rb) in zip(em0["grads"], ref["grads"]):
        assert mr.rel_l2(a, ra) < 1e-12 and mr.rel_l2(b, rb) < 1e-12
    err = mr.rel_max(em["out"], ref["out"])
    assert 1e-5 < err < 2e-2, err


CE_IDS = [f"in{s[0]}_T{s[1]}_h{s[2]}_L{s[3]}_o{s[4]}_B{B}" for s, B, _, _, _ in mr.CE_MATRIX]


@pytest.mark.parametrize("shape,B,seed,share,ties", mr.CE_MATRIX, ids=CE_IDS)
def test_ce_case_is_closed_and_covered_and_a_damaged_tail_is_caught(shape, B, seed, share, ties):
    case = mr.ce_case(shape, B, seed, share)
    ref = mr.check_exact_ce(case, ties)
    c = case["counts"]
    assert case["ce_gout_err"] <= 2.0 ** -149 and (c["ties"] > 0) == ties and c["right"] > 0 and c["wrong"] > 0 and ref["loss"] == case["loss_ce"] > 0
    good = mr.emulate(case["params"], case["x"], gout=case["gout_ce"])
    assert mr.compare(ref, good["out"], good["acts"][0], good["grads"]) == []
    g = case["gout_ce"]
    damaged = {"the two logits' gradients exchanged on one pair": torch.cat((g[:, :2].flip(-1), g[:, 2:]), 1),
               "the row count of a 64-row sub-step": g * (g.numel() // 2) / (64 * shape[4] // 2),
               "one 16-row tile left out": torch.cat((g[:-16], torch.zeros_like(g[-16:]))),
               "one pair's labels from the next row": torch.cat((torch.roll(g[:, :2] , -1, 0), g[:, 2:]), 1)}
    for name, gd in damaged.items():
        res = mr.emulate(case["params"], case["x"], gout=gd)
        assert mr.compare(ref, res["out"], res["acts"][0], res["grads"]), name
    print(f"\n{shape} B={B}: seed {seed}, wrong share {share}: ties / right / wrong = {c['ties']} / {c['right']} / {c['wrong']}, loss {case['loss_ce']!r}")


def test_ce_matrix_rows_have_a_power_of_two_of_logit_pairs():
    rows = {c[0] for c in mr.CE_MATRIX}
    assert all(r in {row[:5] for row in mr.EXACT_MATRIX} and r[4] in (4, 8) for r in rows)
    assert {(35, 7, 128, 3, 4), (450, 150, 128, 3, 4)} <= rows and all({(r, 16), (r, 1024)} <= {c[:2] for c in mr.CE_MATRIX} for r in rows)
    assert not set(mr.CE_LEFT_OUT) & {c[:2] for c in mr.CE_MATRIX}
