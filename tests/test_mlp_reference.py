"""CPU: the host-side proofs behind tests/test_mlp_exact_gpu.py, per (shape, batch) of its matrix and the seed it uses (tests/mlp_reference.py):
closure (every activation and activation gradient is a bf16 value, every accumulation fits 2^24 units of its finest grid, the emulation with and without
rounding equals the fp64 reference bit for bit), coverage (every input column meets a non-zero weight and a non-zero dW_1 entry, every 32-column slice of
every hidden activation is non-zero, every layer has exact-zero pre-activations, every parameter tensor has a non-zero gradient) and that every damaged
variant -- a dropped K chunk, a dropped row tile, a transposed weight, a skipped bias -- is caught by the checker.
One seed closes every row of the matrix: no row is omitted."""
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
