"""CPU: the host-side proofs behind tests/test_mlp_x3_exact_gpu.py (tests/mlp_x3_reference.py), per (family, shape, batch) of its matrix, and the library's
host-side answers for the split plan.
Closure: the fp64 three-product emulation equals the fp64 reference bit for bit, every stored value is hi + lo exactly, every result is an fp32 value, every
product has a factor with lo = 0 and every accumulation fits 2^24 units of its grid.  Coverage: the operand classes a family names carry non-zero lo halves,
and between them the families widen X, every A_l, every dZ_l, the input image, a hidden image and the output image with their transposes.  Damaged variants:
a dropped lo hi term is caught in every wide family, a dropped hi lo term in every wide family but wide_dz (no wide right-hand factor there), exchanged
planes of the input-layer stash in every family."""
import pytest
import torch

from tests import mlp_reference as mr
from tests import mlp_x3_reference as xr

CASES = [(row[:5], B) for row in mr.EXACT_MATRIX for B in row[5]]


@pytest.mark.parametrize("shape,B", CASES, ids=[f"in{s[0]}_T{s[1]}_h{s[2]}_L{s[3]}_o{s[4]}_B{B}" for s, B in CASES])
def test_families_are_closed_cover_every_operand_class_and_catch_the_damaged_variants(shape, B):
    L = shape[3]
    covered, caught = set(), {}
    for family in xr.FAMILIES:
        case = xr.family_case(family, *shape, B)
        if case is None:
            assert family == "wide_w2" and L == 2
            continue
        for key in ("gout_mse", "gout"):      # (ref, wide: the last one, for gout)
            ref, wide = xr.check_family(case, key)
        assert xr.named_classes(family, L) <= wide, (family, xr.named_classes(family, L) - wide)
        if family == "narrow":
            assert not wide
        covered |= wide
        good = xr.emulate_x3(case["params"], case["x"], gout=case["gout"])
        assert mr.compare(ref, good["out"], good["acts"][0], good["grads"]) == []
        for name, res in xr.damaged_variants(case):
            caught[(family, name)] = bool(mr.compare(ref, res["out"], res["acts"][0], res["grads"]))
    assert xr.all_classes(L) <= covered, xr.all_classes(L) - covered
    families = [f for f in xr.FAMILIES if (f, "swap") in caught]
    for f in families:
        assert caught[(f, "swap")], f
        if f != "narrow":
            assert caught[(f, "lo_hi")], f
            assert caught[(f, "hi_lo")] == (f != "wide_dz"), f
    assert not caught[("narrow", "lo_hi")] and not caught[("narrow", "hi_lo")]      # (lo = 0 everywhere: nothing to drop)


def test_split_is_two_roundings_to_nearest_and_hi_zero_implies_lo_zero():
    g = torch.Generator().manual_seed(1)
    v = torch.cat([torch.randn(4096, generator=g), torch.randn(4096, generator=g) * 1e-30, torch.zeros(3)]).double()
    hi, lo = xr.split(v)
    assert mr.is_bf16(hi) and mr.is_bf16(lo)
    assert bool(((hi + lo - v).abs() <= v.abs() * 2.0 ** -16).all())
    assert not bool(((hi == 0) & (lo != 0)).any())


def test_emulation_stays_near_fp64_on_random_fp32_data():
    c = mr.random_case(450, 128, 8, 3, 64, seed=2)
    x = torch.randn(64, 450, generator=torch.Generator().manual_seed(3), dtype=torch.float64).float().double()
    ref, em = mr.reference(c["params"], x, loss="mse", target=c["y"]), xr.emulate_x3(c["params"], x, loss="mse", target=c["y"])
    assert 0 < mr.rel_max(em["out"], ref["out"]) < 1e-4
    for (a, b), (ra, rb) in zip(em["grads"], ref["grads"]):
        assert mr.rel_l2(a, ra) < 1e-4 and mr.rel_l2(b, rb) < 1e-4
    masks = [a > 0 for a in ref["acts"]]
    dec = xr.reference_with_decisions(c["params"], x, masks, loss="mse", target=c["y"])
    assert mr.rel_max(dec["out"], ref["out"]) < 1e-12 and abs(float(dec["loss"]) - float(ref["loss"])) < 1e-12 * float(ref["loss"])
    for (a, b), (ra, rb) in zip(dec["grads"], ref["grads"]):
        assert mr.rel_l2(a, ra) < 1e-12 and mr.rel_l2(b, rb) < 1e-12


def test_library_takes_the_split_plan_on_the_host():
    from morphsym_hgnn_amd import engine
    info = engine.mlp_compile_host(450, 128, 4, 3, dtype="x3")
    ref = engine.mlp_compile_host(450, 128, 4, 3, dtype="bf16")
    assert info.n_flat == ref.n_flat and info.rows_per_tile == 32 and info.n_launches_step == 5
    assert list(info.off_w) == list(ref.off_w) and list(info.off_b) == list(ref.off_b)
    assert ref.lds_bytes == 2 * 32 * (128 + 8) * 2 + 32 * 16 * 4 + 256 * 4      # the bf16 descriptor's answer is unchanged
    assert info.lds_bytes == 2 * 2 * 32 * (128 + 8) * 2 + 32 * 16 * 4 + 256 * 4
    big = engine.mlp_compile_host(16384, 512, 16, 16, dtype="x3")
    assert big.lds_bytes == 2 * 2 * 32 * (512 + 8) * 2 + 32 * 16 * 4 + 256 * 4 <= 163840
    with pytest.raises(engine.MshgnnError, match="bf16"):
        engine.mlp_compile_host(450, 128, 4, 3, dtype="f32")
    with pytest.raises(engine.MshgnnError, match="hidden must be"):
        engine.mlp_compile_host(450, 64, 4, 3, dtype="x3")
