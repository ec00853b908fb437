"""tests/metrics_reference.py on the host: for every case tests/test_metrics_exact_gpu.py runs, the checker accepts the reference's own result and rejects
every damage that has a meaning for the case (`damaged` returns None only where the defect cannot show by construction: it says where); every maker's
condition holds (the makers assert them: building the case is the check); the order mirror agrees with a thread-by-thread restatement in plain Python; and
the plain references agree with oracle/metrics_oracle.py, which stays the independent cross-check, to 1e-14."""
import math

import numpy as np
import pytest

from oracle import metrics_oracle as mo
from tests import metrics_reference as mr

CASES = mr.all_cases()


@pytest.mark.parametrize("family,key", CASES, ids=lambda v: v if isinstance(v, str) else "-".join(str(x) for x in v))
def test_the_checker_accepts_the_reference_and_rejects_every_damage(family, key):
    case = mr.build_case(family, key)
    d = mr.check(family, case, mr.expected(family, case))
    assert d is None, d
    told = 0
    for name in mr.DAMAGES[family]:
        wrong = mr.damaged(name, family, case)
        if wrong is None:
            continue
        assert mr.check(family, case, wrong) is not None, f"{family} {key}: the damage {name} passes the checker"
        told += 1
    assert told >= 3


def test_every_damage_is_told_by_the_smallest_and_the_largest_case_it_applies_to():
    """None is returned only for the stated reasons: each damage is live in at least one step case of its family, the smallest size included where the
    reason does not depend on the size."""
    for family in mr.DAMAGES:
        cases = [mr.build_case(f, k) for f, k in CASES if f == family and k[-1] == 0]
        for name in mr.DAMAGES[family]:
            assert any(mr.damaged(name, family, c) is not None for c in cases), (family, name)
    one = mr.build_case("cls", ("cls_case", 1, "step", 0))
    assert all(mr.damaged(n, "cls", one) is not None for n in mr.CLS_DAMAGES if n not in ("drop_partial",))
    one = mr.build_case("grf", ("grf_exact", 1, 0))
    assert all(mr.damaged(n, "grf", one) is not None for n in mr.GRF_DAMAGES if n != "fp32_sums")


def _plain_order_sum(terms, nt, blocks):
    """The summation order thread by thread, in Python floats."""
    items = len(terms)
    acc = [[0.0] * nt for _ in range(blocks)]
    for b in range(blocks):
        for t in range(nt):
            i = b * nt + t
            while i < items:
                for x in np.atleast_1d(terms[i]):
                    acc[b][t] += float(x)
                i += nt * blocks
    parts = []
    for b in range(blocks):
        waves = []
        for w in range(nt // 64):
            v = acc[b][64 * w:64 * w + 64]
            for m in (32, 16, 8, 4, 2, 1):
                v = [v[l] + v[l ^ m] for l in range(64)]
            assert len(set(v)) == 1
            waves.append(v[0])
        t = 0.0
        for x in waves:
            t += x
        parts.append(t)
    total = 0.0
    for x in parts:
        total += x
    return total


@pytest.mark.parametrize("items,per,nt,blocks", [(1, 1, 256, 1), (1000, 1, 256, 2), (777, 3, 256, 3), (2500, 1, 1024, 1), (1100, 2, 256, 2)])
def test_the_order_mirror_is_the_stated_order(items, per, nt, blocks):
    rng = np.random.default_rng(items)
    terms = rng.standard_normal((items, per)) * 10.0 ** rng.integers(-3, 4, (items, per))
    assert float(mr.order_sum(terms, nt, blocks)) == _plain_order_sum(terms, nt, blocks)


def test_the_launch_geometry_is_the_entry_points():
    assert [mr.geometry("reg", n) for n in (1, 4096, 4097, 8193, 262144, 262145, 10 ** 7)] == [(256, 1), (256, 1), (256, 2), (256, 3), (256, 64), (256, 64), (256, 64)]
    assert [mr.geometry("cls", B) for B in (1, 256, 257, 513, 16384, 16385)] == [(256, 1), (256, 1), (256, 2), (256, 3), (256, 64), (256, 64)]
    assert mr.geometry("com", 16643) == (256, 64) and mr.geometry("reg", 5000, "acc") == (1024, 1) and mr.geometry("cls", 3000, "acc") == (1024, 1)
    assert [mr.geometry("reg", n)[1] for n in mr.SCRATCH_SEQUENCE["reg"]] == [64, 1, 2, 64]
    assert [mr.geometry("cls", n)[1] for n in mr.SCRATCH_SEQUENCE["cls"]] == [64, 1, 2, 64] and mr.geometry("cls", mr.GRAPH_ITEMS["cls"])[1] == 3


def test_the_planted_classification_cells_are_there():
    for B in mr.CLS_B:
        case = mr.cls_case(B)
        want = mr.cls_expected(case)
        c = want["counts"]
        assert c[0] == B and c[2:].sum() == 4 * B
        if B % 2 == 1:
            assert c[6] == c[7] == c[8] == 0 and want["ce_b"][5] == 0.0              # leg 1: tn only -> F1 = 0/0 -> 0
            assert c[10] == 0 and want["ce_b"][6] == 0.0                             # leg 2: no tp
            if B > 1:
                assert c[11] > 0 and c[12] > 0                                       # ... but fp and fn
        if B >= 63:
            lg = case["logits"]
            gap = np.abs(lg[..., 1].astype(np.float64) - lg[..., 0])
            assert (gap == 0).any() and (gap == mr.GAP).any() and (gap == 0).all(axis=1).any() == (B >= 3)
            assert {0, 1, 2, -1} == set(np.unique(case["labels"]).tolist())
            assert (want["terms"] == mr.GAP).any() and (want["terms"] == 0.0).any()
        kept = mr.damaged("f1_nan_kept", "cls", case)
        assert (kept is not None and bool(np.isnan(kept["ce_b"]).any())) == (B % 2 == 1)


def test_the_references_agree_with_the_oracle():
    rng = np.random.default_rng(5)
    # regression
    case = mr.binade_reg(5000)
    want = mr.reg_expected(case)["batch"]
    mse, rmse, l1 = mo.regression_metrics(case["y"], case["pred"])
    assert abs(want[3] - mse) <= 1e-14 * mse and abs(want[4] - rmse) <= 1e-14 * rmse and abs(want[5] - l1) <= 1e-14 * l1
    # classification, labels in {0, 1} (the oracle indexes with them)
    B = 1000
    lg = (rng.standard_normal((B, 4, 2)) * 3).astype(np.float32)
    lab = rng.integers(0, 2, (B, 4)).astype(np.int32)
    terms, counts, _ = mr.cls_windows(lg, lab)
    c = counts.sum(axis=0)
    pub = mr.cls_published(math.fsum(terms.ravel()), c, B)
    o = mo.classification_metrics(lab, lg.reshape(B, 8))
    assert abs(pub[2] - o["ce"]) <= 2.0 ** -23 * o["ce"]                   # (both round the sum to fp32 before dividing: at most one fp32 step apart ...)
    assert abs(pub[0] / (4 * B) - _oracle_ce_sum(lg, lab) / (4 * B)) <= 1e-14          # (... and the fp64 sums agree)
    assert pub[3] == o["acc"] and list(pub[4:8]) == o["f1"]
    assert [list(c[2 + 4 * k:6 + 4 * k]) for k in range(4)] == o["counts"]
    # centroidal momentum
    nb = 4
    cc = mr.com_random(257, nb)
    v = mr.com_expected(cc)["batch"]
    o = mo.com_metrics(cc["y"], cc["pred"], nb, cc["mean"], cc["std"])
    assert abs(v[0] / v[2] - o["mse_lin"]) <= 1e-14 * o["mse_lin"] and abs(v[1] / v[3] - o["mse_ang"]) <= 1e-14 * o["mse_ang"]
    assert abs(v[4] / v[6] - o["cos_sim_lin"]) <= 1e-14 and abs(v[5] / v[6] - o["cos_sim_ang"]) <= 1e-14
    cos = mr.com_cosines(cc["pred"], cc["y"], nb, cc["mean"], cc["std"])
    assert abs(cos[:, 0].mean() - o["cos_sim_lin"]) <= 1e-14 and abs(cos[:, 1].mean() - o["cos_sim_ang"]) <= 1e-14
    # rotation
    g = mr.grf_random(1000)
    assert np.abs(mr.grf_rotate(g["quat"], g["body"]) - mo.body_frame_to_world_frame(g["quat"], g["body"])).max() <= 1e-14 * 200
    assert np.abs(np.asarray(g["want"], dtype=np.float64) - mo.body_frame_to_world_frame(g["quat"], g["body"])).max() <= 1e-14 * 200


def _oracle_ce_sum(lg, lab):
    l, _, _ = mo.classification_useful_values(lg.reshape(-1, 8), lg.shape[0])
    lse = np.log(np.exp(l - l.max(axis=1, keepdims=True)).sum(axis=1)) + l.max(axis=1)
    return float((lse - l[np.arange(l.shape[0]), lab.reshape(-1)]).sum())


def test_the_cosine_bound_sees_an_fp32_step_and_holds_for_fp64():
    """The fp64 evaluation of every window lies within its bound of the extended-precision value (the bound is not too tight for a correct kernel), and an
    fp32 evaluation lies far outside (it is not too loose to matter)."""
    for B, nb in ((257, 4), (16385, 1)):
        case = mr.com_random(B, nb)
        ext = mr.com_cosines(case["pred"], case["y"], nb, case["mean"].astype(mr.EXT), case["std"].astype(mr.EXT), dtype=mr.EXT)
        f64 = mr.com_cosines(case["pred"], case["y"], nb, case["mean"], case["std"])
        f32 = mr.com_cosines(case["pred"], case["y"], nb, case["mean"], case["std"], dtype=np.float32)
        assert (np.abs(f64 - ext) <= case["window_bound"]).all()
        assert np.median(np.abs(f32.astype(mr.EXT) - ext).astype(np.float64) / case["window_bound"]) > 1e4


def test_the_rotation_bound_holds_for_fp64_and_the_exact_cases_tell_the_conventions_apart():
    g = mr.grf_random(1000)
    got = mr.grf_rotate(g["quat"], g["body"]).astype(np.float32)
    assert mr.grf_check(g, got) is None
    e = mr.grf_exact(1)
    R = mr.rotation_matrices(e["quat"])[0]
    assert not np.array_equal(R, R.T) and not np.array_equal(R, mr.rotation_matrices(e["quat"], scalar_first=True)[0])
    assert np.array_equal(mr.grf_rotate(e["quat"], e["body"]), mr.grf_rotate(-e["quat"], e["body"]))
