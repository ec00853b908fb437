"""Per-segment centroidal-momentum sums on the GPU (mshgnn_metrics_com_segmented, metrics.SegmentedComMetrics) against the numpy mirror
`metrics.com_segmented_reference` (tests/test_com_symmetry.py pins that to the reference's metric code).

EXACT DATA.  y / y_pred are multiples of 2^-6 in [-4, 4]: a difference is a multiple of 2^-6 of magnitude <= 8, its square a multiple of 2^-12 <= 64, and a
sum of 4099 * 12 of them stays below 2^22 -- 34 significant bits, every fp64 addition exact in any order, fused or not.  y_std are powers of two and y_mean
is dyadic, so v = x * std + mean is exact; base node 0's lin and ang vectors are, after un-standardising, zero or on one axis with a length in {1/2, 1}: the
sum of squares is one exact square, its root exact, v / |v| is +-1 or 0 and a zero vector meets the clamp (0 / 1e-8 = 0).  Every cosine is -1, 0 or 1 and
the cosine sums are small integers.  The state must equal the mirror bit for bit.

RANDOM DATA.  u = 2^-53, gamma_k = k u / (1 - k u) (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2).  The mirror forms every term in
numpy fp64 with the kernel's operations and adds a segment's terms with math.fsum (the correctly rounded sum); the kernel may fuse a multiply into the add
that follows it and adds in SOME fixed order (a lane's terms, the butterfly over a wave, the entries of the merge, the state).
  * squared errors, a half of a segment of n windows: m = 3 n_bases n terms d * d >= 0.  d is the same fp64 value on both sides (the difference of two fp32
    numbers); the kernel's term carries at most the one rounding of the product (none when fused), any order of m - 1 additions gamma_(m - 1) sum |terms|, the
    mirror's sum one rounding: |state - mirror| <= gamma_(m + 4) sum terms, the bound tests/test_segmented_metrics_gpu.py uses.
  * cosines: tests/metrics_reference.py's `com_window_bound` bounds one window's fp64 cosine, fused or not, against its true value (2 (|dp|_1 / |p| +
    |dy|_1 / |y|) for the un-standardising, 12 u for the arithmetic behind it); kernel and mirror are both within it, so a window's two values differ by at
    most twice that, and the n-term sums add gamma_(n + 4) sum |cos|: |state - mirror| <= 2 sum window_bound + gamma_(n + 4) sum |cos|.
The counts ([2], [3], [6]) are exact."""
import ctypes as C

import numpy as np
import pytest
import torch

from morphsym_hgnn_amd import metrics as M
from tests import metrics_reference as mr

pytestmark = pytest.mark.gpu
EINVAL = -1
SENTINEL = 123.25
BATCHES = [1, 63, 64, 65, 257, 1088, 4099]          # 1088 = 17 slots of 64 entries under all-distinct ids: more than the merge's stage of 512
PATTERNS = ("runs", "shuffled", "equal", "distinct", "overflow")


def _ids(pattern, B, seed):
    """(int32 [B], n_segments) of an id arrangement the kernel must be right for"""
    rng = np.random.default_rng(seed)
    if pattern == "equal":
        return np.full(B, 2, dtype=np.int32), 3
    if pattern == "runs":          # sorted runs whose borders fall inside a wave: run lengths 1, 37, 64, 100, ...
        out, k = [], 0
        while len(out) < B:
            out += [k % 5] * (1, 37, 64, 100)[k % 4]
            k += 1
        return np.asarray(sorted(out[:B]), dtype=np.int32), 5
    if pattern == "distinct":      # every window its own id, in order: 64 entries in every slot
        return np.arange(B, dtype=np.int32), B + 3
    if pattern == "shuffled":      # every window its own id, shuffled: a merging thread's ids arrive interleaved
        return rng.permutation(B).astype(np.int32), B
    assert pattern == "overflow"   # in-range ids mixed with ids on every side of the range
    n_seg = 6
    out = rng.integers(-2, n_seg + 3, B).astype(np.int64)
    edge = [-1, n_seg, 2 ** 31 - 1, -(2 ** 31), 0, n_seg - 1]
    out[:min(B, len(edge))] = edge[:min(B, len(edge))]
    return out.astype(np.int32), n_seg


MEAN = np.array([0.25, -0.5, 0.0, 0.5, -0.25, 0.0])
STD = np.array([0.5, 1.0, 2.0, 2.0, 0.5, 1.0])


def _exact_pair(B, nb, seed):
    rng = np.random.default_rng(seed)
    y, yp = (rng.integers(-256, 257, (B, nb, 6)).astype(np.float64) / 64.0 for _ in range(2))
    for x in (y, yp):          # base node 0: un-standardised vectors that are zero or +-1/2, +-1 on one axis
        v = np.zeros((B, 6))
        for h in range(2):
            axis = rng.integers(0, 3, B)
            length = rng.choice([0.0, 0.5, -0.5, 1.0, -1.0], B)
            v[np.arange(B), 3 * h + axis] = length
        x[:, 0, :] = (v - MEAN) / STD
    assert (np.abs(y) <= 4).all() and (np.abs(yp) <= 4).all() and (y * 64 == np.round(y * 64)).all() and (yp * 64 == np.round(yp * 64)).all()
    _, cos = M.com_window_terms(y, yp, nb, MEAN, STD)
    assert np.isin(cos, [-1.0, 0.0, 1.0]).all()
    if B >= 63:
        assert all((cos == c).any() for c in (-1.0, 0.0, 1.0))
    return torch.from_numpy(y.astype(np.float32)).reshape(B, nb * 6), torch.from_numpy(yp.astype(np.float32)).reshape(B, nb * 6)


def _guarded(m):
    """The metrics' state moved into a buffer with one row more: (the buffer, its sentinel row)"""
    big = torch.zeros(m.n_segments + 2, 8, dtype=torch.float64, device="cuda")
    big[m.n_segments + 1] = SENTINEL
    m.state = big[:m.n_segments + 1]
    return big, big[m.n_segments + 1]


@pytest.mark.parametrize("B", BATCHES)
def test_exact_sums_equal_the_mirror_bit_for_bit(B):
    for nb in (1, 2, 4):
        y, yp = _exact_pair(B, nb, 100 * B + nb)
        y2, yp2 = _exact_pair(B, nb, 100 * B + nb + 7)
        for i, pattern in enumerate(PATTERNS):
            seg, n_seg = _ids(pattern, B, B + i)
            m = M.SegmentedComMetrics(n_seg, nb, MEAN, STD)
            big, guard = _guarded(m)
            m.update(y.cuda(), yp.cuda(), torch.from_numpy(seg).cuda())
            want = M.com_segmented_reference(y, yp, seg, n_seg, nb, MEAN, STD)
            assert torch.equal(m.state.cpu(), torch.from_numpy(want)), (nb, pattern)
            seg2 = np.roll(seg, 11)          # a second call on other data and another arrangement accumulates (same scratch: the ticket was reset)
            m.update(y2.cuda(), yp2.cuda(), torch.from_numpy(seg2).cuda())
            want2 = want + M.com_segmented_reference(y2, yp2, seg2, n_seg, nb, MEAN, STD)
            assert torch.equal(m.state.cpu(), torch.from_numpy(want2)), (nb, pattern, "second call")
            assert bool((guard == SENTINEL).all()), "the row behind the overflow row was written"
            bad = 2 * int(((seg < 0) | (seg >= n_seg)).sum())
            assert m.overflow() == bad == int(want2[n_seg, 6]) and float(want2[:, 6].sum()) == 2 * B
            if bad:
                with pytest.raises(IndexError):
                    m.check()
            else:
                m.check()
            t = m.table()
            assert torch.equal(t["n"].cpu(), torch.from_numpy(want2[:n_seg, 6]))
            full = want2[:n_seg, 6] > 0          # (an empty segment's means are 0 / 0)
            assert np.array_equal(t["MSE"].cpu().numpy()[full], (want2[:n_seg, 0] + want2[:n_seg, 1])[full] / (want2[:n_seg, 2] + want2[:n_seg, 3])[full])
            assert np.array_equal(t["cos_sim_lin"].cpu().numpy()[full], want2[:n_seg, 4][full] / want2[:n_seg, 6][full])
            m.reset()
            assert not bool(m.state.any())


def _random_case(B, nb, seed):
    g = torch.Generator().manual_seed(seed)
    y, yp = torch.randn(B, nb * 6, generator=g), torch.randn(B, nb * 6, generator=g)
    mean, std = torch.randn(6, generator=g).double().numpy(), (torch.rand(6, generator=g).double() + 0.5).numpy()
    return y, yp, mean, std


def _bounds(y, yp, seg, n_seg, nb, mean, std):
    """[n_seg + 1][8]: the module docstring's bound per slot (0: exact)"""
    sq, cos = M.com_window_terms(y, yp, nb, mean, std)
    wb = mr.com_window_bound(yp.numpy(), y.numpy(), nb, mean, std)
    row = np.where((seg >= 0) & (seg < n_seg), seg, n_seg)
    bound = np.zeros((n_seg + 1, 8))
    for s in range(n_seg + 1):
        g = row == s
        n = int(g.sum())
        if n:
            m = 3 * nb * n
            bound[s, 0], bound[s, 1] = mr.gamma(m + 4) * sq[g][:, :, :3].sum(), mr.gamma(m + 4) * sq[g][:, :, 3:].sum()
            for h in range(2):
                bound[s, 4 + h] = 2.0 * wb[g, h].sum() + mr.gamma(n + 4) * np.abs(cos[g, h]).sum()
    return bound


@pytest.mark.parametrize("B,nb,pattern", [(4099, 4, "runs"), (4099, 1, "shuffled"), (1088, 2, "distinct"), (257, 4, "overflow"), (65, 2, "equal"), (1, 1, "equal")])
def test_rounded_sums_are_within_the_bound_and_reproducible(B, nb, pattern):
    y, yp, mean, std = _random_case(B, nb, 31 * B + nb)
    seg, n_seg = _ids(pattern, B, 5)
    want = M.com_segmented_reference(y, yp, seg, n_seg, nb, mean, std)
    states = []
    for _ in range(2):
        m = M.SegmentedComMetrics(n_seg, nb, mean, std)
        m.update(y.cuda(), yp.cuda(), torch.from_numpy(seg).cuda())
        states.append(m.state.cpu())
    assert torch.equal(states[0], states[1])          # the reproducibility claim: the same call twice, the same bits
    got = states[0].numpy()
    assert np.array_equal(got[:, [2, 3, 6, 7]], want[:, [2, 3, 6, 7]])
    bound = _bounds(y, yp, seg, n_seg, nb, mean, std)
    err = np.abs(got - want)
    print(f"B {B} nb {nb} {pattern}: worst error / bound {np.max(err[:, [0, 1, 4, 5]] / np.maximum(bound[:, [0, 1, 4, 5]], 1e-300)):.3e}")
    assert (err <= bound).all(), (err.max(), np.argwhere(err > bound)[:4])


def test_one_scratch_serves_calls_of_different_batch_sizes():
    """The ticket is reset and no slot of an earlier, larger call is read: 4099, 65, 1, 257, 4099 windows through one SegmentedComMetrics."""
    nb = 2
    m = None
    want = None
    for k, B in enumerate((4099, 65, 1, 257, 4099)):
        y, yp = _exact_pair(B, nb, 900 + k)
        seg, n_seg = _ids("overflow", B, k)
        if m is None:
            m, want = M.SegmentedComMetrics(n_seg, nb, MEAN, STD), np.zeros((n_seg + 1, 8))
        m.update(y.cuda(), yp.cuda(), torch.from_numpy(seg).cuda())
        want = want + M.com_segmented_reference(y, yp, seg, n_seg, nb, MEAN, STD)
        assert torch.equal(m.state.cpu(), torch.from_numpy(want)), B
    assert m._scratch.numel() * 8 == 16 + 2568 * ((4099 + 63) // 64) == int(m.lib.mshgnn_metrics_com_segmented_scratch_bytes(4099))


@pytest.mark.parametrize("B,nb", [(4099, 4), (257, 2), (64, 1), (1, 1)])
def test_a_single_segment_is_the_whole_batch_call(B, nb):
    """One segment against mshgnn_metrics_com_step: the counts are equal, the sums agree within the bound of the module docstring -- both calls form a window's
    terms with the same operations and add them in different orders, each within that bound of the mirror."""
    y, yp, mean, std = _random_case(B, nb, 77 * B + nb)
    seg = np.zeros(B, dtype=np.int32)
    m = M.SegmentedComMetrics(1, nb, mean, std)
    m.update(y.cuda(), yp.cuda(), torch.from_numpy(seg).cuda())
    step = torch.zeros(8, dtype=torch.float64, device="cuda")
    scratch = torch.zeros(16384 // 8, dtype=torch.int64, device="cuda")
    yc, pc = y.cuda().contiguous(), yp.cuda().contiguous()
    rc = m.lib.mshgnn_metrics_com_step(pc.data_ptr(), yc.data_ptr(), B, nb, (C.c_double * 6)(*mean), (C.c_double * 6)(*std), step.data_ptr(), None,
                                       scratch.data_ptr(), None)
    assert rc == 0, m.lib.mshgnn_last_error()
    torch.cuda.synchronize()
    got, whole = m.state.cpu().numpy(), step.cpu().numpy()
    assert np.array_equal(got[0, [2, 3, 6, 7]], whole[[2, 3, 6, 7]]) and not got[1].any()
    bound = _bounds(y, yp, seg, 1, nb, mean, std)[0]
    err = np.abs(got[0] - whole)
    print(f"B {B} nb {nb}: |segmented - whole batch| / bound {np.max(err[[0, 1, 4, 5]] / bound[[0, 1, 4, 5]]):.3e}")
    assert (err <= bound).all(), (err, bound)


def test_bad_arguments_are_refused_before_any_launch():
    B, nb, n_seg = 65, 2, 3
    m = M.SegmentedComMetrics(n_seg, nb, MEAN, STD)
    lib = m.lib
    y, yp = [t.cuda() for t in _exact_pair(B, nb, 1)]
    seg = torch.zeros(B, dtype=torch.int32, device="cuda")
    state = torch.full((n_seg + 1, 8), 5.0, dtype=torch.float64, device="cuda")
    m.reserve(B)
    sc = m._scratch
    mean, std = (C.c_double * 6)(*MEAN), (C.c_double * 6)(*STD)
    p = lambda t: t.data_ptr()
    good = [p(yp), p(y), B, nb, mean, std, p(seg), n_seg, p(state), p(sc), None]
    for pos, bad in ((0, None), (1, None), (4, None), (5, None), (6, None), (8, None), (9, None), (2, 0), (2, -3), (3, 0), (3, -1), (7, 0), (7, -1),
                     (8, p(state) + 4), (9, p(sc) + 4)):
        args = list(good)
        args[pos] = bad
        assert lib.mshgnn_metrics_com_segmented(*args) == EINVAL, (pos, bad)
        assert b"mshgnn_metrics_com_segmented" in lib.mshgnn_last_error()
    torch.cuda.synchronize()
    assert bool((state == 5.0).all()) and not bool(sc.any())          # nothing was written: no launch
    assert int(lib.mshgnn_metrics_com_segmented_scratch_bytes(0)) == 0 and int(lib.mshgnn_metrics_com_segmented_scratch_bytes(64)) == 16 + 2568
    assert lib.mshgnn_metrics_com_segmented(*good) == 0          # (and the good arguments are good)
    torch.cuda.synchronize()
    assert float(state[0, 6]) == 5.0 + B
    with pytest.raises(ValueError):
        M.SegmentedComMetrics(0, nb, MEAN, STD)
    with pytest.raises(ValueError):
        M.SegmentedComMetrics(3, nb, MEAN[:5], STD)
    with pytest.raises(ValueError):
        m.update(y, yp[:-1], seg)
