"""A numpy float32 mirror of the three definitions of include/mshgnn.h's orbit entry points (mshgnn_orbit_average, mshgnn_orbit_average_backward,
mshgnn_orbit_defect), with the kernels' operation order -- the yardstick tests/test_orbit_average_gpu.py compares bit for bit against -- plus damaged variants
of it and the case matrix of that test, so that tests/test_orbit_reference.py can prove on the host that the GPU cases tell every damaged variant from the
mirror.

Layout: o float32 [K * B, U * width], element-major (row e * B + w = element e of base window w); perm / sign: [K][U] host tables, y_e[k] = sign[e][k] y[perm[e][k]].
Signs are applied as an XOR of the fp32 sign bit (exact, -0 included), never as a multiply."""
import numpy as np

THREADS = 1024      # the defect kernel's workgroup: thread t adds elements t, t + 1024, ... in that order, then a tree of strides 512 .. 1
VARIANTS = ("perm_for_pinv", "dropped_sign", "reverse_order", "scale_first")


def inverse(p):
    q = [0] * len(p)
    for k, x in enumerate(p):
        q[int(x)] = k
    return q


def _flip(x, neg):
    """x float32 [..., U, width], neg bool [U]: the sign bit of every unit with neg flipped"""
    bits = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) ^ (np.asarray(neg, dtype=np.uint32)[:, None] << np.uint32(31))
    return bits.view(np.float32)


def inv_k(K):
    return np.float32(1.0) / np.float32(K)


def mapped_back(o, perm, sign, width, B, e, variant=None):
    """t_e [B, U, width]: element e's block read through pinv_e, with the sign of the unit it came from"""
    U = len(perm[0])
    blk = np.asarray(o, dtype=np.float32).reshape(-1, U, width)[e * B:(e + 1) * B]
    idx = list(perm[e]) if variant == "perm_for_pinv" else inverse(perm[e])
    neg = [sign[e][idx[j]] < 0 and variant != "dropped_sign" for j in range(U)]
    return _flip(blk[:, idx, :], neg)


def average(o, perm, sign, width, B, variant=None):
    """avg float32 [B, U * width] = (t_0 + t_1 + ... + t_{K-1}) * fl32(1 / K): fp32 adds in element order starting from t_0, then the one multiply."""
    K, U = len(perm), len(perm[0])
    s = inv_k(K)
    order = list(range(K))
    if variant == "reverse_order":
        order.reverse()
    acc = None
    for e in order:
        t = mapped_back(o, perm, sign, width, B, e, variant)
        if variant == "scale_first":
            t = (t * s).astype(np.float32)
        acc = t.copy() if acc is None else (acc + t).astype(np.float32)
    if variant != "scale_first":
        acc = (acc * s).astype(np.float32)
    return acc.reshape(B, U * width)


def average_backward(g, perm, sign, width, B, variant=None):
    """g_o float32 [K * B, U * width]: g_o[e B + w][k width + s] = sign[e][k] (g[w][perm[e][k] width + s] * fl32(1 / K)) -- the exact transpose of `average`.
    Variants: perm_for_pinv (here: pinv where perm belongs), dropped_sign."""
    K, U = len(perm), len(perm[0])
    gs = (np.asarray(g, dtype=np.float32).reshape(B, U, width) * inv_k(K)).astype(np.float32)
    out = np.empty((K, B, U, width), dtype=np.float32)
    for e in range(K):
        idx = inverse(perm[e]) if variant == "perm_for_pinv" else list(perm[e])
        neg = [sign[e][k] < 0 and variant != "dropped_sign" for k in range(U)]
        out[e] = _flip(gs[:, idx, :], neg)
    return out.reshape(K * B, U * width)


def _thread_sums(v):
    """the kernel's reduction of a float64 vector: THREADS per-thread sums in index order, then the fixed tree"""
    n = v.shape[0]
    pad = np.zeros((n + THREADS - 1) // THREADS * THREADS, dtype=np.float64)
    pad[:n] = v
    part = np.zeros(THREADS, dtype=np.float64)
    for r in pad.reshape(-1, THREADS):
        part = part + r
    st = THREADS // 2
    while st > 0:
        part[:st] = part[:st] + part[st:2 * st]
        st //= 2
    return part[0]


def defect(o, perm, sign, width, B, state=None):
    """The state double [K][4] = {sum d^2, sum o_0^2, max |d|, count} after one call ADDED TO `state` (None: zeros): d = t_e - o_0 in fp32, the sums in fp64 in
    the kernel's order; row 0: zeros for sum d^2 and max |d|."""
    K, U = len(perm), len(perm[0])
    st = np.zeros((K, 4), dtype=np.float64) if state is None else np.array(state, dtype=np.float64).reshape(K, 4).copy()
    o0 = np.asarray(o, dtype=np.float32).reshape(-1, U, width)[:B]
    x0 = o0.reshape(-1).astype(np.float64)
    for e in range(K):
        d = (mapped_back(o, perm, sign, width, B, e) - o0).astype(np.float32).reshape(-1).astype(np.float64)
        if e == 0:
            st[e, 0], st[e, 2] = 0.0, 0.0
        else:
            st[e, 0] += _thread_sums(d * d)
            st[e, 2] = max(st[e, 2], float(np.abs(d).max()))
        st[e, 1] += _thread_sums(x0 * x0)
        st[e, 3] += float(x0.shape[0])
    return st


def apply_action(y, perm, sign, width, e):
    """rho(g_e) y for y float32 [B, U * width]: y_e[k] = sign[e][k] y[perm[e][k]]"""
    U = len(perm[0])
    return _flip(np.asarray(y, dtype=np.float32).reshape(-1, U, width)[:, list(perm[e]), :], [c < 0 for c in sign[e]]).reshape(-1, U * width)


# ---- actions and data of the GPU case matrix ---------------------------------------------------------------------------------------------------------------

def three_cycle_action():
    """K = 3 on 6 units with mixed signs: the identity, g (a 3-cycle on units 0 1 2 and one on 3 4 5) and g^2 = g . g -- NOT involutions, so perm and its
    inverse differ (the real groups' label permutations are all involutions and cannot tell them apart)."""
    p = [1, 2, 0, 4, 5, 3]
    s = [1, -1, 1, -1, -1, 1]
    p2 = [p[p[k]] for k in range(6)]                 # y_gg[k] = s[k] y_g[p[k]] = s[k] s[p[k]] y[p[p[k]]]
    s2 = [s[k] * s[p[k]] for k in range(6)]
    return [list(range(6)), p, p2], [[1] * 6, s, s2]


def make_action(K, U, seed=0):
    """element 0 the identity, the others random permutations with random signs (the 3-cycle action for K = 3, U = 6)"""
    if (K, U) == (3, 6):
        return three_cycle_action()
    rng = np.random.default_rng(1000 * K + 10 * U + seed)
    perm, sign = [list(range(U))], [[1] * U]
    for _ in range(1, K):
        perm.append([int(x) for x in rng.permutation(U)])
        sign.append([int(x) for x in rng.choice([-1, 1], U)])
    return perm, sign


def make_data(rows, cols, seed):
    """float32 [rows, cols] of mixed magnitude (exponents -30 .. 30) with +0, -0 and subnormals sprinkled in"""
    rng = np.random.default_rng(seed)
    x = (rng.uniform(1.0, 2.0, (rows, cols)) * np.exp2(rng.integers(-30, 31, (rows, cols))) * rng.choice([-1.0, 1.0], (rows, cols))).astype(np.float32)
    flat = x.reshape(-1)
    special = np.array([0.0, -0.0, 1e-40, -1e-40, 1.4e-45, -3e-39], dtype=np.float32)
    pos = rng.choice(flat.shape[0], max(1, flat.shape[0] // 5), replace=False)
    flat[pos] = special[rng.integers(0, len(special), pos.shape[0])]
    return x


WINDOWS = (1, 17, 64, 257)
ELEMENTS = (1, 2, 3, 4, 8)
SHAPES = ((4, 1), (12, 1), (6, 1), (4, 2), (5, 3), (3, 4))      # (n_units, width); (5, 3): 15 floats per row, the element-wise path; (3, 4): a unit is a whole quad, 16-byte loads of permuted units
CASES = [(B, K, U, w) for B in WINDOWS for K in ELEMENTS for (U, w) in SHAPES]


def case(B, K, U, width):
    """(perm, sign, o [K B, U width], g [B, U width]) of one case of the matrix"""
    perm, sign = make_action(K, U)
    seed = ((B * 16 + K) * 64 + U) * 16 + width
    return perm, sign, make_data(K * B, U * width, seed), make_data(B, U * width, seed + 7)
