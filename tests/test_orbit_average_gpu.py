"""mshgnn_orbit_average / _backward / _defect on the device, bit for bit against the numpy mirror (tests/orbit_reference.py, whose host test proves that this
case matrix tells every damaged variant from the mirror): 4 batch sizes x 5 orbit sizes x 6 output shapes on data with +-0, subnormals and mixed magnitudes,
the 16-byte and the element-wise path (odd rows, a pointer offset by one float), sentinels behind every output, the exact adjoint on integer data, the defect
state, the refusals (nothing launched) and a captured graph."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import orbit_reference as orb

pytestmark = pytest.mark.gpu
SENTINEL = 7.0
PAD = 64      # sentinel floats behind (and, for offset views, in front of) every output


def _action(perm, sign, width):
    from morphsym_hgnn_amd.symmetrise import OutputAction
    return OutputAction.from_tables(perm, sign, width)


def _dev(a, offset=0):
    """a float32 array on the device, at a 16-byte aligned address + `offset` floats"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    buf = torch.zeros(a.size + 8, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    v = buf[offset:offset + a.size].view(a.shape)
    v.copy_(torch.from_numpy(a))
    return v


def _out(rows, cols, offset=0, dtype=torch.float32, fill=SENTINEL):
    buf = torch.full((PAD + rows * cols + PAD,), fill, dtype=dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0 and PAD % 4 == 0
    return buf, buf[PAD + offset:PAD + offset + rows * cols].view(rows, cols)


def _untouched(buf, view, fill=SENTINEL):
    lo = (view.data_ptr() - buf.data_ptr()) // buf.element_size()
    return bool((buf[:lo] == fill).all()) and bool((buf[lo + view.numel():] == fill).all())


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


@pytest.mark.parametrize("U,w", orb.SHAPES)
@pytest.mark.parametrize("K", orb.ELEMENTS)
def test_average_and_backward_equal_the_mirror_bit_for_bit(K, U, w):
    from morphsym_hgnn_amd import symmetrise as sym
    for B in orb.WINDOWS:
        perm, sign, o, g = orb.case(B, K, U, w)
        act = _action(perm, sign, w)
        want, want_b = orb.average(o, perm, sign, w, B), orb.average_backward(g, perm, sign, w, B)
        for offset in (0, 1):      # 1: both pointers off the 16-byte grid -> the element-wise path, same bits
            buf, avg = _out(B, U * w, offset)
            sym._launch("mshgnn_orbit_average", act, _dev(o, offset), B, avg)
            buf_b, go = _out(K * B, U * w, offset)
            sym._launch("mshgnn_orbit_average_backward", act, _dev(g, offset), B, go)
            torch.cuda.synchronize()
            assert np.array_equal(_bits(avg), want.view(np.uint32)), (B, offset)
            assert np.array_equal(_bits(go), want_b.view(np.uint32)), (B, offset)
            assert _untouched(buf, avg) and _untouched(buf_b, go), (B, offset)
        if K == 1:
            assert np.array_equal(_bits(avg), o.view(np.uint32))      # one element: the output itself, -0 and subnormals included
    assert bool((o.view(np.uint32) == 0x80000000).any()) and bool(((np.abs(o) < 1e-38) & (o != 0)).any())


@pytest.mark.parametrize("K", [1, 2, 4, 8])
def test_the_backward_is_the_exact_adjoint_on_integer_data(K):
    from morphsym_hgnn_amd import symmetrise as sym
    rng = np.random.default_rng(K)
    for (U, w) in orb.SHAPES:
        B = 257
        perm, sign = orb.make_action(K, U)
        act = _action(perm, sign, w)
        o = rng.integers(-64, 65, (K * B, U * w)).astype(np.float32)
        v = rng.integers(-64, 65, (B, U * w)).astype(np.float32)
        od, vd = _dev(o), _dev(v)
        avg, go = torch.empty(B, U * w, device="cuda"), torch.empty(K * B, U * w, device="cuda")
        sym._launch("mshgnn_orbit_average", act, od, B, avg)
        sym._launch("mshgnn_orbit_average_backward", act, vd, B, go)
        lhs = float((avg.double() * vd.double()).sum())
        rhs = float((od.double() * go.double()).sum())
        assert lhs == rhs and lhs != 0.0, (U, w)


def test_orbit_average_is_an_autograd_function_on_any_layout():
    """no_grad, a non-contiguous input and an fp64 input: made contiguous fp32 as the engine's entry points do; the gradient comes back in the input's shape and dtype."""
    from morphsym_hgnn_amd import symmetrise as sym
    B, K, U, w = 17, 3, 6, 1
    perm, sign, o, g = orb.case(B, K, U, w)
    act = _action(perm, sign, w)
    want, want_b = orb.average(o, perm, sign, w, B), orb.average_backward(g, perm, sign, w, B)
    od = _dev(o)
    with torch.no_grad():
        assert np.array_equal(_bits(sym.orbit_average(od, act, B)), want.view(np.uint32))
    wide = torch.zeros(K * B, 2 * U * w, device="cuda")
    wide[:, ::2] = od
    for x in (od.clone().requires_grad_(), wide[:, ::2].requires_grad_(), od.double().requires_grad_()):
        avg = sym.orbit_average(x, act, B)
        assert avg.dtype == torch.float32 and avg.shape == (B, U * w) and np.array_equal(_bits(avg), want.view(np.uint32))
        (gx,) = torch.autograd.grad(avg, x, _dev(g))
        assert gx.shape == x.shape and gx.dtype == x.dtype and np.array_equal(_bits(gx.float()), want_b.view(np.uint32))
    with pytest.raises(ValueError, match="orbit-complete"):
        sym.orbit_average(od[:-1], act, B)


def _state(fill=0.0):
    return torch.full((8, 4), fill, dtype=torch.float64, device="cuda")


@pytest.mark.parametrize("U,w", [(6, 1), (12, 1), (4, 2), (5, 3)])
def test_the_defect_state(U, w):
    from morphsym_hgnn_amd import symmetrise as sym
    for K, B in ((3, 17), (4, 257), (2, 1), (8, 64)):
        if U == 6 and K != 3:
            continue
        if U != 6 and K == 3:
            continue
        perm, sign = orb.make_action(K, U)
        act = _action(perm, sign, w)
        # an equivariant output o_e = rho(g_e) o_0: exactly zero
        o0 = orb.make_data(B, U * w, 11 * K + U)
        o = np.concatenate([orb.apply_action(o0, perm, sign, w, e) for e in range(K)])
        st = _state()
        sym._launch("mshgnn_orbit_defect", act, _dev(o), B, st)
        got = st.cpu().numpy()
        assert np.array_equal(got[:K, 0], np.zeros(K)) and np.array_equal(got[:K, 2], np.zeros(K)) and np.array_equal(got[K:], np.zeros((8 - K, 4)))
        assert np.array_equal(got[:K], orb.defect(o, perm, sign, w, B))
        # random outputs: the mirror's state bit for bit, two calls accumulate, two runs give the same bits
        _, _, o, _ = orb.case(B, K, U, w)
        runs = []
        for _ in range(2):
            st = _state()
            sym._launch("mshgnn_orbit_defect", act, _dev(o), B, st)
            one = st.cpu().numpy().copy()
            sym._launch("mshgnn_orbit_defect", act, _dev(o, 1), B, st)
            runs.append((one, st.cpu().numpy().copy()))
        want1 = orb.defect(o, perm, sign, w, B)
        want2 = orb.defect(o, perm, sign, w, B, want1)
        assert np.array_equal(runs[0][0][:K].view(np.uint64), want1.view(np.uint64)) and np.array_equal(runs[0][1][:K].view(np.uint64), want2.view(np.uint64))
        assert np.array_equal(runs[0][0].view(np.uint64), runs[1][0].view(np.uint64)) and np.array_equal(runs[0][1].view(np.uint64), runs[1][1].view(np.uint64))
        if K > 1:
            assert want1[1, 0] > 0 and want1[1, 2] > 0 and want1[1, 3] == B * U * w


def test_a_planted_difference_gives_the_hand_computed_state_and_report():
    from morphsym_hgnn_amd import symmetrise as sym
    perm, sign = orb.three_cycle_action()
    act = sym.OutputAction.from_tables(perm, sign, 1, [None, "g", "gg"])
    B = 2
    o0 = np.arange(1, 13, dtype=np.float32).reshape(B, 6)
    o = np.concatenate([orb.apply_action(o0, perm, sign, 1, e) for e in range(3)])
    o[1 * B + 1, 2] += 0.5
    o[2 * B + 0, 4] -= 2.0
    s0 = float((o0.astype(np.float64) ** 2).sum())
    d = sym.EquivarianceDefect(act)
    assert d.operators == ["g", "gg"]
    d.update(_dev(o), B)
    assert d.state.cpu().tolist() == [[0.0, s0, 0.0, 12.0], [0.25, s0, 0.5, 12.0], [4.0, s0, 2.0, 12.0]]
    d.update(_dev(o).double(), B)      # (any dtype: made fp32)
    rep = d.report()
    assert rep["g"] == {"rms": math.sqrt(0.5 / 24), "max_abs": 0.5, "relative_rms": math.sqrt(0.5 / (2 * s0)), "n": 24}
    assert rep["gg"] == {"rms": math.sqrt(8.0 / 24), "max_abs": 2.0, "relative_rms": math.sqrt(8.0 / (2 * s0)), "n": 24}
    d.reset()
    assert not bool(d.state.any())


def test_bad_arguments_are_refused_before_anything_is_launched():
    from morphsym_hgnn_amd import engine as eng
    lib = eng.load_library()
    K, U, w, B = 3, 6, 1, 17
    perm, sign = orb.three_cycle_action()
    flat = lambda rows: (C.c_int32 * sum(len(r) for r in rows))(*[x for r in rows for x in r])
    src = torch.ones(K * B * U * w, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def damaged(what):
        p, s = [list(r) for r in perm], [list(r) for r in sign]
        if what == "not a permutation":
            p[2][3] = p[2][0]
        elif what == "out of range":
            p[1][5] = U
        elif what == "negative":
            p[1][0] = -1
        elif what == "zero sign":
            s[1][2] = 0
        elif what == "sign two":
            s[2][5] = 2
        elif what == "element 0 permuted":
            p[0][0], p[0][1] = 1, 0
        elif what == "element 0 signed":
            s[0][4] = -1
        return flat(p), flat(s)

    good = (flat(perm), flat(sign))
    cases = [("null perm", (None, good[1]), (K, U, w, B), True, True), ("null sign", (good[0], None), (K, U, w, B), True, True),
             ("null src", good, (K, U, w, B), False, True), ("null dst", good, (K, U, w, B), True, False),
             ("no element", good, (0, U, w, B), True, True), ("nine elements", good, (9, U, w, B), True, True),
             ("no unit", good, (K, 0, w, B), True, True), ("65 units", good, (K, 65, w, B), True, True),
             ("width 0", good, (K, U, 0, B), True, True), ("width 17", good, (K, U, 17, B), True, True),
             ("no window", good, (K, U, w, 0), True, True), ("negative windows", good, (K, U, w, -5), True, True),
             ("windows beyond the 64-bit element index", good, (K, U, w, 2 ** 62), True, True)]
    cases += [(what, damaged(what), (K, U, w, B), True, True) for what in ("not a permutation", "out of range", "negative", "zero sign", "sign two",
                                                                          "element 0 permuted", "element 0 signed")]
    for name in ("mshgnn_orbit_average", "mshgnn_orbit_average_backward", "mshgnn_orbit_defect"):
        is_defect = name.endswith("defect")
        for what, (p, s), (k, u, ww, b), has_src, has_dst in cases:
            if is_defect:
                dst = torch.full((8 * 4,), SENTINEL, dtype=torch.float64, device="cuda")
            else:
                dst = torch.full((K * B * U * w + PAD,), SENTINEL, device="cuda")
            torch.cuda.synchronize()
            rc = getattr(lib, name)(p, s, k, u, ww, src.data_ptr() if has_src else None, b, dst.data_ptr() if has_dst else None, stream)
            torch.cuda.synchronize()
            assert rc == -1, (name, what, rc)      # MSHGNN_EINVAL
            assert name in lib.mshgnn_last_error().decode(), (name, what)
            assert bool((dst == SENTINEL).all()), (name, what)
        if is_defect:      # a state off the 8-byte grid
            dst = torch.full((8 * 4 + 1,), SENTINEL, dtype=torch.float64, device="cuda")
            assert getattr(lib, name)(good[0], good[1], K, U, w, src.data_ptr(), B, dst.data_ptr() + 4, stream) == -1 and "8-byte aligned" in lib.mshgnn_last_error().decode()
            torch.cuda.synchronize()
            assert bool((dst == SENTINEL).all())
        # the good tables pass
        dst = torch.zeros(8 * 4, dtype=torch.float64, device="cuda") if is_defect else torch.empty(K * B * U * w, device="cuda")
        assert getattr(lib, name)(good[0], good[1], K, U, w, src.data_ptr(), B, dst.data_ptr(), stream) == 0
    torch.cuda.synchronize()


def test_forward_and_backward_captured_in_a_graph_replay_on_new_contents():
    """torch.cuda.graph on one stream: the tables travel in the kernel arguments, so the captured graph holds them; a replay on new contents equals eager."""
    from morphsym_hgnn_amd import symmetrise as sym
    B, K, U, w = 64, 4, 12, 1
    perm, sign, o, g = orb.case(B, K, U, w)
    act = _action(perm, sign, w)
    x = torch.zeros(K * B, U * w, device="cuda", requires_grad=True)
    gin = torch.zeros(B, U * w, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):      # warm-up outside the capture
            (gx,) = torch.autograd.grad(sym.orbit_average(x, act, B), x, gin)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            avg = sym.orbit_average(x, act, B)
            (gx,) = torch.autograd.grad(avg, x, gin)
    torch.cuda.current_stream().wait_stream(side)
    for seed in (1, 2):
        o2, g2 = orb.make_data(K * B, U * w, seed), orb.make_data(B, U * w, seed + 50)
        with torch.no_grad():
            x.copy_(torch.from_numpy(o2)); gin.copy_(torch.from_numpy(g2))
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_bits(avg), orb.average(o2, perm, sign, w, B).view(np.uint32)), seed
        assert np.array_equal(_bits(gx), orb.average_backward(g2, perm, sign, w, B).view(np.uint32)), seed
