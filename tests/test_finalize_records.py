"""Host plan (no GPU): the per-workgroup finalize records of the bf16 / split plans against the fin table they are derived from (csrc/mshgnn_plan.hpp).

The slab-free records of the weight-gradient launch (SIDE_INTS: decoder sums, zero fills of phase 0, zero fills of phase 1) and k_finalize's records (FSLAB_INTS) must
write exactly the elements the fin table's ops write -- every element of the flat gradient once, the same kind of op on it, in the same phase, from the same lanes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bench
from morphsym_hgnn_amd import engine as eng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "morphsym_hgnn_amd", "csrc")
H = 128
FIN_INTS, SIDE_INTS, FSLAB_INTS, TGT_INTS = 8, 8, 10, 8
FIN_MATRIX, FIN_BIAS, FIN_ZERO, FIN_DEC_W, FIN_DEC_B = range(5)
M = dict(NFIN=15, FIN_OFF=146, NFIN_PH0=147, SIDE_OFF=148, NSIDE_DEC=149, NSIDE_Z0=150, NSIDE_Z1=151, FSLAB_OFF=152, NFSLAB=153, NFSLAB_PH0=154, TGT_OFF=155, SPLIT_LO=156, SPLIT_HI=157)


def _plan(cfg, layers, dtype):
    subprocess.run(["make", "-C", CSRC, "../libmshgnn_hostplan.so"], check=True, capture_output=True)
    lib = C.CDLL(os.path.join(ROOT, "morphsym_hgnn_amd", "libmshgnn_hostplan.so"))
    lib.mshgnn_hostplan_compile.argtypes = [C.POINTER(eng.MshgnnDesc), C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int32), C.c_int]
    lib.mshgnn_hostplan_last_error.restype = C.c_char_p
    spec = bench.build_spec(layers, cfg)
    holder = eng._DescHolder(spec, eng.DTYPE_CODES[dtype])
    meta = (C.c_int32 * 160)()
    n = lib.mshgnn_hostplan_compile(C.byref(holder.desc), None, 0, meta, 1)
    assert n > 0, lib.mshgnn_hostplan_last_error()
    tables = (C.c_int32 * n)()
    lib.mshgnn_hostplan_compile(C.byref(holder.desc), tables, n, meta, 0)
    return spec, np.frombuffer(tables, dtype=np.int32).copy(), list(meta)


def _dst(lo, hi):
    return (int(lo) & 0xFFFFFFFF) | (int(hi) << 32)


@pytest.mark.parametrize("cfg,layers,dtype", [("a1c2", 3, "bf16"), ("a1c2", 3, "x3"), ("a1c2", 8, "bf16"), ("mck4", 8, "bf16")])
def test_records_write_what_the_fin_table_writes(cfg, layers, dtype):
    spec, T, meta = _plan(cfg, layers, dtype)
    m = {k: meta[v] for k, v in M.items()}
    n_flat = spec.flat_size()
    split = _dst(m["SPLIT_LO"], m["SPLIT_HI"])
    if split >= 1 << 63:
        split -= 1 << 64
    # what the fin table says about every element: (kind, phase, lane range of its slab sum, source element of the slab)
    kind = np.full(n_flat, -1); phase = np.full(n_flat, -1); lanes = np.full((n_flat, 2), -1); src = np.full(n_flat, -1)
    fin0 = m["FIN_OFF"]
    for i in range(m["NFIN"]):
        f = T[fin0 + i * FIN_INTS: fin0 + (i + 1) * FIN_INTS]
        rows, cols, ld, tg, k, extra = (int(v) for v in f[2:8])
        dsts = [_dst(f[0], f[1])]
        if extra:
            nm = int(T[fin0 + extra])
            dsts += [_dst(T[fin0 + extra + 1 + 2 * j], T[fin0 + extra + 2 + 2 * j]) for j in range(nm)]
        for d in dsts:
            for r in range(rows):
                at = slice(d + r * ld, d + r * ld + cols)
                assert (kind[at] == -1).all(), "the fin table writes an element twice"
                kind[at] = k; phase[at] = 0 if i < m["NFIN_PH0"] else 1
                if k in (FIN_MATRIX, FIN_BIAS):
                    t = T[m["TGT_OFF"] + tg * TGT_INTS: m["TGT_OFF"] + tg * TGT_INTS + 2]
                    lanes[at] = (int(t[0]), int(t[1]) - int(t[0]))
                    src[at] = (r * H if k == FIN_MATRIX else H * H) + np.arange(cols)
                elif k in (FIN_DEC_W, FIN_DEC_B):
                    src[at] = (r * H if k == FIN_DEC_W else 8 * H) + np.arange(cols)
    assert (kind >= 0).all()
    # the records
    kind2 = np.full(n_flat, -1); phase2 = np.full(n_flat, -1); lanes2 = np.full((n_flat, 2), -1); src2 = np.full(n_flat, -1)

    def put(at, k, ph):
        assert at.start >= 0 and at.stop <= n_flat and (kind2[at] == -1).all(), "a record writes outside the buffer or an element twice"
        kind2[at] = k; phase2[at] = ph

    n_dec, n_z0, n_z1 = m["NSIDE_DEC"], m["NSIDE_Z0"], m["NSIDE_Z1"]
    assert n_dec > 0
    for i in range(n_dec + n_z0 + n_z1):
        f = [int(v) for v in T[m["SIDE_OFF"] + i * SIDE_INTS: m["SIDE_OFF"] + (i + 1) * SIDE_INTS]]
        d, a, cols, ld, k, last = _dst(f[0], f[1]), f[2], f[3], f[4], f[5], f[6]
        if i < n_dec:
            assert k in (FIN_DEC_W, FIN_DEC_B) and 0 <= a < last <= a + 16
            for e in range(a, last):
                at = slice(d + (e // cols) * ld + e % cols, d + (e // cols) * ld + e % cols + 1)
                put(at, k, 0)
                src2[at] = ((e // cols) * H if k == FIN_DEC_W else 8 * H) + e % cols
        else:
            assert k == FIN_ZERO and a >= 1 and a * cols <= 8192
            for r in range(a):
                put(slice(d + r * ld, d + r * ld + cols), k, 0 if i < n_dec + n_z0 else 1)
    for i in range(m["NFSLAB"]):
        f = [int(v) for v in T[m["FSLAB_OFF"] + i * FSLAB_INTS: m["FSLAB_OFF"] + (i + 1) * FSLAB_INTS]]
        d, row0, rows, cols, ld, l0, nl, extra, k = _dst(f[0], f[1]), *f[2:10]
        assert k in (FIN_MATRIX, FIN_BIAS) and 1 <= rows <= 8 and 1 <= cols <= H and nl >= 1
        dsts = [d]
        if extra:
            nm = int(T[fin0 + extra])
            dsts += [_dst(T[fin0 + extra + 1 + 2 * j], T[fin0 + extra + 2 + 2 * j]) for j in range(nm)]
        for dd in dsts:
            for r in range(row0, row0 + rows):
                at = slice(dd + r * ld, dd + r * ld + cols)
                put(at, k, 0 if i < m["NFSLAB_PH0"] else 1)
                lanes2[at] = (l0, nl)
                src2[at] = (r * H if k == FIN_MATRIX else H * H) + np.arange(cols)
    assert (kind2 == kind).all() and (phase2 == phase).all() and (lanes2 == lanes).all() and (src2 == src).all()
    # the phases split the buffer at grad_split (the encoder's parameters are phase 1), or there is one phase
    if split >= 0:
        assert (phase[:split] == 1).all() and (phase[split:] == 0).all()
    else:
        assert (phase == 0).all() and n_z1 == 0 and m["NFSLAB_PH0"] == m["NFSLAB"]
