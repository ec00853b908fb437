"""`mshgnn_assemble_windows` (csrc/mshgnn_windows.hip: k_assemble_windows, k_assemble_windows_fast, k_window_labels[_orbit]; run_stats / standardise_one /
window_labels_one of mshgnn_device.hpp) ELEMENT BY ELEMENT through the C ABI, on HAND-BUILT device tables, against tests/window_reference.py.  The gather is
the root of the suite's bit-identity chain -- the fused series steps, mshgnn_forward_series, the transformed siblings, the orbit batches, ResidentDataset, the
wrappers' WindowBatch route and the MLP series step are all held to "assemble, then the dense entry point" with torch.equal -- so whatever it got wrong was
wrong on both sides of those comparisons.  Unstandardised data must be a BIT-EXACT copy (the expected bits are torch's own fp32 -> bf16 cast; any NaN matches
any NaN, the sign of a zero counts), standardised values and rotated labels must lie, per element, inside the interval DERIVED in window_reference (no
tolerance here is a measured number).  Every output buffer is larger than the result and filled with a NaN of a payload no kernel produces: rows behind the
batch, features no run covers and pad columns outside what the chunk kernel documents (zeros up to the end of a row's last 16-byte chunk) must still hold
it; y and quat have 64 such elements behind them.  tests/test_window_reference.py shows on the host that the checker accepts an fp64 emulation of the kernels
and rejects eighteen mutations, on the descriptors used here.  A failure prints the first (window, type, node, feature, got, want), the run and the position.

What tests/test_windows.py, test_window_symmetry_gpu.py and test_window_orbit_gpu.py left unreached, and what reaches it now:
  * only robot recipes: every run `history` long at a multiple of `history`, 1 / 2 / 3 / 6 (18) runs per row.  Any first feature, lengths 1 .. 256, rows
    that mix lengths, uncovered features, 1 .. 17 runs per row (the WIN_ROW_RUNS = 8 batches), 1 .. 128 runs (NSET), 1 .. 65 rows, 12 sources, column 255,
    four types, pitch > width, the run-by-run kernel on descriptors that do not promise the fast layout
                                                      -> test_run_lengths_*, test_rows_of_runs_*, test_run_and_row_counts, test_129_runs_*
  * K = 2 / K = 8 element blocks that differ in columns and signs, element indices K and 255 in a device start -> test_orbit_blocks_*
  * chunks that straddle two runs at every position, opposite signs in both orders, the 256-task stride, WIN_MAX_ROWS and the fall-back past it, zeroed
    pad columns, the alignment test of the fast path -> test_chunk_kernel_*, test_chunk_counts_*, test_chunk_kernel_64_rows_*
  * standardised windows were held to 2e-7 max |ref| (2^-7 on bf16) over a whole tensor of smooth data: a biased variance, an fp32-formed mean, a sign
    after the statistics, a wrong small element were invisible -> test_standardised_*
  * body-frame labels to 1e-6 max |y| on 12 labels and unit quaternions: the LMAX = 24 chunks, the normalisation, the sign after the rotation
                                                      -> test_labels_*
  * the error returns of the entry point              -> test_error_returns_launch_nothing (sign / orbit tables: test_window_symmetry_gpu.py::
    test_bad_sign_tables_are_refused_before_anything_is_written, test_window_orbit_gpu.py::test_bad_orbit_tables_are_refused_before_anything_is_written)
  * split point n0 = 7 of splice8f / standardise_oct / sign_mask8_* (and 1 .. 6 under alternating signs) on the fused routes -> test_fused_routes_at_every_split_point

Matrix.  Run-by-run kernel (fast_layout = 0, and every normalize = 1 case), fp32 and bf16 outputs, MSHGNN_BF16X3 once: lengths {1, 2, 3, 63, 64, 65, 127,
128, 129, 130, 255, 256} x first feature even / odd; runs per row {1, 7, 8, 9, 16, 17}; (n_runs, n_rows) in {(1, 1), (63, 3), (64, 4), (65, 5), (128, 64),
(128, 65)}, 129 runs refused; B in {1, 2, 5, 257}; src_cstride = rows + {0, 8, 13}; starts 0, the last valid row, repeats; odd pitches and an output base
that is only element-aligned (the packed stores, see "Found").  Special values in every unstandardised series: +-0, fp32 subnormals, the largest finite
fp32 (infinity on bf16), the largest finite bf16, +-inf, NaN.  Chunk kernel (fast_layout = 1, first feature 0): history {1, 2, 3, 4, 5, 7, 8, 9, 150, 256}
x rows of {9, 1, 8, 3} runs + width-1 constant rows, signs + + - -; 255 / 256 / 257 / > 512 chunks per window; 64 rows, 65 rows (fall-back); every such
descriptor again with an odd pitch and an element-aligned base (same values through the run-by-run kernel, no pad zeros); K = 2.  Standardisation:
lengths {2, 3, 64, 129, 256} x {random, constant, negated constant, offset 1e6 under noise of a few fp32 spacings, two-valued, 1e30, 1e-30, NaN inside,
negated beside plain, constant 1}.  Labels: n_label {1, 4, 12, 23, 24, 25, 48, 49} unrotated, {3, 12, 24, 27, 48, 51} rotated with quaternions {unit,
norm 0.5, norm 3, negative w, near identity, near a half turn} by row, signed, K = 2 label blocks, column 255, B {1, 255, 256, 257}, quat_out copied /
NULL / requested with n_label == 0.

Not covered, and why:
  * infinities in a STANDARDISED series: the reference's nan_to_num turns them into the largest finite value and oracle/window_oracle.py leaves that
    open; window_reference refuses such a run.
  * a zero quaternion: NaN in the reference too.
  * starts past the series' end, node / feature / column indices outside their tensors: device-given and unchecked by contract (include/mshgnn.h); this
    file validates every descriptor on the host before it launches.
  * fast_layout = 1 on rows whose first feature is not 0: the header now says feature 0 (it said "the row's first run's feature", which the 16-byte stores
    of the chunk kernel never supported); the host cannot read the device tables to check.

Found and fixed with these tests: k_assemble_windows chose its packed two-element store from the parity of the offset INSIDE the window's block, which
assumed 16-byte aligned node rows; the entry point only asks for pitch >= width and a non-null pointer, so an odd pitch with an odd batch index * nodes, or
an element-aligned x_out, put a 4- / 8-byte store on an address that is no multiple of its size.  It now decides from the destination's own element
address (uniform per run).  test_run_lengths_* and test_rows_of_runs_* run odd pitches and an element-aligned base.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from morphsym_hgnn_amd import engine as eng
from tests import window_reference as wr

pytestmark = pytest.mark.gpu
DEV = "cuda"
EINVAL, EUNSUPPORTED = -1, -2
DTYPE_CODE = {"f32": 0, "bf16": 1, "x3": 2}
EPC = {"f32": 4, "bf16": 8, "x3": 4}


def _require_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (there is no CPU fallback to fall through to)")


def _validate(tab, series, starts):
    """Everything the kernels trust: the test's own bug must not become an out-of-bounds access on the device."""
    n_rows = min(s.shape[0] for s in series)
    signed = bool(tab.sign_flags & 1) or tab.K > 1
    assert 1 <= len(tab.type_nodes) <= 4 and len(tab.pitch) == len(tab.type_nodes) and 1 <= len(series) <= 12
    assert 1 <= tab.n_runs <= 128 and len(tab.runs) == tab.K and all(len(blk) == tab.n_runs for blk in tab.runs)
    for blk in tab.runs:
        for t, node, f0, word, ln in blk:
            assert 0 <= t < len(tab.type_nodes) and 0 <= node < tab.type_nodes[t] and 0 <= f0 and 1 <= ln <= 256 and f0 + ln <= tab.pitch[t]
            s, c, _ = wr.decode(word, signed)
            assert s is None or (0 <= s < len(series) and 0 <= c < series[s].shape[1])
    assert all(0 <= a < b <= tab.n_runs for a, b in tab.rows)
    need = max(tab.history, max(r[4] for r in tab.runs[0]))
    for sw in starts:
        _, row = wr.split_start(sw, tab.K)
        assert 0 <= row and row + need <= n_rows
    if tab.n_label:
        assert len(tab.label_cols) == tab.K
        assert all(0 <= (c & ~wr.SIGN_FLAG) < series[tab.label_src].shape[1] for blk in tab.label_cols for c in blk)
    assert tab.quat_src < 0 or series[tab.quat_src].shape[1] >= 4


class Harness:
    """Device tables, series and sentinel-filled outputs of one descriptor; `call` runs mshgnn_assemble_windows with optional overrides."""

    def __init__(self, tab, series, starts, dtype, fast_layout=0, base_offset=0, rows_behind=2, want_y=True, want_quat=True):
        _require_gpu()
        _validate(tab, series, starts)
        self.tab, self.starts, self.dtype = tab, list(starts), dtype
        self.lib = eng.load_library()
        self.B = B = len(starts)
        self.out_dtype = "bf16" if dtype == "bf16" else "f32"
        self.series = []
        cs, rows = [], []
        for i, a in enumerate(series):      # column-major, NaN between a column's last row and the next column
            n, ncol = a.shape
            stride = n + wr.CSTRIDE_EXTRA[i % 3]
            buf = torch.full((ncol, stride), float("nan"), dtype=torch.float32)
            buf[:, :n] = torch.from_numpy(np.ascontiguousarray(a.T))
            self.series.append(buf.to(DEV))
            cs.append(stride); rows.append(n)
        self.src = (C.c_void_p * len(series))(*[s.data_ptr() for s in self.series])
        self.cstride = (C.c_int64 * len(series))(*cs)
        self.src_rows = (C.c_int64 * len(series))(*rows)
        self.runs = torch.tensor([r for blk in tab.runs for r in blk], dtype=torch.int32, device=DEV)
        self.rows = torch.tensor(tab.rows, dtype=torch.int32, device=DEV)
        self.label_cols = torch.tensor([c for blk in tab.label_cols for c in blk] or [0], dtype=torch.int32, device=DEV)
        self.starts_dev = torch.tensor(self.starts, dtype=torch.int64, device=DEV)
        d = eng.MshgnnWindowDesc()
        d.n_types = len(tab.type_nodes); d.dtype = DTYPE_CODE[dtype]; d.history = tab.history; d.normalize = tab.normalize
        for t, (n, w) in enumerate(zip(tab.type_nodes, tab.type_width)):
            d.type_nodes[t] = n; d.type_width[t] = w
        d.n_src = len(series); d.n_runs = tab.n_runs; d.n_rows = len(tab.rows); d.fast_layout = fast_layout
        d.runs = self.runs.data_ptr(); d.rows = self.rows.data_ptr()
        d.n_label = tab.n_label; d.label_src = tab.label_src; d.label_rotate = tab.label_rotate; d.quat_src = tab.quat_src
        d.label_cols = self.label_cols.data_ptr(); d.sign_flags = tab.sign_flags
        self.desc = d
        esize = 2 if self.out_dtype == "bf16" else 4
        self.flat, self.xs = [], []
        for n, p in zip(tab.type_nodes, tab.pitch):
            flat = wr.sentinel_tensor((base_offset + (B + rows_behind) * n * p + 8,), self.out_dtype, DEV)
            self.flat.append(flat)
            self.xs.append(flat[base_offset:base_offset + (B + rows_behind) * n * p].view(B + rows_behind, n, p))
        self.x_ptr = (C.c_void_p * len(self.xs))(*[f.data_ptr() + base_offset * esize for f in self.flat])
        self.pitch = (C.c_int64 * len(self.xs))(*tab.pitch)
        self.y = wr.sentinel_tensor((B * tab.n_label + 64,), "f32", DEV) if want_y else None
        self.quat = wr.sentinel_tensor((B * 4 + 64,), "f32", DEV) if want_quat else None

    def call(self, **over):
        a = dict(desc=C.byref(self.desc), src=self.src, cstride=self.cstride, rows=self.src_rows, starts=self.starts_dev.data_ptr(), batch=self.B, x=self.x_ptr,
                 pitch=self.pitch, y=self.y.data_ptr() if self.y is not None else None, quat=self.quat.data_ptr() if self.quat is not None else None)
        a.update(over)
        rc = self.lib.mshgnn_assemble_windows(a["desc"], a["src"], a["cstride"], a["rows"], a["starts"], a["batch"], a["x"], a["pitch"], a["y"], a["quat"],
                                              C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        return rc

    def untouched(self):
        """True when every output buffer still holds nothing but the sentinel."""
        bufs = self.flat + [b for b in (self.y, self.quat) if b is not None]
        return all(wr._sentinel_broken(b.cpu(), np.ones(tuple(b.shape), dtype=bool)) is None for b in bufs)

    def verdict(self, exp):
        for t, (f, x) in enumerate(zip(self.flat, self.xs)):      # the elements in front of an offset base and behind the tensor
            lo, hi = x.storage_offset(), x.storage_offset() + x.numel()
            edge = torch.cat([f[:lo], f[hi:]]).cpu()
            if wr._sentinel_broken(edge, np.ones(edge.numel(), dtype=bool)) is not None:
                return f"type {t}: wrote in front of or behind its output tensor"
        return wr.check(self.tab, exp, [x.cpu() for x in self.xs], self.y, self.quat, self.starts)


def _run(tab, series, starts, dtype, fast_layout=0, chunk=0, base_offset=0, exp=None, **kw):
    h = Harness(tab, series, starts, dtype, fast_layout, base_offset, **kw)
    rc = h.call()
    assert rc == 0, (rc, h.lib.mshgnn_last_error())
    exp = exp if exp is not None else wr.reference(tab, series, starts, chunk)
    v = h.verdict(exp)
    assert v is None, f"[{dtype}, fast_layout {fast_layout}, base offset {base_offset}] {v}"
    return exp


# ---- the run-by-run kernel -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_run_lengths_and_first_feature_parities_are_exact_copies(dtype):
    """Every length of the matrix at an even and an odd first feature, odd pitch 261, signed runs, special values; then the same with an output base that is
    only element-aligned (the packed stores must give way to scalar ones)."""
    tab, series = wr.lengths_case(signed=True)
    starts = wr.starts_for(tab, series, 5)
    exp = _run(tab, series, starts, dtype)
    _run(tab, series, starts, dtype, base_offset=1, exp=exp)
    _run(tab, series, starts, dtype, fast_layout=1, exp=exp)      # (a promise the aligned-rows test of the fast path turns down: pitch 261)


@pytest.mark.parametrize("dtype", ["f32", "bf16", "x3"])
def test_rows_of_runs_are_exact_copies(dtype):
    """Rows of 1, 7, 8, 9, 16, 17 runs of mixed lengths with gaps in front, between and behind, constant-1 runs between sourced ones, four types with
    different node counts and pitches (two of them odd), 12 sources, column 255, signs + + - -."""
    tab, series = wr.general_case([1, 7, 8, 9, 16, 17], 3, signed=True)
    assert len(series) == 12 and any(p % 2 for p in tab.pitch) and any((r[3] & 0xff) == 255 and r[3] >> 8 & 0xf == 0 for r in tab.runs[0] if r[3] != -1)
    for B in (1, 2, 5):
        starts = wr.starts_for(tab, series, B)
        exp = _run(tab, series, starts, dtype)
        if B == 5 and dtype != "x3":
            _run(tab, series, starts, dtype, base_offset=1, exp=exp)


@pytest.mark.parametrize("n_runs,n_rows,B", [(1, 1, 257), (63, 3, 5), (64, 4, 5), (65, 5, 257), (128, 64, 2), (128, 65, 5)])
def test_run_and_row_counts(n_runs, n_rows, B):
    """The NSET switch (64 / 65 runs), the four waves' round-robin over the rows, 128 runs, more than one block of windows."""
    counts = [1] * (n_rows - 1) + [n_runs - (n_rows - 1)]
    tab, series = wr.general_case(counts, 100 + n_runs + n_rows, signed=n_runs % 2 == 1)
    assert tab.n_runs == n_runs and len(tab.rows) == n_rows
    starts = wr.starts_for(tab, series, B)
    for dtype in ("f32", "bf16"):
        _run(tab, series, starts, dtype)


def test_129_runs_are_unsupported_and_nothing_is_written():
    tab, series = wr.general_case([1, 128], 7)
    assert tab.n_runs == 129
    starts = wr.starts_for(tab, series, 2)
    tab128 = wr.WindowTables([tab.runs[0][:128]], [[0, 1], [1, 128]], tab.type_nodes, tab.pitch, tab.history)
    h = Harness(tab128, series, starts, "f32")      # (validated tables; the 129th run only exists in n_runs)
    h.desc.n_runs = 129
    assert h.call() == EUNSUPPORTED and b"128 feature runs" in h.lib.mshgnn_last_error() and h.untouched()


@pytest.mark.parametrize("K", [2, 8])
@pytest.mark.parametrize("normalize", [0, 1])
def test_orbit_blocks_pick_their_own_columns_and_signs(K, normalize):
    """K element blocks that differ in columns and signs, an element per window, element indices K and 255 in a device start (clamped to K - 1)."""
    tab, series = wr.general_case([1, 7, 8, 9], 5, signed=True, K=K, normalize=normalize)
    assert any(a[3] != b[3] for a, b in zip(tab.runs[0], tab.runs[K - 1]))
    starts = wr.starts_for(tab, series, 12, elements=list(range(K)) + [K, 255, K - 1, 0])
    for dtype in ("f32", "bf16"):
        _run(tab, series, starts, dtype)


# ---- the chunk kernel ----------------------------------------------------------------------------------------------------------------------------------
def _chunk_and_fallback(tab_of, starts_n, dtype, **kw):
    """A fast-layout descriptor through the chunk kernel, then with an odd pitch and with an element-aligned base through the other kernel: same values."""
    chunk = EPC[dtype]
    tab, series = tab_of(chunk)
    starts = wr.starts_for(tab, series, starts_n, **kw)
    _run(tab, series, starts, dtype, fast_layout=1, chunk=chunk)
    plain = wr.reference(tab, series, starts, 0)
    _run(tab, series, starts, dtype, fast_layout=1, base_offset=1, exp=plain)
    tab.pitch = [p + 1 for p in tab.pitch]      # (not a whole number of chunks any more)
    _run(tab, series, starts, dtype, fast_layout=1)
    return tab


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("history", [1, 2, 3, 4, 5, 7, 8, 9, 150, 256])
def test_chunk_kernel_at_every_history(history, dtype):
    """Rows of 9, 1, 8 and 3 runs (a chunk splits between two runs at every position 1 .. EPC - 1 for history 7 and 9) with signs + + - -, widths that are no
    whole chunks (zeros inside the last chunk, the sentinel beyond it), two width-1 constant rows."""
    tab = _chunk_and_fallback(lambda c: wr.general_case([9, 1, 8, 3], 6, n_types=3, signed=True, fast_layout=True, history=history, chunk=c, const_rows=2), 5, dtype)
    if history in (7, 9):
        splits = {(k * history) % EPC[dtype] for k in range(1, 9)}
        assert splits >= set(range(1, EPC[dtype]))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("extra", [3, 4, 5])
def test_chunk_counts_around_the_256_task_stride(extra, dtype):
    """255, 256 and 257 chunks per window: one row of 63 runs of four chunks each, one of `extra` runs of one chunk."""
    c = EPC[dtype]
    tab = _chunk_and_fallback(lambda c: wr.general_case([63, extra], 8, signed=True, fast_layout=True, row_lengths=[4 * c, c], chunk=c), 2, dtype)
    assert sum((b - a) * tab.runs[0][a][4] for a, b in tab.rows) == (252 + extra) * c


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_chunk_counts_beyond_512(dtype):
    tab = _chunk_and_fallback(lambda c: wr.general_case([17, 2], 9, signed=True, fast_layout=True, history=256, chunk=c, const_rows=1), 2, dtype)
    assert 17 * 256 // EPC[dtype] > 512


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("n_rows", [64, 65])
def test_chunk_kernel_64_rows_and_the_fall_back_past_them(n_rows, dtype):
    """WIN_MAX_ROWS = 64 node rows go through the chunk kernel (pad zeros), 65 fall back to the run-by-run kernel (none)."""
    c = EPC[dtype]
    tab, series = wr.general_case([1 + i % 2 for i in range(n_rows)], 10, signed=True, fast_layout=True, history=5, chunk=c)
    starts = wr.starts_for(tab, series, 5)
    _run(tab, series, starts, dtype, fast_layout=1, chunk=c if n_rows <= 64 else 0)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_chunk_kernel_orbit_blocks(dtype):
    _chunk_and_fallback(lambda c: wr.general_case([9, 1, 8, 3], 11, n_types=3, signed=True, K=2, fast_layout=True, history=7, chunk=c, const_rows=1), 8, dtype,
                        elements=[0, 1, 2, 255])


# ---- standardisation ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16", "x3"])
def test_standardised_runs_lie_inside_the_derived_bound(dtype):
    """Lengths 2, 3, 64, 129, 256 x random / constant / negated constant / offset 1e6 / two-valued / 1e30 / 1e-30 / NaN inside / negated beside plain / the
    constant 1: every element inside its interval, the exact ones (constant and NaN runs: +0.0, the constant 1) bit for bit."""
    tab, series = wr.standardise_case()
    starts = wr.starts_for(tab, series, 5)
    exp = _run(tab, series, starts, dtype)
    assert sum(int(((b == 0) & c).sum()) for b, c in zip(exp.bound, exp.covered)) > 100 and max(float(b.max()) for b in exp.bound) < 2.0 ** -23
    _run(tab, series, starts, dtype, fast_layout=1, base_offset=0, exp=exp)      # (normalize always takes the run-by-run kernel)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_standardised_rows_of_mixed_runs(dtype):
    """The run-by-run matrix under normalize: mixed lengths (1 included: 0 / 0 -> 0), gaps, constant-1 runs between sourced ones, signs, an element-aligned base."""
    tab, series = wr.general_case([1, 7, 8, 9, 16, 17], 13, signed=True, normalize=1)
    starts = wr.starts_for(tab, series, 5)
    exp = _run(tab, series, starts, dtype)
    _run(tab, series, starts, dtype, base_offset=1, exp=exp)
    tab, series = wr.lengths_case(normalize=1, signed=True)
    _run(tab, series, wr.starts_for(tab, series, 2), dtype)


# ---- labels and quaternions ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_label", [1, 4, 12, 23, 24, 25, 48, 49])
def test_labels_unrotated_are_exact_copies(n_label):
    for signed in (False, True):
        tab, series = wr.label_case(n_label, False, signed=signed)
        _run(tab, series, wr.starts_for(tab, series, 7), "f32")


@pytest.mark.parametrize("n_label", [3, 12, 24, 27, 48, 51])
def test_labels_rotated_lie_inside_the_derived_bound(n_label):
    """Quaternions by row: unit, norm 0.5, norm 3, negative w, near identity, near a half turn; signed labels are negated after the rotation."""
    for signed in (False, True):
        tab, series = wr.label_case(n_label, True, signed=signed)
        starts = wr.starts_for(tab, series, 24)
        assert {(wr.split_start(s, 1)[1] + tab.history - 1) % wr.QUAT_KINDS for s in starts} == set(range(wr.QUAT_KINDS))
        exp = _run(tab, series, starts, "f32")
        assert float(exp.y_bound.max()) < 2.0 ** -40 * float(np.abs(exp.y).max())


@pytest.mark.parametrize("B", [1, 255, 256, 257])
def test_labels_one_thread_per_window(B):
    tab, series = wr.label_case(12, True, signed=True, seed=B)
    _run(tab, series, wr.starts_for(tab, series, B, seed=B), "bf16")


def test_labels_orbit_blocks_and_quaternion_options():
    tab, series = wr.label_case(27, True, K=2)
    starts = wr.starts_for(tab, series, 12, elements=[0, 1, 2, 255])
    _run(tab, series, starts, "f32")
    _run(tab, series, starts, "f32", want_quat=False)                     # quat_out == NULL: the labels all the same
    tab, series = wr.label_case(25, False, K=8)
    _run(tab, series, wr.starts_for(tab, series, 12, elements=list(range(8)) + [8, 255]), "f32")
    tab, series = wr.label_case(0, False)                                # quat_out requested with n_label == 0: an exact copy, y untouched
    _run(tab, series, wr.starts_for(tab, series, 7), "f32")
    tab, series = wr.label_case(5, False, quat=False)                    # no quaternion source: quat_out untouched
    _run(tab, series, wr.starts_for(tab, series, 7), "f32")


# ---- error returns ----------------------------------------------------------------------------------------------------------------------------------------
def test_error_returns_launch_nothing():
    """Every `return set_err` of mshgnn_assemble_windows: its code, a message, and every output buffer still the sentinel.  (The refusals of the sign / orbit
    table check: test_window_symmetry_gpu.py, test_window_orbit_gpu.py; K > 8 and K > 1 without bit 0 are repeated here because they need no tables.)"""
    tab, series = wr.label_case(12, True)
    starts = wr.starts_for(tab, series, 3)
    h = Harness(tab, series, starts, "f32")
    fields = [f[0] for f in eng.MshgnnWindowDesc._fields_]

    def with_desc(**kw):
        d = eng.MshgnnWindowDesc()
        for f in fields:
            setattr(d, f, getattr(h.desc, f))
        for k, v in kw.items():
            if k in ("type_nodes", "type_width"):
                getattr(d, k)[0] = v
            else:
                setattr(d, k, v)
        return dict(desc=C.byref(d), _keep=d)

    def arr(ctype, values):
        return (ctype * len(values))(*values)
    n = len(series)
    cases = [(dict(desc=None), EINVAL), (dict(src=None), EINVAL), (dict(cstride=None), EINVAL), (dict(rows=None), EINVAL), (dict(starts=None), EINVAL),
             (dict(x=None), EINVAL), (dict(pitch=None), EINVAL), (dict(batch=0), EINVAL), (dict(batch=-3), EINVAL)]
    cases += [(with_desc(**kw), EINVAL) for kw in (dict(n_types=0), dict(n_types=5), dict(n_src=0), dict(n_src=13), dict(n_runs=0), dict(runs=None), dict(n_rows=0),
                                                   dict(rows=None), dict(history=0), dict(history=-1), dict(history=1, normalize=1), dict(dtype=3), dict(dtype=-1),
                                                   dict(label_cols=None), dict(label_src=-1), dict(label_src=n), dict(n_label=11), dict(quat_src=-1), dict(quat_src=n),
                                                   dict(type_nodes=0), dict(type_width=tab.pitch[0] + 1), dict(sign_flags=2 << 8), dict(sign_flags=1 | (9 << 8)))]
    cases += [(dict(y=None), EINVAL),
              (dict(src=arr(C.c_void_p, [None, h.series[1].data_ptr()])), EINVAL),
              (dict(cstride=arr(C.c_int64, [series[0].shape[0] - 1, h.cstride[1]])), EINVAL),
              (dict(rows=arr(C.c_int64, [tab.history - 1, h.src_rows[1]])), EINVAL),
              (dict(x=arr(C.c_void_p, [None])), EINVAL),
              (dict(pitch=arr(C.c_int64, [0])), EINVAL),
              (with_desc(history=257, label_rotate=0), EUNSUPPORTED),
              (with_desc(n_runs=129), EUNSUPPORTED)]
    for over, code in cases:
        keep = over.pop("_keep", None)
        rc = h.call(**over)
        assert rc == code and len(h.lib.mshgnn_last_error()) > 0, (over, keep and {f: getattr(keep, f) for f in fields[:4]}, rc, code)
        assert h.untouched(), over
    assert h.call() == 0 and h.verdict(wr.reference(tab, series, starts)) is None      # (and the harness itself was sound)


# ---- the fused encoders at every split point -------------------------------------------------------------------------------------------------------------
def _split_point_case(plan, history, normalize):
    """A recipe in the style of tests/test_windows.py::_more_than_16_runs: one base row of 12 runs of `history` steps with alternating signs -- with 8 elements
    per 16-byte chunk (bf16) / per splice (fp32) the run boundaries k * history, k = 1 .. 11, fall on every position 1 .. 7 of a chunk for history 9 and 15."""
    from morphsym_hgnn_amd import synth, topology
    from morphsym_hgnn_amd.spec import ModelSpec
    from morphsym_hgnn_amd.windows import SequenceStore, quadsdk_a1_c2_recipe
    from tests import test_windows as tw
    recipe = quadsdk_a1_c2_recipe(tw.JP, tw.FP, history, 3, n_base=1, normalize=normalize)
    recipe.variables["base"] = recipe.variables["base"] * 2
    signs, k = {}, 0
    for t in recipe.node_types:
        signs[t] = []
        for _, cols in recipe.variables.get(t, []):
            signs[t].append([[1 if (k + n + a) % 2 == 0 else -1 for a in range(len(node))] for n, node in enumerate(cols)])
            k += 1
    recipe.variable_signs = signs
    assert recipe.width("base") == 12 * history and {(j * history) % 8 for j in range(1, 12)} >= set(range(1, 8))
    spec = ModelSpec(kind="mi", topology=topology.TOPOLOGIES["quadruped-mi"](), hidden=128, num_layers=2,
                     widths={t: recipe.width(t) for t in recipe.node_types}, regression=True, grf_dimension=3, group=None, num_timesteps=history)
    store = SequenceStore(tw.SEQ, recipe, dtype=plan)
    e = eng.Engine(spec, plan)
    assert not e.generic
    B = 37
    starts = torch.randint(0, tw.N - history + 1, (B,), generator=torch.Generator().manual_seed(history))
    starts[0], starts[-1] = 0, tw.N - history
    flat = eng.flatten_params(spec, synth.make_params(8, spec.param_shapes()), e.device)
    # the gathered windows against the table-reading reference
    names = store.names
    tab = wr.recipe_tables(recipe, names, plan, store.padded_width)
    series = [wr.f32(tw.SEQ[s]).reshape(len(tw.SEQ[s]), -1) for s in names]
    exp = wr.reference(tab, series, starts.tolist())
    return store, e, flat, starts.cuda(), tab, exp


def _windows_match(store, tab, exp, xs, y, starts):
    v = wr.check(tab, exp, [x.reshape(len(starts), n, -1) for x, n in zip(xs, tab.type_nodes)], y.reshape(-1) if y is not None else None, None,
                 starts.tolist(), sentinels=False)
    assert v is None, v
    for x, t in zip(xs, store.recipe.node_types):
        assert not x[:, store.recipe.width(t):].float().abs().sum().item()      # pad columns stay zero


@pytest.mark.parametrize("history", [9, 15])
@pytest.mark.parametrize("plan", ["bf16", "x3"])
def test_fused_routes_at_every_split_point(plan, history):
    """step_mse_series (bf16: with and without x_out), forward_series, and on the standardised recipe step_mse_series_std and forward_series: each bit for bit
    what assemble followed by the dense entry point gives, the assembled windows checked against window_reference: n0 = 1 .. 7 of splice8f, standardise_oct
    and the sign masks."""
    _require_gpu()
    for normalize in (False, True):
        store, e, flat, starts, tab, exp = _split_point_case(plan, history, normalize)
        B = int(starts.numel())
        xs, y, _ = store.assemble(starts)
        xs = [x.clone() for x in xs]; y = y.clone()
        _windows_match(store, tab, exp, xs, y, starts.cpu())
        out_f = e.forward(xs, flat, B, training=False).clone()
        out_a, loss_a, g_a = (t.clone() for t in e.step_mse(xs, flat, y.reshape(-1), B))
        y_e, _, _, out_e = e.forward_series(store, starts, flat)
        torch.cuda.synchronize()
        assert torch.equal(out_e, out_f) and torch.equal(y_e, y), ("forward_series", normalize)
        routes = [("std", None)] if normalize else [("plain", True)] + ([("plain", False)] if plan == "bf16" else [])
        for route, materialize in routes:
            for x, t in zip(store._buffers(B)[0], store.recipe.node_types):
                x.fill_(float("nan")); x[:, store.recipe.width(t):] = 0
            if route == "std":
                xs2, y2, out_b, loss_b, g_b = e.step_mse_series_std(store, starts, flat)
            else:
                xs2, y2, out_b, loss_b, g_b = e.step_mse_series(store, starts, flat, materialize=materialize)
            torch.cuda.synchronize()
            if xs2 is not None:
                assert all(torch.equal(a, b) for a, b in zip(xs, xs2)), (route, materialize)
            assert torch.equal(y, y2) and torch.equal(out_a, out_b) and torch.equal(loss_a, loss_b) and torch.equal(g_a, g_b), (route, materialize)
