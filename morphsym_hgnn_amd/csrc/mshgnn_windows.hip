// mshgnn_assemble_windows (include/mshgnn.h): a batch of windows gathered from a sequence's resident raw series into the engine's input layout, and their labels.
// mshgnn_dataset_starts: the dataset indices of several concatenated sequences -> the start rows the gathers take.
// The series entry points that fuse this gather into the encoder are mshgnn.hip's; WindowArgs (mshgnn_device.hpp) is what the two share.
#include "mshgnn_device.hpp"

// ------------------------------------------------------------------------------------------------------
// On-device window assembly: the raw time series of a sequence stay in HBM and a batch of
// windows [start, start + T) is gathered straight into the engine's input layout [B][n_t][pitch] at the plan dtype --
// what the reference does per window in Python (quadSDKDataset_Morph.py:304-369: axis-major flatten('F') of each
// variable, joint re-ordering, base tiling, all-ones feet) followed by PyG's collate.
// One wave per RUN = T consecutive features of one node row: feature f0 + t = src[start + t][col] (optionally
// standardised over the window like flexibleDataset.py:390-396), or the constant 1.
// ------------------------------------------------------------------------------------------------------
constexpr int WIN_ROW_RUNS = 8;          // runs per node row handled with all loads in flight

// one WORKGROUP per window, its 4 waves take the node rows round-robin.  Lane r resolves run r ONCE (source pointer, destination
// offset, length) and the waves fetch those with v_readlane, so there is no dependent descriptor load per run; every run
// of a row is a contiguous stretch of a column-major series, read coalesced with all of the row's loads in flight.
// ORBIT (with a.sign's K > 1): the window's element picks its block of `runs`; the row structure (a.rows, lengths, destinations) is every element's.
template <typename T, int NSET, bool ORBIT = false> __global__ __launch_bounds__(256) void k_assemble_windows(WindowArgs a) {
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t b = blockIdx.x;
    const int64_t start = ORBIT ? start_row(a.starts[b]) : a.starts[b];
    const int* runs = a.runs;
    if constexpr (ORBIT) runs += (size_t)start_element(a.starts[b], orbit_elements(a.sign)) * a.n_runs * 5;
    // lane r & 63 of register set r >> 6 <- run r (n_runs <= 64 NSET, checked by the host)
    int v_lo[NSET], v_hi[NSET], v_doff[NSET], v_len[NSET], v_t[NSET];
#pragma unroll
    for (int set = 0; set < NSET; ++set) {
        const int* run = (ORBIT ? runs : a.runs) + (size_t)min(lane + 64 * set, a.n_runs - 1) * 5;
        const int t = run[0], node = run[1], f0 = run[2];
        bool neg;
        const int sc = run_source(run[3], a.sign, neg);
        const float* sp = nullptr;
#pragma unroll
        for (int k = 0; k < WIN_MAX_SRC; ++k) if (sc >= 0 && (sc >> 8) == k) sp = a.src[k] + (size_t)(sc & 0xff) * a.src_cstride[k] + start;
        int nodes = 0; int64_t pitch = 0;
#pragma unroll
        for (int k = 0; k < MSHGNN_MAX_TYPES; ++k) if (t == k) { nodes = a.nodes[k]; pitch = a.x_pitch[k]; }
        v_lo[set] = (int)((uintptr_t)sp & 0xffffffffu); v_hi[set] = (int)((uintptr_t)sp >> 32);
        v_doff[set] = (int)(((size_t)b * nodes + node) * pitch + f0 - (size_t)b * nodes * pitch);     // offset inside the window's block of this type
        v_len[set] = run[4] | (neg ? WIN_SIGN_FLAG : 0); v_t[set] = t;      // (lengths are <= 256: the run's sign rides in bit 30)
    }
    auto rl = [&](const int (&v)[NSET], int r) {
        if constexpr (NSET == 1) return __builtin_amdgcn_readlane(v[0], r);
        else return r < 64 ? __builtin_amdgcn_readlane(v[0], r & 63) : __builtin_amdgcn_readlane(v[NSET - 1], r & 63);
    };
    // lane handles the element pairs (2 lane + 128 j, +1), j = 0, 1: one packed store per pair where the run's first destination element sits at an
    // even ELEMENT ADDRESS and its length is even, so pairs are 4-byte (bf16) / 8-byte (fp32) aligned whatever the pitch, the batch index and the
    // base pointer are (the entry point only asks for element-aligned rows); two scalar stores otherwise.  Uniform per run.  Lengths up to 256
    for (int row = wv; row < a.n_rows; row += 4) {
        const int r_begin = a.rows[2 * row], r_end = a.rows[2 * row + 1];
        for (int rb = r_begin; rb < r_end; rb += WIN_ROW_RUNS) {
            float v[WIN_ROW_RUNS][4];
#pragma unroll
            for (int i = 0; i < WIN_ROW_RUNS; ++i) {
                const int r = min(rb + i, r_end - 1);
                const float* sp = reinterpret_cast<const float*>((uintptr_t)(unsigned)rl(v_lo, r) | ((uintptr_t)(unsigned)rl(v_hi, r) << 32));
                const int len = rl(v_len, r) & ~WIN_SIGN_FLAG;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int k = 2 * lane + 128 * (q >> 1) + (q & 1);
                    v[i][q] = 1.0f;
                    if (rb + i < r_end && sp != nullptr && k < len) v[i][q] = sp[k];
                }
            }
#pragma unroll
            for (int i = 0; i < WIN_ROW_RUNS; ++i) {
                if (rb + i >= r_end) break;
                const int r = rb + i;
                const int lw = rl(v_len, r), t = rl(v_t, r), len = lw & ~WIN_SIGN_FLAG, doff = rl(v_doff, r);
                const bool has_src = (rl(v_lo, r) | rl(v_hi, r)) != 0;
                T* dst = reinterpret_cast<T*>(a.x[t]) + (size_t)b * a.nodes[t] * a.x_pitch[t] + doff;
                if (lw & WIN_SIGN_FLAG) {      // a negated run: the sign goes on before the statistics (uniform)
#pragma unroll
                    for (int q = 0; q < 4; ++q) v[i][q] = xor_sign(v[i][q], true);
                }
                if (a.normalize && has_src) {
                    // (x - mean) / std with the unbiased estimator, NaN -> 0 (flexibleDataset.py:390-396); fp64, two passes over registers.  The arithmetic
                    // is run_stats / standardise_one (mshgnn_device.hpp), shared with the standardising series encoders of mshgnn_forward_series
                    const RunStats rs = run_stats(v[i], len, lane);
#pragma unroll
                    for (int q = 0; q < 4; ++q) v[i][q] = standardise_one(v[i][q], rs.mean, rs.sd);
                }
                const bool even = ((((uintptr_t)dst / sizeof(T)) | (uintptr_t)len) & 1) == 0;
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int k = 2 * lane + 128 * j;
                    if (even && k < len) {
                        if constexpr (sizeof(T) == 2) {
                            union { unsigned u; __bf16 e[2]; } pk; pk.e[0] = (__bf16)v[i][2 * j]; pk.e[1] = (__bf16)v[i][2 * j + 1];
                            *reinterpret_cast<unsigned*>(dst + k) = pk.u;
                        } else *reinterpret_cast<f32x2*>(dst + k) = f32x2{v[i][2 * j], v[i][2 * j + 1]};
                    } else {
                        if (k < len) dst[k] = from_f32<T>(v[i][2 * j]);
                        if (k + 1 < len) dst[k + 1] = from_f32<T>(v[i][2 * j + 1]);
                    }
                }
            }
        }
    }
}

// Fast path of the same gather (no standardisation, 16-byte aligned output rows whose runs all have one length -- what SequenceStore builds):
// a thread owns one 16-BYTE CHUNK of one node row -- EPC consecutive features, which live in at most two runs of that length -- gathers them
// with EPC scalar loads (consecutive lanes read consecutive elements of a column-major series) and writes ONE 16-byte store; all chunks of a
// window are independent, so every load of the window is in flight at once.  The general kernel above writes 4 bytes per lane and walks a row's
// runs in turn: 0.12 ms for 8192 A1 windows against 0.03-0.04 ms here.  Pad columns inside a row's last chunk are written as zeros.
constexpr int WIN_MAX_ROWS = 64;
template <typename T, bool ORBIT = false> __global__ __launch_bounds__(256) void k_assemble_windows_fast(WindowArgs a) {
    constexpr int EPC = 16 / (int)sizeof(T);
    __shared__ unsigned long long s_src[WIN_MAX_RUNS];                    // source pointer of run r at this window's first step (0: the constant 1)
    __shared__ int s_first[WIN_MAX_ROWS + 1];                             // chunk prefix per node row
    __shared__ int s_run0[WIN_MAX_ROWS], s_len[WIN_MAX_ROWS], s_width[WIN_MAX_ROWS];
    __shared__ unsigned long long s_dst[WIN_MAX_ROWS];                    // destination of the row's first element
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x, start = ORBIT ? start_row(a.starts[b]) : a.starts[b];
    if (tid < a.n_runs) {
        bool neg;
        // (ORBIT: the source word of the window's element's block; the row structure read below is element 0's, which the host check made every element's)
        const size_t rblk = ORBIT ? (size_t)start_element(a.starts[b], orbit_elements(a.sign)) * a.n_runs : 0;
        const int sc = run_source(a.runs[(rblk + tid) * 5 + 3], a.sign, neg);
        const float* sp = nullptr;
#pragma unroll
        for (int k = 0; k < WIN_MAX_SRC; ++k) if (sc >= 0 && (sc >> 8) == k) sp = a.src[k] + (size_t)(sc & 0xff) * a.src_cstride[k] + start;
        s_src[tid] = (unsigned long long)sp | (neg && sp ? RUN_PTR_SIGN : 0ull);      // (a chunk's elements may come from two runs of opposite signs: per element)
    }
    if (tid < a.n_rows) {
        const int r0 = a.rows[2 * tid], r1 = a.rows[2 * tid + 1];
        const int* run = a.runs + (size_t)r0 * 5;
        const int t = run[0], node = run[1], len = run[4];
        int nodes = 0; int64_t pitch = 0; char* xb = nullptr;
#pragma unroll
        for (int k = 0; k < MSHGNN_MAX_TYPES; ++k) if (t == k) { nodes = a.nodes[k]; pitch = a.x_pitch[k]; xb = reinterpret_cast<char*>(a.x[k]); }
        s_run0[tid] = r0; s_len[tid] = len; s_width[tid] = (r1 - r0) * len;
        s_dst[tid] = (unsigned long long)(xb + (((size_t)b * nodes + node) * pitch + run[2]) * sizeof(T));
    }
    __syncthreads();
    if (tid == 0) {
        int acc = 0;
        for (int r = 0; r < a.n_rows; ++r) { s_first[r] = acc; acc += (s_width[r] + EPC - 1) / EPC; }
        s_first[a.n_rows] = acc;
    }
    __syncthreads();
    const int total = s_first[a.n_rows];
    int row = 0;
    for (int task = tid; task < total; task += 256) {
        while (task >= s_first[row + 1]) ++row;                            // (tasks of a thread ascend)
        const int j = task - s_first[row], len = s_len[row], width = s_width[row];
        const int k0 = j * EPC;
        int run = s_run0[row] + k0 / len, off = k0 % len;
        float v[EPC];
#pragma unroll
        for (int e = 0; e < EPC; ++e) {
            v[e] = 0.f;
            if (k0 + e < width) {
                const unsigned long long p = s_src[run];
                const float* sp = reinterpret_cast<const float*>(run_ptr_addr(p));
                v[e] = sp ? xor_sign(sp[off], (p & RUN_PTR_SIGN) != 0) : 1.0f;
            }
            if (++off == len) { off = 0; ++run; }
        }
        T* dst = reinterpret_cast<T*>(s_dst[row]) + k0;
        if constexpr (sizeof(T) == 2) {
            union { u32x4 u; __bf16 e[8]; } pk;
#pragma unroll
            for (int e = 0; e < 8; ++e) pk.e[e] = (__bf16)v[e];
            *reinterpret_cast<u32x4*>(dst) = pk.u;
        } else *reinterpret_cast<f32x4*>(dst) = f32x4{v[0], v[1], v[2], v[3]};
    }
}

// labels of a window = the label row of its LAST time step (quadSDKDataset.py: grfs[-1]); with label_rotate the world-frame
// GRFs are taken into the body frame with the world->body quaternion of that step, R f per foot (the as_matrix() @ grfs_T
// branch of load_data_at_dataset_seq_3d); quat out = that quaternion (data.r_o, quadSDKDataset_Morph.py:365-367)
// (window_labels_one itself lives in mshgnn_device.hpp: the fused-gather encoders run it in extra workgroups of their own launch)
__device__ __forceinline__ LabelArgs label_args_of(const WindowArgs& a, int32_t* labels_int) {
    LabelArgs l{};
    l.lab = a.src[a.label_src]; l.lab_cs = a.src_cstride[a.label_src];
    l.quat_src = a.quat_src >= 0 ? a.src[a.quat_src] : nullptr; l.quat_cs = a.quat_src >= 0 ? a.src_cstride[a.quat_src] : 0;
    l.starts = a.starts; l.B = a.B; l.T = a.T; l.label_cols = a.label_cols; l.n_label = a.n_label; l.label_rotate = a.label_rotate;
    l.y = a.y; l.quat = a.quat; l.labels_int = labels_int; l.sign = a.sign;
    return l;
}

__global__ void k_window_labels(WindowArgs a) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b < a.B) window_labels_one(label_args_of(a, nullptr), b);
}
__global__ void k_window_labels_orbit(WindowArgs a) {      // K > 1: the label columns of each window's own element
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b < a.B) window_labels_one<true>(label_args_of(a, nullptr), b);
}

// The sign tables of a descriptor (sign_flags bit 0) are the caller's statement about DEVICE memory; before the first launch that reads them they are copied back
// once and checked, afterwards the caller vouches (bit 1).  What is refused: see MSHGNN_WINDOW_SIGN_FLAG in include/mshgnn.h.
// Orbit descriptors (sign_flags bits 8..15 = K > 1): all K element blocks are read back; besides every block's sign words, what makes a per-window choice of block safe
// is checked -- K <= 8, the row structure {type, node, first feature, length} of every run equal to element 0's, constant-1 runs constant-1 in every element.
int check_sign_tables(const mshgnn_window_desc* d, bool labels, hipStream_t st) {
    const int K = desc_elements(d);
    if (K > 1 && !(d->sign_flags & 1)) return set_err(MSHGNN_EINVAL, "window descriptor: K > 1 group elements imply sign_flags bit 0");
    if (K > MSHGNN_WINDOW_MAX_ELEMENTS) return set_err(MSHGNN_EINVAL, "window descriptor: " + std::to_string(K) + " group elements, at most " + std::to_string(MSHGNN_WINDOW_MAX_ELEMENTS) + " are supported");
    if (!(d->sign_flags & 1) || (d->sign_flags & 2)) return MSHGNN_OK;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (st && hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone)
        return set_err(MSHGNN_EINVAL, "sign tables must be checked by a call outside a stream capture first (then vouch with sign_flags bit 1)");
    if (d->n_runs < 1 || d->n_runs > WIN_MAX_RUNS || !d->runs) return set_err(MSHGNN_EINVAL, "bad window descriptor");
    std::vector<int32_t> runs((size_t)K * d->n_runs * 5), lab(labels && d->n_label > 0 ? (size_t)K * d->n_label : 0);
    HIPCHK(hipMemcpy(runs.data(), d->runs, runs.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (!lab.empty()) {
        if (!d->label_cols) return set_err(MSHGNN_EINVAL, "bad label description");
        HIPCHK(hipMemcpy(lab.data(), d->label_cols, lab.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    for (int e = 0; e < K; ++e)
        for (int r = 0; r < d->n_runs; ++r) {
            const int32_t* run = &runs[((size_t)e * d->n_runs + r) * 5], * run0 = &runs[(size_t)r * 5];
            const std::string who = (K > 1 ? "element " + std::to_string(e) + ", " : std::string()) + "window run " + std::to_string(r);
            if (run[0] != run0[0] || run[1] != run0[1] || run[2] != run0[2] || run[4] != run0[4])
                return set_err(MSHGNN_EINVAL, who + ": {type, node, first feature, length} differs from element 0's");
            const int32_t w = run[3];
            if ((w == -1) != (run0[3] == -1)) return set_err(MSHGNN_EINVAL, who + ": a constant-1 run must be constant-1 in every element");
            if (w == -1) continue;
            if (w < 0) return set_err(MSHGNN_EINVAL, who + ": a constant-1 run (source word -1) cannot carry a sign");
            if (((w & ~MSHGNN_WINDOW_SIGN_FLAG) >> 8) >= d->n_src) return set_err(MSHGNN_EINVAL, who + ": source out of range");
        }
    for (size_t k = 0; k < lab.size(); ++k)
        if (lab[k] < 0 || (lab[k] & ~MSHGNN_WINDOW_SIGN_FLAG) >= 256) return set_err(MSHGNN_EINVAL, "label column " + std::to_string(k % (size_t)d->n_label) + ": column part out of range [0, 256)");
    return MSHGNN_OK;
}

extern "C" int mshgnn_assemble_windows(const mshgnn_window_desc* d, const float* const* src, const int64_t* src_cstride, const int64_t* src_rows,
                                       const int64_t* starts, int64_t batch, void* const* x_out, const int64_t* x_pitch, float* y_out,
                                       float* quat_out, void* stream) {
    if (!d || !src || !src_cstride || !src_rows || !starts || !x_out || !x_pitch || batch < 1) return set_err(MSHGNN_EINVAL, "null argument to mshgnn_assemble_windows");
    if (d->n_types < 1 || d->n_types > MSHGNN_MAX_TYPES || d->n_src < 1 || d->n_src > WIN_MAX_SRC || d->n_runs < 1 || !d->runs || d->n_rows < 1 || !d->rows)
        return set_err(MSHGNN_EINVAL, "bad window descriptor");
    if (d->history < 1 || (d->normalize && d->history < 2)) return set_err(MSHGNN_EINVAL, "history must be >= 1 (>= 2 when normalising)");
    if (d->dtype != MSHGNN_F32 && d->dtype != MSHGNN_BF16 && d->dtype != MSHGNN_BF16X3) return set_err(MSHGNN_EINVAL, "dtype must be MSHGNN_F32, MSHGNN_BF16 or MSHGNN_BF16X3");
    if (d->n_label > 0 && (!d->label_cols || !y_out || d->label_src < 0 || d->label_src >= d->n_src)) return set_err(MSHGNN_EINVAL, "bad label description");
    if (d->label_rotate && (d->n_label % 3 != 0 || d->quat_src < 0)) return set_err(MSHGNN_EINVAL, "label rotation needs 3-D labels and a quaternion source");
    if (d->quat_src >= d->n_src) return set_err(MSHGNN_EINVAL, "quat_src out of range");
    WindowArgs a{};
    for (int i = 0; i < d->n_src; ++i) {
        if (!src[i] || src_cstride[i] < src_rows[i] || src_rows[i] < d->history) return set_err(MSHGNN_EINVAL, "bad source array");
        a.src[i] = src[i]; a.src_cstride[i] = src_cstride[i];
    }
    for (int t = 0; t < d->n_types; ++t) {
        if (!x_out[t] || d->type_nodes[t] < 1 || x_pitch[t] < d->type_width[t]) return set_err(MSHGNN_EINVAL, "bad output tensor");
        a.x[t] = x_out[t]; a.x_pitch[t] = x_pitch[t]; a.nodes[t] = d->type_nodes[t];
    }
    if (d->history > 256) return set_err(MSHGNN_EUNSUPPORTED, "history longer than 256 steps is not supported by this build");
    a.runs = d->runs; a.n_runs = d->n_runs; a.rows = d->rows; a.n_rows = d->n_rows; a.starts = starts; a.B = batch; a.T = d->history; a.normalize = d->normalize;
    a.label_cols = d->label_cols; a.n_label = d->n_label; a.label_src = d->label_src; a.label_rotate = d->label_rotate; a.quat_src = d->quat_src;
    a.y = y_out; a.quat = quat_out; a.sign = desc_sign_word(d);
    const bool orbit = desc_elements(d) > 1;
    hipStream_t st = (hipStream_t)stream;
    if (const int rc = check_sign_tables(d, d->n_label > 0, st)) return rc;
    if (d->n_runs > 128) return set_err(MSHGNN_EUNSUPPORTED, "more than 128 feature runs per window are not supported by this build");
    // fast path: no standardisation, every row's runs of one length starting at the row's first feature 0, 16-byte aligned rows whose pitch covers whole chunks
    const bool f32 = d->dtype == MSHGNN_F32 || d->dtype == MSHGNN_BF16X3;      // the split plan takes fp32 inputs
    bool fast = !d->normalize && d->n_rows <= WIN_MAX_ROWS && d->n_runs <= WIN_MAX_RUNS && d->fast_layout != 0;
    for (int t = 0; t < d->n_types && fast; ++t) {
        const int epc = f32 ? 4 : 8;
        if (((uintptr_t)x_out[t] & 15) || x_pitch[t] % epc || x_pitch[t] < (d->type_width[t] + epc - 1) / epc * epc) fast = false;
    }
    if (orbit) {      // a group element per window: the ORBIT instantiations of the same kernels
        if (fast) {
            if (f32) hipLaunchKernelGGL((k_assemble_windows_fast<float, true>), dim3((unsigned)batch), dim3(256), 0, st, a);
            else hipLaunchKernelGGL((k_assemble_windows_fast<__bf16, true>), dim3((unsigned)batch), dim3(256), 0, st, a);
        } else if (f32) {
            if (d->n_runs <= 64) hipLaunchKernelGGL((k_assemble_windows<float, 1, true>), dim3((unsigned)batch), dim3(256), 0, st, a);
            else hipLaunchKernelGGL((k_assemble_windows<float, 2, true>), dim3((unsigned)batch), dim3(256), 0, st, a);
        } else {
            if (d->n_runs <= 64) hipLaunchKernelGGL((k_assemble_windows<__bf16, 1, true>), dim3((unsigned)batch), dim3(256), 0, st, a);
            else hipLaunchKernelGGL((k_assemble_windows<__bf16, 2, true>), dim3((unsigned)batch), dim3(256), 0, st, a);
        }
    } else if (fast) {
        if (f32) hipLaunchKernelGGL(k_assemble_windows_fast<float>, dim3((unsigned)batch), dim3(256), 0, st, a);
        else hipLaunchKernelGGL(k_assemble_windows_fast<__bf16>, dim3((unsigned)batch), dim3(256), 0, st, a);
    } else if (f32) {
        if (d->n_runs <= 64) hipLaunchKernelGGL((k_assemble_windows<float, 1>), dim3((unsigned)batch), dim3(256), 0, st, a);
        else hipLaunchKernelGGL((k_assemble_windows<float, 2>), dim3((unsigned)batch), dim3(256), 0, st, a);
    } else {
        if (d->n_runs <= 64) hipLaunchKernelGGL((k_assemble_windows<__bf16, 1>), dim3((unsigned)batch), dim3(256), 0, st, a);
        else hipLaunchKernelGGL((k_assemble_windows<__bf16, 2>), dim3((unsigned)batch), dim3(256), 0, st, a);
    }
    if (d->n_label > 0 || (quat_out && d->quat_src >= 0)) {
        if (orbit) hipLaunchKernelGGL(k_window_labels_orbit, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, st, a);
        else hipLaunchKernelGGL(k_window_labels, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, st, a);
    }
    HIPCHK(hipGetLastError());
    return MSHGNN_OK;
}

// ------------------------------------------------------------------------------------------------------
// A dataset of several sequences (train_regression-grf_msgn.py:57-73: ConcatDataset of per-sequence Subsets): the sequences' series are concatenated
// row-wise, a view takes a window range per sequence, and a dataset index becomes a start row of the concatenated series.  One thread per index:
// binary search for the sequence over the cumulative window counts (8 bytes each: up to DATASET_LDS_SEQ sequences they are staged in LDS once per
// workgroup, ten dependent LDS reads per index instead of ten trips to L2; beyond that the search reads global memory), one load of the sequence's
// first row, one store.  Invariant of the search: cum[lo] <= i < cum[hi], so an empty range (cum[s] == cum[s + 1]) is never the answer and lo stays
// inside [0, n_seq - 1] whatever cum holds.  An index outside the view gets row 0 and raises the caller's flag with a plain store of 1.
// ------------------------------------------------------------------------------------------------------
constexpr int DATASET_LDS_SEQ = 1024;

template <bool LDS> __global__ __launch_bounds__(256) void k_dataset_starts(const int64_t* __restrict__ cum, const int64_t* __restrict__ first_row, int n_seq,
                                                                            const int64_t* __restrict__ index, int64_t batch, int64_t* __restrict__ starts,
                                                                            int32_t* __restrict__ bad) {
    __shared__ int64_t s_cum[LDS ? DATASET_LDS_SEQ + 1 : 1];
    if constexpr (LDS) {
        for (int k = threadIdx.x; k <= n_seq; k += 256) s_cum[k] = cum[k];
        __syncthreads();
    }
    const int64_t* c = LDS ? s_cum : cum;
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= batch) return;
    const int64_t i = index[b];
    if (i < 0 || i >= c[n_seq]) {
        starts[b] = 0;
        bad[0] = 1;
        return;
    }
    int lo = 0, hi = n_seq;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (c[mid] <= i) lo = mid; else hi = mid;
    }
    starts[b] = first_row[lo] + (i - c[lo]);
}

extern "C" int mshgnn_dataset_starts(const int64_t* cum, const int64_t* first_row, int32_t n_seq, const int64_t* index, int64_t batch, int64_t* starts_out,
                                     int32_t* bad_out, void* stream) {
    if (!cum || !first_row || !index || !starts_out || !bad_out) return set_err(MSHGNN_EINVAL, "null argument to mshgnn_dataset_starts");
    if (n_seq < 1) return set_err(MSHGNN_EINVAL, "mshgnn_dataset_starts: n_seq must be >= 1");
    if (batch < 1) return set_err(MSHGNN_EINVAL, "mshgnn_dataset_starts: batch must be >= 1");
    if (batch > ((int64_t)1 << 31) * 256 - 256) return set_err(MSHGNN_EUNSUPPORTED, "mshgnn_dataset_starts: more than 2^39 indices in one call");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((batch + 255) / 256));
    if (n_seq <= DATASET_LDS_SEQ) hipLaunchKernelGGL(k_dataset_starts<true>, grid, dim3(256), 0, st, cum, first_row, (int)n_seq, index, batch, starts_out, bad_out);
    else hipLaunchKernelGGL(k_dataset_starts<false>, grid, dim3(256), 0, st, cum, first_row, (int)n_seq, index, batch, starts_out, bad_out);
    HIPCHK(hipGetLastError());
    return MSHGNN_OK;
}
