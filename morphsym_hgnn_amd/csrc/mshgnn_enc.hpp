// The encoder kernels of the three LDS-resident plans: device templates only.  mshgnn.hip instantiates k_enc_fwd (fp32 / bf16 plans), mshgnn_x3.hip k_enc_x3 (split plan).
//   X_0[node] = relu((mask . x) W_enc^T + b)      (hgnn_c2.py:143-147)
// One workgroup = MB row blocks of ONE node; K is streamed in chunks of 128 through LDS with the next chunk prefetched in registers.  Shared: the decode of a workgroup's
// role (enc_role), how a chunk of a window row divides between two runs of the series (series_split, ChunkState), the fp32 gather of such a chunk (series_fetch_f32), the
// ReLU-bit epilogue (enc_relu_bits).  Each kernel's own, on purpose: the K loop, the LDS staging (raw chunks against hi + lo planes), the MACs (one product against three),
// the output store and WHERE THE MATERIALISED WINDOW ROWS ARE STORED: k_enc_fwd behind the next chunk's loads (its vmcnt comment says why), k_enc_x3 in the staging pass.
// The template switches (both kernels; k_enc_x3 has no T):
// ALIGNED: every input row starts 16-byte aligned with a pitch of whole 16-byte chunks (the engine's own input layout): raw 16-byte loads only -- the general
// element-wise path is compiled out of this instantiation (a third of the kernel's code).
// SERIES (with ALIGNED; k_enc_fwd: bf16): the rows come out of the sequence's resident series (SeriesSrc) and are ALSO written to a.x as materialised windows (the
// weight-gradient kernel reads them later): window assembly fused into the encoder, no separate gather pass over 118 MB.  Element k of a node row = element
// starts[w] + k % T of run k / T.  bf16 series: one unaligned (2-byte aligned, served at full rate) 16-byte load per chunk, two and splice8 where the chunk
// straddles two runs; fp32 series (k_enc_x3, k_enc_fwd<.., NORM>): two 4-byte-aligned 16-byte loads per piece and splice8f (series_fetch_f32).
// SRC (8 / 4, with ALIGNED, without SERIES; k_enc_fwd: bf16): the rows come from the caller's own fp64 / fp32 tensors at their dense pitch (WideSrc, mshgnn_device.hpp),
// are converted in registers and ALSO written to a.x as plan-dtype rows at the engine's pitch for the weight-gradient kernel -- the cast + re-pitch pass fused into
// the encoder (mshgnn_*_src entry points).
// NORM (with SERIES; mshgnn_forward_series / mshgnn_step_*_series_std on a standardised recipe): every run with a source column is standardised over its window with
// the statistics k_series_stats left in ser.stats -- fp64 -> fp32 (-> bf16), the roundings of mshgnn_assemble_windows(normalize) (standardise_one, mshgnn_device.hpp).
// Evaluation materialises nothing (a.x null); the training steps get the standardised rows written to a.x like the plain SERIES rows.
// SIGN (with SERIES; a descriptor with sign_flags): the run pointers may carry RUN_PTR_SIGN -- the chunk's elements are negated per element (sign_mask8_*: a chunk's
// two runs may differ) before the standardisation and before the window rows are written out, so a.x receives g . window.  Unsigned descriptors launch the
// instantiations without it: the code they always ran.
// ORBIT (with SIGN; a descriptor with K > 1 group elements, include/mshgnn.h): every window row of a tile has its own element, so the run pointers -- address and sign --
// stop being uniform over the tile: next to srow[] each thread keeps its window rows' elements (erow[]; k_enc_x3: their run-table offsets erun[]) and fetches pa / pb per window row; how a
// chunk divides between two runs (j, off, n0, whether a run has a source column) is the row structure, which all elements share.  Only the ORBIT instantiations pay for it.
#pragma once
#include "mshgnn_device.hpp"
__device__ __forceinline__ u32x4 splice8(u32x4 A, u32x4 B, int n0) {      // bf16 elements A[0 .. n0) ++ B[0 .. 8 - n0), 0 < n0 < 8
    const unsigned __int128 a = ((unsigned __int128)(((unsigned long long)A[3] << 32) | A[2]) << 64) | (((unsigned long long)A[1] << 32) | A[0]);
    const unsigned __int128 b = ((unsigned __int128)(((unsigned long long)B[3] << 32) | B[2]) << 64) | (((unsigned long long)B[1] << 32) | B[0]);
    const int sh = 16 * n0;
    const unsigned __int128 r = (a & ((((unsigned __int128)1) << sh) - 1)) | (b << sh);
    return u32x4{(unsigned)r, (unsigned)(r >> 32), (unsigned)(r >> 64), (unsigned)(r >> 96)};
}

// What a workgroup of an encoder launch does.  SERIES: the FIRST workgroups compute the batch's window labels (SeriesSrc.lab) -- chains of dependent round trips that finish
// under the encoder's body (as the last workgroups they stretched its tail instead: measured); enc_role runs them.  Behind the encoder's own workgroups (wg_prefix[n_types])
// come those of the embedded layer-pack prep (EncArgs.prep): reported with their index (prep_wg), the kernel calls its plan's prep.  The others encode one (type, node, tile).
enum EncWg { ENC_WG_LABELS, ENC_WG_PREP, ENC_WG_ENCODE };
struct EncRole {
    int prep_wg;             // ENC_WG_PREP: which of the prep's workgroups
    int t, node, tile;
    bool skip;               // window rows only: nobody reads this node's X_0 (uniform; EncArgs.skip_mask)
    int F, nt, nkc, vb;      // nt: nodes of the type in the input rows (not the launch's list)
    const uint8_t* sg; const float* bias; int64_t pitch;
};
template <bool SERIES, bool ORBIT = false> __device__ __forceinline__ EncWg enc_role(const EncArgs& a, const SeriesSrc& ser, int tid, EncRole& r) {
    const int lab_blocks = SERIES ? (int)((ser.lab.B + 255) / 256) : 0;
    if constexpr (SERIES) {
        if ((int)blockIdx.x < lab_blocks) {
            const int64_t b = (int64_t)blockIdx.x * 256 + tid;
            if (b < ser.lab.B) window_labels_one<ORBIT>(ser.lab, b);
            return ENC_WG_LABELS;
        }
    }
    const int bid = (int)blockIdx.x - lab_blocks;
    if (bid >= a.wg_prefix[a.n_types]) { r.prep_wg = bid - a.wg_prefix[a.n_types]; return ENC_WG_PREP; }
    int t = 0;
    while (t + 1 < a.n_types && bid >= a.wg_prefix[t + 1]) ++t;
    const int local = bid - a.wg_prefix[t];
    r.t = t;
    r.node = a.node_list[a.node_off[t] + (ENC_ORDER ? local % a.nodes[t] : local / a.tiles)]; r.tile = ENC_ORDER ? local / a.nodes[t] : local % a.tiles;
    r.skip = SERIES && ((a.skip_mask >> (a.tbase[t] + r.node)) & 1ull) != 0;
    r.pitch = a.pitch[t];
    r.F = a.width[t]; r.nt = a.tbase[t + 1] - a.tbase[t]; r.nkc = a.nkc[t]; r.vb = a.vb[t];
    r.sg = a.signs + a.sign_off[t] + (size_t)r.node * r.nkc * H;
    r.bias = a.bias + (size_t)max(a.bias_idx[t], 0) * H;      // (a type whose X_0 nobody reads has no packs and no bias row: skip)
    return ENC_WG_ENCODE;
}

// How elements [k0, k0 + 8) of a node row divide between the runs of the series: n0 of them from run j at time offset off, the rest (second) from run j + 1 at offset 0;
// pa / pb: the runs' column pointers, 0 = the constant-1 run (or nothing to read).  SIGN: the pointers' sign flags go into the state and are masked off.  run_ptr_of(jj) is each
// kernel's own, on purpose: k_enc_fwd keeps the row's first 16 run pointers in LDS (no dependent load in front of a chunk's data loads), k_enc_x3 reads the global table.
struct ChunkState {      // of the chunk in flight: set by fetch, read by the next staging pass (standardise_oct, sign_mask8_*)
    int n0 = 8; bool has_a = false, has_b = false, neg_a = false, neg_b = false;
};
struct SeriesSplit { int j, off; bool second; unsigned long long pa, pb; ChunkState st; };
template <bool SIGN, typename RunPtr> __device__ __forceinline__ SeriesSplit series_split(int k0, int nvalid, int T, RunPtr run_ptr_of) {
    SeriesSplit s;
    s.j = k0 / T; s.off = k0 - s.j * T; s.st.n0 = min(8, T - s.off);
    s.second = nvalid > s.st.n0;
    s.pa = nvalid > 0 ? run_ptr_of(s.j) : 0ull; s.pb = s.second ? run_ptr_of(s.j + 1) : 0ull;
    if constexpr (SIGN) {
        s.st.neg_a = (s.pa & RUN_PTR_SIGN) != 0; s.st.neg_b = (s.pb & RUN_PTR_SIGN) != 0;
        s.pa = run_ptr_addr(s.pa); s.pb = run_ptr_addr(s.pb);
    }
    s.st.has_a = s.pa != 0ull; s.st.has_b = s.pb != 0ull;
    return s;
}

// One window's 8 fp32 elements of a chunk as (a0, a1): srow = the window's first series row, any = the chunk has an element inside the row.  The loads are 4-byte aligned; the
// second of a piece may run up to 7 elements past the window's last step: the columns' slack.  NORM: stats -> {mean, sd} of (window, run j), then of run j + 1; runs without a
// source column keep {0, 1}.  STATS_FIRST: the statistics loads go out in front of the data loads (k_enc_x3) or behind their run's (k_enc_fwd): the order each was measured with.
template <bool NORM, bool STATS_FIRST> __device__ __forceinline__ void series_fetch_f32(const SeriesSplit& s, bool any, int srow, const double* stats, u32x4& a0, u32x4& a1, RunStats& rsa, RunStats& rsb) {
    const u32x4 ones = u32x4{0x3f800000u, 0x3f800000u, 0x3f800000u, 0x3f800000u};      // the constant-1 run
    auto stats_of = [&](int run) { const f64x2 sv = *reinterpret_cast<const f64x2*>(stats + 2 * run); return RunStats{sv[0], sv[1]}; };
    a0 = any ? ones : u32x4{0, 0, 0, 0}; a1 = a0;
    if constexpr (NORM) {
        rsa = RunStats{0.0, 1.0}; rsb = RunStats{0.0, 1.0};
        if constexpr (STATS_FIRST) { if (s.pa) rsa = stats_of(0); if (s.pb) rsb = stats_of(1); }
    }
    if (s.pa) {
        const float* sp = reinterpret_cast<const float*>(s.pa) + srow + s.off;
        a0 = *reinterpret_cast<const u32x4*>(sp); a1 = *reinterpret_cast<const u32x4*>(sp + 4);
        if constexpr (NORM && !STATS_FIRST) rsa = stats_of(0);
    }
    if (s.second) {
        u32x4 b0 = ones, b1 = ones;
        if (s.pb) {
            const float* sp = reinterpret_cast<const float*>(s.pb) + srow;
            b0 = *reinterpret_cast<const u32x4*>(sp); b1 = *reinterpret_cast<const u32x4*>(sp + 4);
            if constexpr (NORM && !STATS_FIRST) rsb = stats_of(1);
        }
        splice8f(a0, a1, b0, b1, s.st.n0);
    }
}

// ReLU of one 16-window block's accumulator in place + its relu bytes (training: read by the backward stack kernels at layer 0); w_blk: the block's first window
template <typename T> __device__ __forceinline__ void enc_relu_bits(const EncArgs& a, typename Prec<T>::Acc& acc, int gnode, int w_blk, int wv, int lane) {
    if (w_blk < a.B) {     // uniform: the 16-window block exists (rows past the batch land in the mask buffer's padding)
        const unsigned bits = relu_with_bits<T>(acc);
        if (a.mask0) a.mask0[relu_tile_base(gnode, a.B, w_blk >> 4, wv) + lane] = (uint8_t)bits;
    }
}

// ---- k_enc_fwd: the fp32 / bf16 plans; MB = Prec<T>::ENC_MB row blocks (of 16 windows) per workgroup ----
template <typename T, bool ALIGNED, bool SERIES = false, int SRC = 0, bool NORM = false, bool SIGN = false, bool ORBIT = false> __global__ __launch_bounds__(256) void k_enc_fwd(EncArgs a, SeriesSrc ser, WideSrc wsrc) {
    using P = Prec<T>;
    static_assert(!ORBIT || SIGN, "a group element per window: part of the signed series gather");
    static_assert(!NORM || SERIES, "standardisation is part of the series gather");
    static_assert(!SIGN || SERIES, "signs are part of the series gather");
    static_assert(!SERIES || (sizeof(T) == 2 && ALIGNED), "the series gather is a bf16 path");
    static_assert(SRC == 0 || (sizeof(T) == 2 && ALIGNED && !SERIES), "wide source rows: bf16 plan, aligned destination rows");
    constexpr int MB = P::ENC_MB;
    constexpr int VPB = P::ROWS * P::CPR, NIT = VPB / 256 > 0 ? VPB / 256 : 1, BPP = 256 / VPB > 0 ? 256 / VPB : 1;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    EncRole r;
    const EncWg role = enc_role<SERIES, ORBIT>(a, ser, tid, r);
    if (role != ENC_WG_ENCODE) {
        if constexpr (sizeof(T) == 2 && ALIGNED && !SERIES) if (role == ENC_WG_PREP) prep_one<T, false>(a.prep, r.prep_wg * 256 + tid, false);      // (bf16 plan; see EncArgs.prep)
        return;
    }
    const int t = r.t, node = r.node, F = r.F, nt = r.nt, nkc = r.nkc;
    const bool skip = r.skip;
    const int64_t pitch = r.pitch;
    const int w0 = r.tile * MB * P::ROWS;
    const T* x = reinterpret_cast<const T*>(a.x[t]);
    const T* wpack = reinterpret_cast<const T*>(a.wpack);

    typename P::Acc acc[MB];
#pragma unroll
    for (int m = 0; m < MB; ++m) acc_init_bias<T>(acc[m], r.bias, wv, lane);
    // staging map: fp32 block = 512 chunks -> 2 per thread; bf16 block = 256 chunks -> 1 per thread
    const int c = tid % P::CPR, r0 = (tid % VPB) / P::CPR, sub = tid / VPB;   // sub is 0 for fp32
    typename P::BFrag bf;
    typename P::AFrag af;
    const AOff<T> ao(lane);      // fragment offsets once per kernel (the generic load_afrag rebuilds them per call: 14 VALU instructions)
    u32x4 v[MB / BPP][NIT];
    u32x4 rawv[(SERIES || SRC) ? MB / BPP : 1][NIT];      // SERIES / SRC: the chunk being multiplied, kept until its window rows have been written
    u32x2 wv8[SRC ? MB / BPP : 1][SRC ? SRC : 1];          // SRC: the chunk's 8 source elements as 8-byte units, untouched until the staging pass
    const bool unit_ok = SRC == 8 || (F & 1) == 0;        // every 8-byte unit of a row is wholly valid or wholly past its end (uniform)
    const int64_t spitch = SRC ? wsrc.pitch[t] : 0;
    int srow[SERIES ? MB / BPP : 1];      // SERIES: first series row of this thread's window rows
    // NORM: the chunk's fp32 elements and the statistics of its two runs per window
    u32x4 vn[NORM ? MB / BPP : 1][2];
    RunStats rsa[NORM ? MB / BPP : 1], rsb[NORM ? MB / BPP : 1];
    ChunkState cs;
    // SERIES: the column pointers of this node row's first 16 runs (a chunk takes its pieces from runs j, j + 1); ORBIT: of every element, 16 each
    __shared__ unsigned long long rp_s[SERIES ? (ORBIT ? 16 * MSHGNN_WINDOW_MAX_ELEMENTS : 16) : 1];
    int rfirst = 0, rend = 0;      // SERIES: the node row's runs
    int erow[ORBIT ? MB / BPP : 1];      // ORBIT: the element of this thread's window rows
    bool neg_a[ORBIT ? MB / BPP : 1], neg_b[ORBIT ? MB / BPP : 1];      // ORBIT: the signs of the chunk in flight per window row (cs.neg_a / neg_b otherwise)
    if constexpr (SERIES) {
#pragma unroll
        for (int mi = 0; mi < MB / BPP; ++mi) {
            const int64_t sw = ser.starts[min(w0 + (mi * BPP + sub) * P::ROWS + r0, a.B - 1)];
            srow[mi] = (int)(ORBIT ? start_row(sw) : sw);
            if constexpr (ORBIT) erow[mi] = start_element(sw, orbit_elements(ser.sign));
        }
        rfirst = ser.rows[2 * (ser.row0[t] + node)]; rend = ser.rows[2 * (ser.row0[t] + node) + 1];
        if constexpr (ORBIT) {
            if (tid < 16 * orbit_elements(ser.sign)) rp_s[tid] = rfirst + (tid & 15) < rend ? ser.run_ptr[(size_t)(tid >> 4) * ser.n_runs + rfirst + (tid & 15)] : 0ull;
        } else if (tid < 16) rp_s[tid] = rfirst + tid < rend ? ser.run_ptr[rfirst + tid] : 0ull;
        __syncthreads();
    }
    auto fetch = [&](int kc) {
        const int k0 = kc * H + c * P::EPC;
        const int nvalid = min(P::EPC, F - k0);
        if constexpr (SERIES) {
            // (runs past the 16th -- a node row of more than 16 T-long variables -- come from the global table: a dependent load, rare recipes only)
            auto run_ptr_of = [&](int e, int jj) -> unsigned long long {
                if constexpr (ORBIT) return jj < 16 ? rp_s[16 * e + jj] : (rfirst + jj < rend ? ser.run_ptr[(size_t)e * ser.n_runs + rfirst + jj] : 0ull);
                else return jj < 16 ? rp_s[jj] : (rfirst + jj < rend ? ser.run_ptr[rfirst + jj] : 0ull);
            };
            // (ORBIT: element 0's split gives the chunk's geometry and which runs have a source column -- the row structure every element shares)
            const SeriesSplit s = series_split<SIGN>(k0, nvalid, ser.T, [&](int jj) -> unsigned long long { return run_ptr_of(0, jj); });
            cs = s.st;
            if constexpr (NORM) {
#pragma unroll
                for (int mi = 0; mi < MB / BPP; ++mi) {
                    if constexpr (ORBIT) {
                        const SeriesSplit se = series_split<SIGN>(k0, nvalid, ser.T, [&](int jj) -> unsigned long long { return run_ptr_of(erow[mi], jj); });
                        neg_a[mi] = se.st.neg_a; neg_b[mi] = se.st.neg_b;
                        const double* sp2 = ser.stats + ((size_t)min(w0 + (mi * BPP + sub) * P::ROWS + r0, a.B - 1) * ser.n_runs + rfirst + se.j) * 2;
                        series_fetch_f32<true, false>(se, nvalid > 0, srow[mi], sp2, vn[mi][0], vn[mi][1], rsa[mi], rsb[mi]);
                        continue;
                    }
                    // (the window of this thread's row: rows past the batch repeat the last window, as srow does)
                    const double* sp2 = ser.stats + ((size_t)min(w0 + (mi * BPP + sub) * P::ROWS + r0, a.B - 1) * ser.n_runs + rfirst + s.j) * 2;
                    series_fetch_f32<true, false>(s, nvalid > 0, srow[mi], sp2, vn[mi][0], vn[mi][1], rsa[mi], rsb[mi]);
                }
                return;
            }
            const u32x4 ones = u32x4{0x3f803f80u, 0x3f803f80u, 0x3f803f80u, 0x3f803f80u};      // the constant-1 run (bf16 1.0)
#pragma unroll
            for (int mi = 0; mi < MB / BPP; ++mi) {
                unsigned long long pa = s.pa, pb = s.pb;
                if constexpr (ORBIT) {      // this window row's own run pointers and signs
                    const SeriesSplit se = series_split<SIGN>(k0, nvalid, ser.T, [&](int jj) -> unsigned long long { return run_ptr_of(erow[mi], jj); });
                    pa = se.pa; pb = se.pb; neg_a[mi] = se.st.neg_a; neg_b[mi] = se.st.neg_b;
                }
                u32x4 va = nvalid > 0 ? ones : u32x4{0, 0, 0, 0};
                if (pa) va = *reinterpret_cast<const u32x4*>(reinterpret_cast<const T*>(pa) + srow[mi] + s.off);       // 2-byte aligned: served at full rate
                if (s.second) {
                    u32x4 vb2 = ones;
                    if (pb) vb2 = *reinterpret_cast<const u32x4*>(reinterpret_cast<const T*>(pb) + srow[mi]);
                    va = splice8(va, vb2, s.st.n0);
                }
                v[mi][0] = va;
            }
            return;
        }
        if constexpr (SRC > 0) {
#pragma unroll
            for (int mi = 0; mi < MB / BPP; ++mi) {
                const int w = w0 + (mi * BPP + sub) * P::ROWS + r0;
                const char* row = reinterpret_cast<const char*>(wsrc.p[t]) + ((size_t)min(w, a.B - 1) * nt + node) * spitch * SRC;
                wide_fetch<SRC>(wv8[mi], row, k0, F, unit_ok, w < a.B);
            }
            return;
        }
#pragma unroll
        for (int mi = 0; mi < MB / BPP; ++mi)
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                const int m = mi * BPP + sub, row = r0 + it * (256 / P::CPR), w = w0 + m * P::ROWS + row;
                if constexpr (ALIGNED) {
                    // unconditional raw 16-byte load (nothing uses it here): rows past the batch re-read the last row, chunks past the
                    // row's end re-read the K chunk's first one -- the staging pass zeroes both
                    const T* src = x + ((size_t)min(w, a.B - 1) * nt + node) * pitch + (nvalid > 0 ? k0 : kc * H);
                    v[mi][it] = ld16<ENC_NT>(src);
                } else {
                    v[mi][it] = u32x4{0, 0, 0, 0};
                    if (w < a.B) v[mi][it] = load_chunk<T>(x + ((size_t)w * nt + node) * pitch + k0, nvalid, r.vb);
                }
            }
    };
    // (two K chunks in flight per thread were measured: no gain, ENC_DEEP of round 2; the plain loop keeps the kernel at 82 VGPRs = five workgroups per CU)
    fetch(0);
    for (int kc = 0; kc < nkc; ++kc) {
        const u32x4 sx = sign_xor<T>(r.sg + kc * H + c * P::EPC);   // apply_symmetry: +-1 mask as a sign-bit XOR
        const int nv = F - (kc * H + c * P::EPC);                  // valid elements of this thread's chunk (pad columns dropped)
        u32x4 gm = u32x4{0, 0, 0, 0}, gm0 = gm, gm1 = gm;          // SIGN: the chunk's per-element sign masks (bf16 elements; NORM: the fp32 elements it standardises)
        if constexpr (SIGN && NORM && !ORBIT) sign_mask8_f32(cs.n0, cs.neg_a, cs.neg_b, gm0, gm1);
        else if constexpr (SIGN && !ORBIT) gm = sign_mask8_bf16(cs.n0, cs.neg_a, cs.neg_b);
        __syncthreads();   // previous chunk's MFMAs are done reading LDS
#pragma unroll
        for (int mi = 0; mi < MB / BPP; ++mi)
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                if constexpr (ORBIT && NORM) sign_mask8_f32(cs.n0, neg_a[mi], neg_b[mi], gm0, gm1);      // (per window row)
                else if constexpr (ORBIT) gm = sign_mask8_bf16(cs.n0, neg_a[mi], neg_b[mi]);
                u32x4 raw;
                if constexpr (SRC > 0) {      // fp64 / fp32 -> (fp32 ->) bf16, round to nearest even twice as torch's .to(bfloat16) does; elements past the row: zero
                    f32x4 lo4, hi4;
                    wide_to_f32<SRC>(wv8[mi], nv, lo4, hi4);
                    raw = pack_oct(lo4, hi4);
                } else if constexpr (NORM) {
                    u32x4 a0 = vn[mi][0], a1 = vn[mi][1];
                    if constexpr (SIGN) { a0 ^= gm0; a1 ^= gm1; }
                    standardise_oct(a0, a1, cs.n0, cs.has_a, cs.has_b, rsa[mi], rsb[mi]);
                    raw = pack_oct(__builtin_bit_cast(f32x4, a0), __builtin_bit_cast(f32x4, a1));
                    if (kc + 1 == nkc) raw = chunk_keep_first<T>(raw, nv);
                } else if constexpr (SIGN)
                raw = kc + 1 == nkc ? chunk_keep_first<T>(v[mi][it] ^ gm, nv) : v[mi][it] ^ gm;
                else
                raw = kc + 1 == nkc ? chunk_keep_first<T>(v[mi][it], nv) : v[mi][it];      // only the last K chunk has pad columns
                *reinterpret_cast<u32x4*>(smem + lds_chunk<T>(mi * BPP + sub, r0 + it * (256 / P::CPR), c)) = raw ^ sx;
                if constexpr (SERIES || SRC > 0) rawv[mi][it] = raw;
            }
        __syncthreads();
        if (!skip) load_bfrag<T>(bf, wpack, a.pack0[t] + kc, wv, lane);   // before the prefetch: vmcnt retires in order
        if (kc + 1 < nkc) fetch(kc + 1);   // the next K chunk streams from HBM under this chunk's MFMAs
        if constexpr (SERIES || SRC > 0) {
            // the materialised window rows of THIS chunk (raw values: the sign mask is applied by whoever reads them) go out BEHIND the next chunk's
            // loads: vmcnt retires in issue order, so a load issued after stores can only be waited for together with them -- with the stores
            // youngest, the next chunk's wait leaves them in flight
#pragma unroll
            for (int mi = 0; mi < MB / BPP; ++mi)
#pragma unroll
                for (int it = 0; it < NIT; ++it) {
                    const int w = w0 + (mi * BPP + sub) * P::ROWS + r0 + it * (256 / P::CPR), k0 = kc * H + c * P::EPC;
                    if (x != nullptr && w < a.B && k0 < (int)pitch) *reinterpret_cast<u32x4*>(const_cast<T*>(x) + ((size_t)w * nt + node) * pitch + k0) = rawv[mi][it];
                }
        }
        if (!skip) {
#pragma unroll
            for (int m = 0; m < MB; ++m) {
                if (w0 + m * P::ROWS < a.B) {   // uniform
                    load_afrag<T>(af, smem, m, ao);
                    mac(acc[m], af, bf);
                }
            }
        }
    }
    if (skip) return;
    T* x0 = reinterpret_cast<T*>(a.x0);
    const int gnode = a.tbase[t] + node;
#pragma unroll
    for (int m = 0; m < MB; ++m) {
        const int w = w0 + m * P::ROWS + c_win(lane);
        enc_relu_bits<T>(a, acc[m], gnode, w0 + m * P::ROWS, wv, lane);
        if (w < a.B) store_oct(x0 + act_idx(w, gnode, a.B) + wv * 32 + c_oct(lane), acc[m].c[0], acc[m].c[1]);
    }
}

// ---- k_enc_x3: the split plan, from fp32 inputs; one workgroup = 64 windows of ONE node, LDS hi blocks [0, 4), lo blocks [4, 8) ----
template <bool ALIGNED, bool SERIES = false, int SRC = 0, bool NORM = false, bool SIGN = false, bool ORBIT = false> __global__ __launch_bounds__(256) void k_enc_x3(EncArgs a, int n_img, SeriesSrc ser, WideSrc wsrc) {
    static_assert(!ORBIT || SIGN, "a group element per window: part of the signed series gather");
    static_assert(!NORM || SERIES, "standardisation is part of the series gather");
    static_assert(!SIGN || SERIES, "signs are part of the series gather");
    static_assert(!SERIES || ALIGNED, "the series gather writes aligned window buffers");
    static_assert(SRC == 0 || (ALIGNED && !SERIES), "wide source rows: aligned destination rows, no series gather");
    using P = P16;
    constexpr int MB = 4;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    EncRole r;
    const EncWg role = enc_role<SERIES, ORBIT>(a, ser, tid, r);
    if (role != ENC_WG_ENCODE) {
        if constexpr (ALIGNED && !SERIES) if (role == ENC_WG_PREP) prep_one<__bf16, true>(a.prep, r.prep_wg * 256 + tid, false);
        return;
    }
    const int t = r.t, node = r.node, F = r.F, nt = r.nt, nkc = r.nkc;
    const bool skip = r.skip;
    const int64_t pitch = r.pitch;
    const int w0 = r.tile * MB * P::ROWS;
    const float* x = reinterpret_cast<const float*>(a.x[t]);
    const T16* wpack = reinterpret_cast<const T16*>(a.wpack);

    P::Acc acc[MB];
#pragma unroll
    for (int m = 0; m < MB; ++m) acc_init_bias<T16>(acc[m], r.bias, wv, lane);
    const int c = tid & 15, r0 = tid >> 4;      // staging: thread = (row, 8-element chunk) of each of the MB row blocks
    P::BFrag bfh, bfl;
    P::AFrag af;
    const AOff<T16> ao(lane);
    u32x4 v[MB][2];                             // the 8 fp32 elements of the chunk (two 16-byte loads)
    u32x2 wv8[SRC ? MB : 1][SRC ? SRC : 1];     // SRC: the chunk's 8 source elements as 8-byte units, untouched until the staging pass
    const bool unit_ok = SRC == 8 || (F & 1) == 0;
    const int64_t spitch = SRC ? wsrc.pitch[t] : 0;
    int srow[SERIES ? MB : 1]; int rfirst = 0;  // SERIES: first series row of this thread's window rows, the node row's first run
    RunStats rsa[NORM ? MB : 1], rsb[NORM ? MB : 1];      // NORM: the statistics of the chunk's two runs per window
    ChunkState cs;
    int erun[ORBIT ? MB : 1];      // ORBIT: this thread's window rows' offsets into the run-pointer table (element x n_runs)
    bool neg_a[ORBIT ? MB : 1], neg_b[ORBIT ? MB : 1];      // ORBIT: the signs of the chunk in flight per window row (cs.neg_a / neg_b otherwise)
    if constexpr (SERIES) {
#pragma unroll
        for (int m = 0; m < MB; ++m) {
            const int64_t sw = ser.starts[min(w0 + m * P::ROWS + r0, a.B - 1)];
            srow[m] = (int)(ORBIT ? start_row(sw) : sw);
            if constexpr (ORBIT) erun[m] = start_element(sw, orbit_elements(ser.sign)) * ser.n_runs;
        }
        rfirst = ser.rows[2 * (ser.row0[t] + node)];
    }
    auto fetch = [&](int kc) {
        const int k0 = kc * H + c * 8;
        const int nv = F - k0;
        if constexpr (SERIES) {
            // (ORBIT: element 0's split gives the chunk's geometry and which runs have a source column -- the row structure every element shares)
            const SeriesSplit s = series_split<SIGN>(k0, min(nv, 8), ser.T, [&](int jj) -> unsigned long long { return ser.run_ptr[rfirst + jj]; });
            cs = s.st;
#pragma unroll
            for (int m = 0; m < MB; ++m) {
                // (rows past the batch repeat the last window, as srow does)
                const double* sp2 = NORM ? ser.stats + ((size_t)min(w0 + m * P::ROWS + r0, a.B - 1) * ser.n_runs + rfirst + s.j) * 2 : nullptr;
                if constexpr (ORBIT) {      // this window row's own run pointers and signs
                    const SeriesSplit se = series_split<SIGN>(k0, min(nv, 8), ser.T, [&](int jj) -> unsigned long long { return ser.run_ptr[erun[m] + rfirst + jj]; });
                    neg_a[m] = se.st.neg_a; neg_b[m] = se.st.neg_b;
                    series_fetch_f32<NORM, true>(se, nv > 0, srow[m], sp2, v[m][0], v[m][1], rsa[NORM ? m : 0], rsb[NORM ? m : 0]);
                } else
                series_fetch_f32<NORM, true>(s, nv > 0, srow[m], sp2, v[m][0], v[m][1], rsa[NORM ? m : 0], rsb[NORM ? m : 0]);
            }
            return;
        }
        if constexpr (SRC > 0) {
#pragma unroll
            for (int m = 0; m < MB; ++m) {
                const int w = w0 + m * P::ROWS + r0;
                const char* row = reinterpret_cast<const char*>(wsrc.p[t]) + ((size_t)min(w, a.B - 1) * nt + node) * spitch * SRC;
                wide_fetch<SRC>(wv8[m], row, k0, F, unit_ok, w < a.B);
            }
            return;
        }
#pragma unroll
        for (int m = 0; m < MB; ++m) {
            const int w = w0 + m * P::ROWS + r0;
            if constexpr (ALIGNED) {
                // unconditional raw loads (nothing uses them here): rows past the batch re-read the last row, halves past the row's end
                // re-read the K chunk's first elements -- the staging pass zeroes the latter, the former are never stored
                const float* src = x + ((size_t)min(w, a.B - 1) * nt + node) * pitch;
                v[m][0] = ld16<ENC_NT>(src + (nv > 0 ? k0 : kc * H));
                v[m][1] = ld16<ENC_NT>(src + (nv > 4 ? k0 + 4 : kc * H));
            } else {
                v[m][0] = u32x4{0, 0, 0, 0}; v[m][1] = u32x4{0, 0, 0, 0};
                if (w < a.B) {
                    const float* src = x + ((size_t)w * nt + node) * pitch + k0;
                    v[m][0] = load_chunk<float>(src, nv, r.vb);
                    v[m][1] = load_chunk<float>(src + 4, nv - 4, r.vb);
                }
            }
        }
    };
    fetch(0);
    for (int kc = 0; kc < nkc; ++kc) {
        const u32x4 sxa = sign_xor<float>(r.sg + kc * H + c * 8), sxb = sign_xor<float>(r.sg + kc * H + c * 8 + 4);   // apply_symmetry: +-1 mask as a sign-bit XOR
        const int nv = F - (kc * H + c * 8);
        u32x4 gm0 = u32x4{0, 0, 0, 0}, gm1 = gm0;      // SIGN: the chunk's per-element sign masks
        if constexpr (SIGN && !ORBIT) sign_mask8_f32(cs.n0, cs.neg_a, cs.neg_b, gm0, gm1);
        __syncthreads();   // previous chunk's MFMAs are done reading LDS
#pragma unroll
        for (int m = 0; m < MB; ++m) {
            if constexpr (ORBIT) sign_mask8_f32(cs.n0, neg_a[m], neg_b[m], gm0, gm1);      // (per window row)
            u32x4 fa = v[m][0], fb = v[m][1];
            if constexpr (SRC > 0) {      // fp64 -> fp32 (round to nearest even, as torch's .float()), or the fp32 units as they are; elements past the row: zero
                f32x4 lo4, hi4;
                wide_to_f32<SRC>(wv8[m], nv, lo4, hi4);
                fa = __builtin_bit_cast(u32x4, lo4); fb = __builtin_bit_cast(u32x4, hi4);
            } else
            {
                if constexpr (SIGN) { fa ^= gm0; fb ^= gm1; }
                if constexpr (NORM) standardise_oct(fa, fb, cs.n0, cs.has_a, cs.has_b, rsa[m], rsb[m]);
                if (kc + 1 == nkc) { fa = chunk_keep_first<float>(fa, nv); fb = chunk_keep_first<float>(fb, nv - 4); }     // only the last K chunk has pad columns
            }
            if constexpr (SERIES || SRC > 0) {      // the materialised window row (raw values: the sign mask is applied by whoever reads it)
                const int w = w0 + m * P::ROWS + r0, k0 = kc * H + c * 8;
                if (x != nullptr && w < a.B) {
                    float* dst = const_cast<float*>(x) + ((size_t)w * nt + node) * pitch + k0;
                    if (k0 < (int)pitch) *reinterpret_cast<u32x4*>(dst) = fa;
                    if (k0 + 4 < (int)pitch) *reinterpret_cast<u32x4*>(dst + 4) = fb;
                }
            }
            fa ^= sxa; fb ^= sxb;
            u32x4 hi, lo;
            split_oct(__builtin_bit_cast(f32x4, fa), __builtin_bit_cast(f32x4, fb), hi, lo);
            *reinterpret_cast<u32x4*>(smem + lds_chunk<T16>(m, r0, c)) = hi;
            *reinterpret_cast<u32x4*>(smem + lds_chunk<T16>(MB + m, r0, c)) = lo;
        }
        __syncthreads();
        if (!skip) {
            load_bfrag<T16>(bfh, wpack, a.pack0[t] + kc, wv, lane);              // before the prefetch: vmcnt retires in order
            load_bfrag<T16>(bfl, wpack, n_img + a.pack0[t] + kc, wv, lane);
        }
        if (kc + 1 < nkc) fetch(kc + 1);   // the next K chunk streams from HBM under this chunk's MFMAs
        if (!skip) {
#pragma unroll
            for (int m = 0; m < MB; ++m) {
                if (w0 + m * P::ROWS < a.B) {   // uniform
                    load_afrag<T16>(af, smem, m, ao);
                    mac(acc[m], af, bfh);
                    mac(acc[m], af, bfl);
                    load_afrag<T16>(af, smem, MB + m, ao);
                    mac(acc[m], af, bfh);
                }
            }
        }
    }
    if (skip) return;
    T16* x0 = reinterpret_cast<T16*>(a.x0);
    const int gnode = a.tbase[t] + node;
#pragma unroll
    for (int m = 0; m < MB; ++m) {
        const int w = w0 + m * P::ROWS + c_win(lane);
        enc_relu_bits<T16>(a, acc[m], gnode, w0 + m * P::ROWS, wv, lane);
        if (w < a.B) {
            u32x4 hi, lo;
            split_oct(acc[m].c[0], acc[m].c[1], hi, lo);
            T16* q = x0 + x3_idx(w, gnode, a.B) + wv * 32 + c_oct(lane);
            *reinterpret_cast<u32x4*>(q) = hi;
            *reinterpret_cast<u32x4*>(q + H) = lo;
        }
    }
}
