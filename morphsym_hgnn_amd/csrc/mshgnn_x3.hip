// Split-bf16 parity plan (MSHGNN_BF16X3) of the MS-HGNN engine: the same path as the bf16 plan of mshgnn.hip
// (GRF_HGNN_C2.forward hgnn_c2.py:133-182 and its autograd backward, lowered as DESIGN.md section 2 describes) at the
// north_star's tolerance (1e-4 relative) on the bf16 matrix cores.
//
// Every fp32 quantity x that feeds a product -- inputs, weights, activations, activation gradients -- travels as two bf16
// values, hi = bf16(x) and lo = bf16(x - hi): x = hi + lo to 16 mantissa bits.  A product is taken as
//     x w  =  x_hi w_hi + x_lo w_hi + x_hi w_lo          (the lo x lo term is 2^-18 relative: below fp32 resolution)
// with fp32 accumulation, i.e. three bf16 MFMAs per term instead of one fp32 MFMA at 1/16 of the rate.  Layout:
//   * inputs x[t]: fp32 in HBM (as the MSHGNN_F32 plan takes them); split in registers while they are staged;
//   * every activation tensor in the workspace: rows of 256 bf16, [hi 128 | lo 128] ([NN][B][2][128]): a window's hi and lo halves are
//     one contiguous 512-byte piece for every stream (stash writes, tile loads, the weight-gradient kernel's operand rows);
//   * LDS tile of the stack kernels: block n = hi plane of node n, block lo_blk + n = its lo plane (A1-C2: 40 blocks = 160 KB,
//     one 8-wave workgroup per CU); k_prep writes a hi and a lo image of every weight pack;
//   * the MAC loop of the stack kernels is the bf16 plan's: the plan compiler (split_segs, mshgnn_plan.hpp) turns each
//     segment into two -- the hi image with the hi and lo block of every source, the lo image with the hi block.
#include "mshgnn_x3_stack.hpp"
#include "mshgnn_enc.hpp"
#include "mshgnn_launch.hpp"

// (k_prep<__bf16, true> / k_prep_tiled<__bf16, true>, the hi and lo MFMA B-fragment images of every weight pack + bias sums: mshgnn_device.hpp)
// (k_enc_x3, the encoder of this plan: defined in mshgnn_enc.hpp, beside k_enc_fwd of the fp32 / bf16 plans)

// ------------------------------------------------------------------------------------------------------
// The stack kernels (mshgnn_x3_stack.hpp) over the plan's run-time tables; those over the compile-time programs are mshgnn_x3_spec_shard.hip's
// ------------------------------------------------------------------------------------------------------
template <bool ALIAS> __global__ __launch_bounds__(LAYER_THREADS, 2) void k_stack_fwd_x3(StackArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    stack_fwd_x3_body<ALIAS, false>(a, smem);
}

__global__ __launch_bounds__(LAYER_THREADS, 2) void k_stack_bwd_x3(StackArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    stack_bwd_x3_body<false>(a, smem);
}

// row `form` (pick::SpecFormX3) of the launch table of the program whose tables are the plan's (a shard's, or the program attached after the build); name: the program's
using SpecSelectorX3 = StackKernelX3 (*)(const HostPlan& hp, int form, const char** name);
static StackKernelX3 x3_spec_kernel(const HostPlan& hp, int form, const char** name = nullptr) {
    if (hp.jit_prog) if (StackKernelX3 kk = reinterpret_cast<SpecSelectorX3>(hp.jit_prog)(hp, form, name)) return kk;      // a program compiled for this plan after the build
#define X3_SHARD_TRY(k) if (StackKernelX3 kk = x3_spec_shard##k(hp, form, name)) return kk;
    SPEC_SHARD_LIST(X3_SHARD_TRY)
#undef X3_SHARD_TRY
    return nullptr;
}


// (k_dec_bwd<T16, true>, the decoder backward on the hi/lo planes of X_L -> dX_L planes: mshgnn_device.hpp; used by mshgnn_backward / _mse / _ce -- mshgnn_step_mse takes
// the fused tail of k_stack_fwd_x3)

// ------------------------------------------------------------------------------------------------------
// weight gradients: all of the step as one split-K MFMA launch, dW[o][k] = sum_w P[w][o] Q[w][k] with P = P_hi + P_lo, Q = Q_hi + Q_lo: four staged tiles
// per 32-window step (32 KB of tiles and three workgroups per CU; 64-window steps at two per CU: 339 vs 301 us), P_hi Q_hi + P_hi Q_lo + P_lo Q_hi on the
// 32x32x16 bf16 MFMA.  Workgroup = (lane = its items, window part); raw encoder inputs (fp32) are split while they are staged.
// ------------------------------------------------------------------------------------------------------
#ifndef GWX3_WPS
#define GWX3_WPS 3
#endif

// k_gradw_x3_lean: the same 32-window step loop with the addressing of k_gradw_bf16_lean (mshgnn.hip): a thread owns TWO CONSECUTIVE windows of
// one 16-byte column chunk, so every global address is  workgroup-uniform stream pointer (scalar registers, advanced by scalar adds)  +  ONE
// per-thread 32-bit offset  +  an immediate (the [hi | lo] row layout puts the four loads of an operand at +0 / +256 / +512 / +768), the relu
// bytes of its two rows are one aligned 16-bit load, and full chunks carry no bound checks.  (Its predecessor of round 2 kept six 64-bit
// per-thread pointers alive and spilled three of them: 28 B of scratch per lane, reloaded inside the step loop in front of the loads that
// needed them.)  A lane's items (all of one target) are swept one after the other over the lane's window part into the same accumulators (any
// number of items per lane: the plan picks the items-per-lane x window-parts split that fills the chip best).  ALIGNED: raw inputs in the
// engine's own 16-byte-aligned layout; the other instantiation reads them element-wise.
template <bool ALIGNED> __global__ __launch_bounds__(256, GWX3_WPS) void k_gradw_x3_lean(GradwArgs a) {
    using T = T16;
    constexpr int KW = 32;
    __shared__ __attribute__((aligned(16))) __bf16 Ph[KW * GWB_PITCH];
    __shared__ __attribute__((aligned(16))) __bf16 Pl[KW * GWB_PITCH];
    __shared__ __attribute__((aligned(16))) __bf16 Qh[KW * GWB_PITCH];
    __shared__ __attribute__((aligned(16))) __bf16 Ql[KW * GWB_PITCH];
    __shared__ __attribute__((aligned(16))) u32x4 mlut[256];       // relu byte -> AND mask of 8 bf16
    __shared__ __attribute__((aligned(16))) u32x4 qfix[16][2];            // raw-input items: per column chunk c the keep masks of its two fp32 halves
    __shared__ __attribute__((aligned(16))) u32x4 qsign_t[GW_IPL][16][2]; // ... and per (item, column chunk) the symmetry sign XORs
    __shared__ unsigned long long sbase[GW_IPL][4];                       // per item: stream bases of P, relu bytes, Q at the part's first window
    // extra workgroups carry the finalize ops that read no slab (GwSide; as in k_gradw_bf16_lean, mshgnn.hip)
    const int sw = (int)blockIdx.x - a.side.wg0;
    if (sw >= 0 && sw < a.side.n_grid) { if (sw < a.side.n) gw_side_workgroup(a.side, sw); return; }
    const int bx = (int)blockIdx.x - a.side.main0;
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    mlut[tid] = chunk_mask_bits<__bf16>(u32x4{0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu}, (unsigned)tid);   // (visible after the first barrier)
    const int wr = wv >> 1, wc = wv & 1;
    const int ln = a.lane_order[bx % a.n_pad], part = bx / a.n_pad;
    if (ln < 0) return;
    const int* lh = a.lanes + ln * LANE_INTS;
    const int it0 = lh[0], nit = lh[1] - lh[0], bias_flag = lh[3];
    const int* im0 = a.items + it0 * ITEM_INTS;
    const int nchunks = (a.B + KW - 1) / KW;
    const int ch0 = (int)((int64_t)part * nchunks / a.n_parts), ch1 = (int)((int64_t)(part + 1) * nchunks / a.n_parts);
    const int nsteps = ch1 - ch0, total = nsteps * nit;      // the lane's items interleaved chunk by chunk (every workgroup sweeps the batch at the same pace), into the same accumulators
    const int c = tid & 15, r2 = (tid >> 4) * 2;      // rows r2, r2 + 1 of the 32-window step, columns [8c, 8c + 8)
    constexpr int ROWB = 2 * H * (int)sizeof(T);      // bytes of one [hi | lo] row

    // what every item of the lane shares (one target): operand kinds, the input type and column chunk of a raw Q
    const bool p_masked = im0[9] >= 0, q_act = im0[4] >= 0;
    const int ntile = (a.B + 15) >> 4;
    const unsigned voffP = (unsigned)(r2 * ROWB + c * 16);
    const unsigned voffM = (unsigned)(((c >> 2) * ntile + (r2 >> 4)) * 64 + (c & 3) * 16 + (r2 & 15));
    const int qt = q_act ? 0 : im0[3] - BUF_IN;
    const unsigned qsb = q_act ? (unsigned)ROWB : (unsigned)(a.nodes[qt] * a.pitch[qt]) * 4u;
    const int qn = q_act ? 8 : im0[7] - c * 8, qvb = q_act ? 16 : a.vb[qt];
    if (!q_act && tid < 16) {      // (these constants would cost 16 VGPRs per lane: over the budget of three workgroups per CU)
        const u32x4 ones = u32x4{0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
        qfix[tid][0] = chunk_keep_first<float>(ones, qn); qfix[tid][1] = chunk_keep_first<float>(ones, qn - 4);
    }
    // raw rows: two 16-byte halves of 8 floats; halves past the row's end re-read the chunk's first bytes (never used: the keep masks are 0)
    const unsigned voffQ0 = q_act ? voffP : (unsigned)r2 * qsb + (qn > 0 ? (unsigned)c * 32u : 0u);
    const unsigned qhalf = q_act ? 256u : (qn > 4 ? 16u : 0u);
    if (tid < nit) {     // thread k resolves item k's stream bases (at the part's first window)
        const int* im = a.items + (it0 + tid) * ITEM_INTS;
        sbase[tid][0] = (unsigned long long)(a.ws + a.buf_off[im[0]] + (x3_idx(0, im[2], a.B) + (size_t)ch0 * KW * 2 * H) * sizeof(T));
        sbase[tid][1] = p_masked ? (unsigned long long)(a.ws + a.buf_off[im[9]] + relu_byte(im[2], a.B, 0, 0) + (size_t)ch0 * (KW / 16) * 64) : 0ull;
        sbase[tid][2] = q_act ? (unsigned long long)(a.ws + a.buf_off[im[3]] + (x3_idx(0, im[5], a.B) + (size_t)ch0 * KW * 2 * H) * sizeof(T))
                              : (unsigned long long)(reinterpret_cast<const char*>(a.x[qt]) + ((size_t)im[5] * a.pitch[qt] + im[6]) * 4 + (size_t)ch0 * KW * qsb);
    }
    if (!q_act && tid < nit * 16) {
        const int* im = a.items + (it0 + (tid >> 4)) * ITEM_INTS;
        qsign_t[tid >> 4][c][0] = sign_xor<float>(a.signs + im[8] + c * 8); qsign_t[tid >> 4][c][1] = sign_xor<float>(a.signs + im[8] + c * 8 + 4);
    }
    __syncthreads();
    const char* pS = a.ws; const char* mS = a.ws; const char* qS = a.ws;
    auto ubase = [&](int k, int j, size_t off) -> const char* {      // workgroup-uniform 64-bit pointer out of the LDS table
        const unsigned long long v = sbase[k][j] + off;
        return reinterpret_cast<const char*>(((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32) |
                                             (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v));
    };
    unsigned ldsw[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) ldsw[p] = (unsigned)gwb_elem(r2 + p, c * 8);
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[i][j][q] = 0.f;
    float bsum[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) bsum[e] = 0.f;

    u32x4 ph[2], pl[2], qa[2], qb[2]; unsigned mw = 0xffffu;
    auto load_qa = [&](int p) -> u32x4 {
        if constexpr (ALIGNED) return *reinterpret_cast<const u32x4*>(qS + voffQ0 + p * qsb);
        else return q_act ? *reinterpret_cast<const u32x4*>(qS + voffQ0 + p * qsb) : load_chunk<float>(reinterpret_cast<const float*>(qS + (unsigned)(r2 + p) * qsb + (unsigned)c * 32u), qn, qvb);
    };
    auto load_qb = [&](int p) -> u32x4 {
        if constexpr (ALIGNED) return *reinterpret_cast<const u32x4*>(qS + voffQ0 + p * qsb + qhalf);
        else return q_act ? *reinterpret_cast<const u32x4*>(qS + voffQ0 + p * qsb + qhalf) : load_chunk<float>(reinterpret_cast<const float*>(qS + (unsigned)(r2 + p) * qsb + (unsigned)c * 32u) + 4, qn - 4, qvb);
    };
    int nk = 0, nc = 0;            // (item, chunk of the part) of the next fetch: items interleaved chunk by chunk
    auto fetch = [&]() {
        pS = ubase(nk, 0, (size_t)nc * KW * ROWB);
        if (p_masked) mS = ubase(nk, 1, (size_t)nc * (KW / 16) * 64);
        qS = ubase(nk, 2, (size_t)nc * KW * qsb);
        const int w0 = (ch0 + nc) * KW;
        if (w0 + KW <= a.B) {
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                ph[p] = *reinterpret_cast<const u32x4*>(pS + voffP + p * ROWB);
                pl[p] = *reinterpret_cast<const u32x4*>(pS + voffP + p * ROWB + 256);
                qa[p] = load_qa(p);
                qb[p] = load_qb(p);
            }
            if (p_masked) mw = *reinterpret_cast<const unsigned short*>(mS + voffM);
        } else {                   // last chunk of the batch: rows beyond B are zero
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                ph[p] = u32x4{0, 0, 0, 0}; pl[p] = u32x4{0, 0, 0, 0}; qa[p] = u32x4{0, 0, 0, 0}; qb[p] = u32x4{0, 0, 0, 0};
                if (w0 + r2 + p < a.B) {
                    ph[p] = *reinterpret_cast<const u32x4*>(pS + voffP + p * ROWB);
                    pl[p] = *reinterpret_cast<const u32x4*>(pS + voffP + p * ROWB + 256);
                    qa[p] = load_qa(p);
                    qb[p] = load_qb(p);
                }
            }
            mw = 0xffffu;
            if (p_masked && w0 + r2 < a.B) mw = *reinterpret_cast<const unsigned short*>(mS + voffM);     // (the 16-window tile of row r2 exists)
        }
        if (++nk == nit) { nk = 0; ++nc; }
    };
    int sk = 0;                    // item of the step being staged
    auto stage_to_lds = [&]() {
        const int ks = sk;
        if (++sk == nit) sk = 0;
        u32x4 mk[2];
        if (p_masked) {
#pragma unroll
            for (int p = 0; p < 2; ++p) mk[p] = mlut[(mw >> (8 * p)) & 0xffu];
        }
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            u32x4 h = ph[p], l = pl[p];
            if (p_masked) { h &= mk[p]; l &= mk[p]; }                   // dH = dX . relu bits
            *reinterpret_cast<u32x4*>(&Ph[ldsw[p]]) = h;
            *reinterpret_cast<u32x4*>(&Pl[ldsw[p]]) = l;
            u32x4 qh = qa[p], ql = qb[p];
            if (!q_act) {      // drop pad columns, symmetry sign mask, fp32 -> hi / lo
                const u32x4 fa = (qa[p] & qfix[c][0]) ^ qsign_t[ks][c][0], fb = (qb[p] & qfix[c][1]) ^ qsign_t[ks][c][1];
                split_oct(__builtin_bit_cast(f32x4, fa), __builtin_bit_cast(f32x4, fb), qh, ql);
            }
            *reinterpret_cast<u32x4*>(&Qh[ldsw[p]]) = qh;
            *reinterpret_cast<u32x4*>(&Ql[ldsw[p]]) = ql;
            if (bias_flag) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    bsum[2 * e] += __builtin_bit_cast(float, h[e] << 16) + __builtin_bit_cast(float, l[e] << 16);
                    bsum[2 * e + 1] += __builtin_bit_cast(float, h[e] & 0xffff0000u) + __builtin_bit_cast(float, l[e] & 0xffff0000u);
                }
            }
        }
    };
    if (total > 0) fetch();
    for (int s = 0; s < total; ++s) {
        __syncthreads();      // the previous MFMA phase of every wave is done reading the tiles
        stage_to_lds();
        __syncthreads();
        if (s + 1 < total) fetch();
#pragma unroll
        for (int ks = 0; ks < KW / 16; ++ks) {
            bf16x8 afh[2], afl[2], bqh[2], bql[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                afh[i] = tr_frag(Ph, ks * 16, wr * 64 + i * 32, lane);
                afl[i] = tr_frag(Pl, ks * 16, wr * 64 + i * 32, lane);
                bqh[i] = tr_frag(Qh, ks * 16, wc * 64 + i * 32, lane);
                bql[i] = tr_frag(Ql, ks * 16, wc * 64 + i * 32, lane);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(afh[i], bqh[j], acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(afh[i], bql[j], acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(afl[i], bqh[j], acc[i][j], 0, 0, 0);
                }
        }
    }
    float* slab = a.slabs + (size_t)(part * a.n_lanes + ln) * SLAB_FLOATS;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int o = wr * 64 + i * 32 + (q & 3) + ((q >> 2) << 3) + ((lane >> 5) << 2), k = wc * 64 + j * 32 + (lane & 31);
                slab[o * H + k] = acc[i][j][q];
            }
    if (bias_flag) {
        float* red = reinterpret_cast<float*>(Ph);   // 16 x 128 floats = 8 KB <= one tile
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 8; ++e) red[(tid >> 4) * H + c * 8 + e] = bsum[e];
        __syncthreads();
        if (tid < H) {
            float s2 = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) s2 += red[r * H + tid];
            slab[H * H + tid] = s2;
        }
    }
}

// ------------------------------------------------------------------------------------------------------
// launch sequences: this plan's kernel selection and launches; the argument structs are filled by mshgnn_launch.hpp, as for the fp32 / bf16 plans (mshgnn.hip)
// ------------------------------------------------------------------------------------------------------
void x3_launch_prep(const PrepArgs& a, bool biases, hipStream_t st) {
    if (prep_use_tiled(a.n_packs)) hipLaunchKernelGGL((k_prep_tiled<__bf16, true>), dim3(prep_tiled_grid(a.n_packs, a.n_biases)), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((k_prep<__bf16, true>), dim3(prep_grid(a, 8, biases)), dim3(256), 0, st, a);
}

// launch tables: row k is what pick_stack / pick_enc (mshgnn_pick.hpp) call k on this plan
static constexpr StackKernelX3 X3_TABLE[pick::X3_ROWS] = {k_stack_fwd_x3<false>, k_stack_fwd_x3<true>, k_stack_bwd_x3, k_stack_step_x3<false>, k_stack_step_x3<true>};
using EncKernelX3 = void (*)(EncArgs, int, SeriesSrc, WideSrc);
static constexpr EncKernelX3 ENC_X3_TABLE[pick::ENC_FORMS] = {      // by pick::EncForm
    k_enc_x3<false>, k_enc_x3<true>, k_enc_x3<true, false, 4>, k_enc_x3<true, false, 8>,
    k_enc_x3<true, true>, k_enc_x3<true, true, 0, true>, k_enc_x3<true, true, 0, false, true>, k_enc_x3<true, true, 0, true, true>,
    k_enc_x3<true, true, 0, false, true, true>, k_enc_x3<true, true, 0, true, true, true>};
static_assert(pick::STACK8_THREADS == LAYER_THREADS, "the pick's block size of this plan's stack kernels");
template <typename K, size_t N> static int set_lds_attrs(const K (&table)[N], int bytes) {
    for (K k : table) if (int rc = set_lds_attr(k, bytes)) return rc;
    return MSHGNN_OK;
}
static StackKernelX3 x3_stack_kernel(const HostPlan& hp, const pick::StackPick& pk) {
    return pk.family == pick::X3 ? X3_TABLE[pk.k] : pk.family == pick::X3_SPEC ? x3_spec_kernel(hp, pk.k) : nullptr;
}

static int x3_lds_stack(const HostPlan& hp) { return 2 * hp.fs_blk * P16::BLK; }

// the kernels over this plan's compile-time program, if it has one (built in, or attached): dynamic-LDS attribute, name; else use_spec = false
static int x3_set_spec_attrs(mshgnn_plan* p) {
    const char* nm = nullptr;
    for (int form = 0; form < pick::SPEC_FORMS_X3; ++form)
        if (StackKernelX3 k = x3_spec_kernel(p->hp, form, &nm)) { if (int rc = set_lds_attr(k, x3_lds_stack(p->hp))) return rc; } else break;      // (no program: no form)
    if (!nm) { p->use_spec = false; return MSHGNN_OK; }
    p->spec_name_buf = strncmp(nm, "spec::", 6) == 0 ? nm + 6 : nm;
    p->spec_name = p->spec_name_buf.c_str();
    return MSHGNN_OK;
}
// mshgnn_plan_attach_program on a split plan: `selector` is the mshgnn_jit_program_x3 of a program compiled for this plan
int x3_attach_program(mshgnn_plan* p, void* selector) {
    void* const prev = p->hp.jit_prog;
    p->hp.jit_prog = selector;
    const char* nm = nullptr;
    if (!reinterpret_cast<SpecSelectorX3>(selector)(p->hp, pick::SFX_STEP, &nm) || !nm) { p->hp.jit_prog = prev; return set_err(MSHGNN_EINVAL, "the program's tables are not this plan's"); }
    p->use_spec = true;
    const int rc = x3_set_spec_attrs(p);
    if (rc || !p->use_spec) { p->hp.jit_prog = prev; p->use_spec = false; return rc ? rc : set_err(MSHGNN_EINVAL, "no kernel of the attached program could be used"); }
    return MSHGNN_OK;
}
int x3_set_attrs(mshgnn_plan* p) {
    int rc;
    const int flds = x3_lds_stack(p->hp);
    { const char* esp = getenv("MSHGNN_SPEC"); p->use_spec = !(esp && atoi(esp) == 0); }
    if (p->use_spec && (rc = x3_set_spec_attrs(p))) return rc;
    if ((rc = set_lds_attrs(X3_TABLE, flds)) || (rc = set_lds_attrs(ENC_X3_TABLE, 8 * P16::BLK))) return rc;
    return MSHGNN_OK;
}

// what differs from the bf16 plan on the host side of a launch (mshgnn_launch.hpp): fp32 input rows, 64 windows per encoder workgroup, hi / lo weight images
static constexpr LaunchTraits X3_TRAITS{
    4, 4, 8, P16::BLK, 64, 8 * P16::BLK, 32,
    /*split*/ true, /*embed_prep*/ true, /*src_routes*/ true, /*wide_needs_rows*/ true, /*gradw_series*/ false,
    "the series gather writes 16-byte-aligned window buffers whose pitch is a multiple of 4",
    "wide source rows: the fp32 rows need 16-byte alignment and a pitch that is a multiple of 4"};

static void x3_stack_args(const mshgnn_plan* p, const StepCall& c, const mshgnn_ws_layout& lay, StackArgs& a) {
    const HostPlan& hp = p->hp;
    fill_stack_common(p, c, lay, a);
    a.lo_blk = hp.lo_blk; a.n_img = hp.n_img; a.scr0 = hp.x3_alias ? hp.NN - hp.n_mlp : hp.NN;
}

int x3_forward(const mshgnn_plan* p, StepCall& c) {
    const HostPlan& hp = p->hp;
    const LaunchTraits& tr = X3_TRAITS;
    mshgnn_ws_layout lay; layout_workspace(hp, c.batch, c.training, &lay);
    hipStream_t st = c.stream;
    int rc;
    {   // 1. hi / lo weight images (few packs: the layer packs under the encoder's tail, enc_prep_split), 2. encoder (fp32 inputs)
        EncArgs a{}; unsigned enc_grid = 0; int form = 0;
        if ((rc = prep_and_enc_args(p, c, lay, tr, x3_launch_prep, a, enc_grid))) return rc;
        ProfScope ps(p, hp.ks_enc, st);
        if ((rc = pick_enc_form(c, a, tr, enc_grid, form))) return rc;
        hipLaunchKernelGGL(ENC_X3_TABLE[form], dim3(enc_grid), dim3(256), tr.enc_lds, st, a, hp.n_img, enc_series_src(c, form), enc_wide_src(c, form));
    }
    {   // 3. all layers + decoder (+ loss and decoder backward with a fused loss)
        StackArgs a{};
        x3_stack_args(p, c, lay, a);
        fill_stack_tail(p, c, lay, a);
        a.tile_in = c.ws + lay.x[0]; a.training = c.training;
        a.stamps = stamp_ptr("MSHGNN_STAMPS");
        // (a one-call step: the backward sweep in the same launch, the tail's reduction scratch in the hi plane)
        const pick::StackPick pk = pick::pick_stack(stack_query(p, c, pick::PLAN_X3, forward_op(c), tr.blk, a));
        apply_stack_pick(hp, pk, lay, a);
        if (pk.what == pick::STEP) c.stack_done = true;
        ProfScope ps(p, pk.what == pick::STEP ? hp.ks_stack_step : hp.ks_stack_fwd, st);
        return launch_stack(x3_stack_kernel(hp, pk), pk, st, a);
    }
}

int x3_backward(const mshgnn_plan* p, const StepCall& c) {
    const HostPlan& hp = p->hp;
    const LaunchTraits& tr = X3_TRAITS;
    mshgnn_ws_layout lay; layout_workspace(hp, c.batch, 1, &lay);
    const int B = (int)c.batch;
    hipStream_t st = c.stream;
    if (!c.dec_done && c.gw_phase != 1) {
        DecArgs a{};
        fill_dec_bwd_args(p, c, lay, a);
        ProfScope ps(p, hp.ks_dec_bwd, st);
        hipLaunchKernelGGL((k_dec_bwd<T16, true>), dim3(NWG_DEC), dim3(256), 0, st, a);
    }
    if (c.gw_phase != 1 && !c.stack_done) {
        StackArgs a{};
        x3_stack_args(p, c, lay, a);
        a.tile_in = c.ws + lay.dx[hp.L]; a.training = 1;
        const pick::StackPick pk = pick::pick_stack(stack_query(p, c, pick::PLAN_X3, pick::OP_BWD, tr.blk, a));
        apply_stack_pick(hp, pk, lay, a);
        ProfScope ps(p, hp.ks_stack_bwd, st);
        if (int rc = launch_stack(x3_stack_kernel(hp, pk), pk, st, a)) return rc;
    }
    const int gw_parts = gw_parts_for(hp.n_parts, hp.n_lanes, hp.gw_ipl, B, tr.gw_windows, p->n_cu);      // window parts of this batch's weight-gradient launch (32-window steps)
    if (c.grad_params) {      // (NULL: activation backward only)
        GradwArgs a{};
        fill_gradw_args(p, c, lay, tr, gw_parts, a);
        ProfScope ps(p, hp.ks_gradw, st);
        const dim3 grid(a.side.n_grid + std::max(a.n_pad, 0) * gw_parts);      // the slab-free finalize workgroups first
        a.n_pad = std::max(a.n_pad, 1);      // (a phase without lanes: only those workgroups)
        if (grid.x == 0) {}
        else if (a.aligned) hipLaunchKernelGGL(k_gradw_x3_lean<true>, grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL(k_gradw_x3_lean<false>, grid, dim3(256), 0, st, a);
    }
    return run_finalize(p, c, lay, gw_parts);
}
