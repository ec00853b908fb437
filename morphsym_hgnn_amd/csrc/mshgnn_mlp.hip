// MLP baselines (include/mshgnn.h, "MLP baselines"): y = W_L relu(... relu(W_1 x + b_1) ...) + b_L, the reference's nn.Sequential (gnnLightning.py:391-405),
// on bf16 MFMA operands with fp32 accumulation.  Launches of one step, all on the caller's stream:
//   k_mlp_pack    the fp32 weights rounded to bf16: W_1 [H][K1p] (K zero-padded to 128), W_l and W_l^T for l = 2 .. L (the output layer padded to 16 rows / 32 columns)
//   k_mlp_in      A_1 = relu(X W_1^T + b_1) -> bf16 stash.  X: dense bf16 rows, or gathered per 8-element K chunk from the resident bf16 series (mlp_fetch8: one
//                 unaligned 16-byte load, two and a splice where the chunk straddles two runs; element-wise for history < 8).  Series form: the first workgroups
//                 compute the window labels (window_labels_one), as the HGNN encoders do.
//   k_mlp_stack   one workgroup per 32-row tile: layers 2 .. L with the activations in LDS and the weights streamed; then (step) the loss tail, or (backward) the
//                 caller's gout; then the backward sweep dZ_L -> dZ_1 through W_l^T with the ReLU masks read from the stashes.  forward stops after the output.
//   k_mlp_wgrad   dW_l = dZ_l^T A_{l-1} and db_l = column sums of dZ_l for every layer in one launch, partial sums per row slab; layer 1's A operand is X, dense or
//                 gathered from the series again.
//   k_mlp_reduce  grad = the slabs added in slab order; one more workgroup adds the tiles' loss terms in tile order.
// Rounding points (bf16, round to nearest even): X (given as bf16), every weight, A_l = relu(Z_l + b_l) for l < L, dZ_L = the loss gradient (or gout), dZ_l for l < L.
// Z_l, the bias add, out, the loss and every dW / db are fp32.
// Split plan (dtype MSHGNN_BF16X3, the arithmetic of mshgnn_x3.hip): the same five launches (k_mlp_pack_x3, k_mlp_in_x3, k_mlp_stack_x3, k_mlp_wgrad_x3, k_mlp_reduce) with
// every operand of a product as hi = bf16(v), lo = bf16(v - hi) and every product as hi hi + lo hi + hi lo, fp32 accumulation.  X: dense fp32 rows, split in registers
// while they are staged (no series form).  Every packed weight region is a hi image followed by a lo image; every stash and dZ row is [hi | lo] (A_l, dZ_l: 2 H bf16,
// dZ_L: 2 x 16).  Rounding points: the second rounding (lo) of X, every weight, A_l and dZ_l; the ReLU mask of the backward sweep is [hi > 0].
#include <algorithm>
#include <new>

#include "mshgnn_enc.hpp"

namespace {

constexpr int MLP_TILE = 32;            // rows per workgroup tile (k_mlp_in, k_mlp_stack, one step of k_mlp_wgrad)
constexpr int MLP_MAXL = MSHGNN_MLP_MAX_LAYERS;
constexpr int MLP_OPAD = 16;            // the output layer's features, padded to one MFMA block
constexpr int MLP_GK = 32;              // ... and as the K of the first backward product, padded to one MFMA step
constexpr int MLP_SLAB_ROWS = 2048;     // rows per weight-gradient slab (at most MLP_MAX_SLABS slabs: longer slabs beyond)
constexpr int MLP_MAX_SLABS = 8;
constexpr int WG_T = 64;                // k_mlp_wgrad: a workgroup owns a 64 x 64 tile of one layer's dW
constexpr int WG_LD = 68;               // its LDS row stride (elements): 8-byte aligned rows, the transposed 2-byte reads spread over the banks

enum MlpMode { MODE_INFER = 0, MODE_TRAIN_FWD = 1, MODE_STEP = 2, MODE_BWD = 3 };

inline int in_f(const mshgnn_mlp_desc& d, int i) { return i == 0 ? d.in_channels : d.hidden; }
inline int out_f(const mshgnn_mlp_desc& d, int i) { return i == d.num_layers - 1 ? d.out_channels : d.hidden; }
inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

int mlp_check_desc(const mshgnn_mlp_desc* d, int loss_kind, const char* who) {
    if (!d) return set_err(MSHGNN_EINVAL, std::string("null argument to ") + who);
    if (d->dtype != MSHGNN_BF16 && d->dtype != MSHGNN_BF16X3)
        return set_err(MSHGNN_EUNSUPPORTED, std::string(who) + ": the fused MLP runs the bf16 and the split-bf16 arithmetic only (dtype MSHGNN_BF16 or MSHGNN_BF16X3)");
    if (d->hidden < 128 || d->hidden > 512 || d->hidden % 128) return set_err(MSHGNN_EUNSUPPORTED, std::string(who) + ": hidden must be 128, 256, 384 or 512");
    if (d->in_channels < 1 || d->in_channels > 16384) return set_err(MSHGNN_EUNSUPPORTED, std::string(who) + ": in_channels must be in 1..16384");
    if (d->out_channels < 1 || d->out_channels > 16) return set_err(MSHGNN_EUNSUPPORTED, std::string(who) + ": out_channels must be in 1..16");
    if (d->num_layers < 2 || d->num_layers > MLP_MAXL) return set_err(MSHGNN_EUNSUPPORTED, std::string(who) + ": num_layers must be in 2..16");
    if (loss_kind < -1 || loss_kind > 1) return set_err(MSHGNN_EINVAL, std::string(who) + ": loss_kind must be -1, 0 (MSE) or 1 (cross entropy)");
    if (loss_kind == 1 && d->out_channels % 2) return set_err(MSHGNN_EUNSUPPORTED, std::string(who) + ": cross entropy needs an even out_channels (logit pairs)");
    return MSHGNN_OK;
}

void mlp_fill_info(const mshgnn_mlp_desc& d, mshgnn_mlp_info& info) {
    memset(&info, 0, sizeof(info));
    int64_t off = 0;
    double macs = 0;
    for (int i = 0; i < d.num_layers; ++i) {
        info.off_w[i] = off; off += (int64_t)out_f(d, i) * in_f(d, i);
        info.off_b[i] = off; off += out_f(d, i);
        macs += (double)out_f(d, i) * in_f(d, i);
    }
    info.n_flat = off;
    info.rows_per_tile = MLP_TILE;
    info.n_launches_step = 5;
    info.lds_bytes = (d.dtype == MSHGNN_BF16X3 ? 2 : 1) * 2 * MLP_TILE * (d.hidden + 8) * 2 + MLP_TILE * MLP_OPAD * 4 + 256 * 4;      // (split plan: a hi and a lo plane per buffer)
    info.flops_fwd = 2 * macs;
    info.flops_bwd = 4 * macs - 2.0 * d.hidden * d.in_channels;      // dW of every layer + dA of every layer but the first
}

// ---- workspace ----
struct MlpWs {
    size_t total;
    size_t w1p, wp[MLP_MAXL + 1], wtp[MLP_MAXL + 1];      // packed bf16 weights, layer l = 1 .. L (wp[1] unused: w1p); split plan: the hi image, then the lo image
    size_t act[MLP_MAXL + 1];                             // bf16 stashes A_l, l = 1 .. L - 1 ([Bp][H]; split plan [Bp][hi H | lo H])
    size_t dz[MLP_MAXL + 1];                              // bf16 dZ_l, l = 1 .. L ([Bp][H]; dZ_L [Bp][16]; split plan [Bp][hi | lo])
    size_t loss_part, slabs;
    int64_t Bp, ntiles, slab_rows; int nslab; int K1p;
};
MlpWs mlp_layout(const mshgnn_mlp_desc& d, int64_t n_flat, int64_t B, bool training) {
    MlpWs w; memset(&w, 0, sizeof(w));
    const size_t H = d.hidden; const int L = d.num_layers;
    const size_t eb = d.dtype == MSHGNN_BF16X3 ? 4 : 2;      // bytes per stored element: one bf16, or the pair
    w.ntiles = (B + MLP_TILE - 1) / MLP_TILE; w.Bp = w.ntiles * MLP_TILE;
    w.K1p = (d.in_channels + 127) / 128 * 128;      // whole trips of k_mlp_in's K loop
    w.nslab = (int)std::min<int64_t>(MLP_MAX_SLABS, std::max<int64_t>(1, (B + MLP_SLAB_ROWS - 1) / MLP_SLAB_ROWS));
    w.slab_rows = ((B + w.nslab - 1) / w.nslab + MLP_TILE - 1) / MLP_TILE * MLP_TILE;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += up256(bytes); return at; };
    w.w1p = take(H * w.K1p * eb);
    for (int l = 2; l <= L; ++l) {
        w.wp[l] = take((l == L ? (size_t)MLP_OPAD : H) * H * eb);
        if (training) w.wtp[l] = take(H * (l == L ? (size_t)MLP_GK : H) * eb);
    }
    w.act[1] = take((size_t)w.Bp * H * eb);
    if (training) {
        for (int l = 2; l < L; ++l) w.act[l] = take((size_t)w.Bp * H * eb);
        for (int l = 1; l < L; ++l) w.dz[l] = take((size_t)w.Bp * H * eb);
        w.dz[L] = take((size_t)w.Bp * MLP_OPAD * eb);
        w.loss_part = take((size_t)w.ntiles * 4);
        w.slabs = take((size_t)w.nslab * n_flat * 4);
    }
    w.total = o;
    return w;
}

// ---- the batch's rows: dense bf16 rows, or windows of the resident bf16 series ----
struct MlpIn {
    const __bf16* x; int64_t pitch;                                   // dense (split plan: fp32 rows behind the same pointer, pitch in floats)
    const unsigned long long* run_ptr; const int64_t* starts; int T;  // series
    int in; int64_t B;
};
struct RowRef { const __bf16* p; int64_t s; };
template <bool SERIES> __device__ __forceinline__ RowRef mlp_row(const MlpIn& a, int64_t b) {      // b < B
    RowRef r; r.p = nullptr; r.s = 0;
    if constexpr (SERIES) r.s = a.starts[b]; else r.p = a.x + b * a.pitch;
    return r;
}
// elements [k0, k0 + 8) of a row as 8 bf16 (k0 a multiple of 8); elements at or beyond `in` are zeros
template <bool SERIES> __device__ __forceinline__ u32x4 mlp_fetch8(const MlpIn& a, const RowRef& r, int k0) {
    u32x4 v = u32x4{0, 0, 0, 0};
    const int nvalid = a.in - k0;
    if (nvalid <= 0) return v;
    if constexpr (!SERIES) {
        v = *reinterpret_cast<const u32x4*>(r.p + k0);
    } else {
        const int T = a.T;
        if (T >= 8) {
            const u32x4 ones = u32x4{0x3f803f80u, 0x3f803f80u, 0x3f803f80u, 0x3f803f80u};      // a constant-1 run (run pointer 0)
            const int j = k0 / T, off = k0 - j * T, n0 = min(8, T - off);
            const unsigned long long pa = a.run_ptr[j];
            v = ones;
            if (pa) v = *reinterpret_cast<const u32x4*>(reinterpret_cast<const __bf16*>(pa) + r.s + off);      // 2-byte aligned; may run into the column's slack
            if (min(nvalid, 8) > n0) {      // the chunk's tail belongs to run j + 1 (then n0 < 8, and (j + 1) T = k0 + n0 < in: the run exists)
                const unsigned long long pb = a.run_ptr[j + 1];
                u32x4 vb = ones;
                if (pb) vb = *reinterpret_cast<const u32x4*>(reinterpret_cast<const __bf16*>(pb) + r.s);
                v = splice8(v, vb, n0);
            }
        } else {      // runs shorter than a chunk: element by element
            unsigned e16[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                e16[e] = 0u;
                const int k = k0 + e;
                if (k < a.in) {
                    const int j = k / T, off = k - j * T;
                    const unsigned long long p = a.run_ptr[j];
                    e16[e] = p ? (unsigned)reinterpret_cast<const unsigned short*>(p)[r.s + off] : 0x3f80u;
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = e16[2 * q] | (e16[2 * q + 1] << 16);
        }
    }
    if (nvalid < 8) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const unsigned lo = 2 * q < nvalid ? 0xffffu : 0u, hi = 2 * q + 1 < nvalid ? 0xffff0000u : 0u;
            v[q] &= lo | hi;
        }
    }
    return v;
}

__device__ __forceinline__ u32x2 pack4_bf16(f32x4 v) {
    union { u32x2 r; __bf16 e[4]; } u;
#pragma unroll
    for (int i = 0; i < 4; ++i) u.e[i] = (__bf16)v[i];
    return u.r;
}
__device__ __forceinline__ f32x4 mfma_bf16(u32x4 a, u32x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// ---- run pointers of the series form (what k_series_run_ptrs of mshgnn.hip resolves, for unsigned tables and any number of runs) ----
struct MlpSrc { const void* src16[WIN_MAX_SRC]; int64_t cstride[WIN_MAX_SRC]; };
__global__ void k_mlp_run_ptrs(const int* runs, int n_runs, MlpSrc s, unsigned long long* run_ptr) {
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < n_runs; r += gridDim.x * blockDim.x) {
        const int sc = runs[(size_t)r * 5 + 3];
        unsigned long long p = 0ull;
#pragma unroll
        for (int k = 0; k < WIN_MAX_SRC; ++k)
            if (sc >= 0 && (sc >> 8) == k) p = (unsigned long long)(reinterpret_cast<const char*>(s.src16[k]) + (size_t)(sc & 0xff) * s.cstride[k] * 2);
        run_ptr[r] = p;
    }
}

// ---- weight pack ----
struct PackRegion { __bf16* dst; int64_t src; int rows, cols, srows, scols, transposed; };      // dst [rows][cols] <- W [srows][scols] at params + src (or its transpose), zero-padded
struct PackArgs { PackRegion r[2 * MLP_MAXL]; int64_t prefix[2 * MLP_MAXL + 1]; int n; };
__global__ __launch_bounds__(256) void k_mlp_pack(PackArgs a, const float* params) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= a.prefix[a.n]) return;
    int i = 0;
    while (i + 1 < a.n && idx >= a.prefix[i + 1]) ++i;
    const PackRegion& g = a.r[i];
    const int64_t local = idx - a.prefix[i];
    const int row = (int)(local / g.cols), col = (int)(local - (int64_t)row * g.cols);
    const int sr = g.transposed ? col : row, sc = g.transposed ? row : col;
    float v = 0.f;
    if (sr < g.srows && sc < g.scols) v = params[g.src + (int64_t)sr * g.scols + sc];
    g.dst[local] = (__bf16)v;
}

// ---- input layer ----
struct InArgs {
    MlpIn in; const __bf16* w1p; int K1p; const float* bias; __bf16* act1; int H; int lab_blocks; LabelArgs lab;
};
template <bool SERIES> __global__ __launch_bounds__(256) void k_mlp_in(InArgs a) {
    const int tid = threadIdx.x;
    if constexpr (SERIES) {
        if ((int)blockIdx.x < a.lab_blocks) {
            const int64_t b = (int64_t)blockIdx.x * 256 + tid;
            if (b < a.lab.B) window_labels_one<false>(a.lab, b);
            return;
        }
    }
    const int64_t bid = (int64_t)blockIdx.x - (SERIES ? a.lab_blocks : 0);
    const int nh = a.H / 128;
    const int64_t tile = bid / nh; const int hc = (int)(bid - tile * nh);
    const int wave = tid >> 6, lane = tid & 63, g = lane >> 4, c = lane & 15;
    const int n0 = hc * 128 + wave * 32;
    const int64_t b0 = tile * MLP_TILE;
    RowRef rr[2];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) rr[rb] = mlp_row<SERIES>(a.in, min(b0 + rb * 16 + c, a.in.B - 1));
    f32x4 acc[2][2];
#pragma unroll
    for (int fb = 0; fb < 2; ++fb)
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) acc[fb][rb] = f32x4{0.f, 0.f, 0.f, 0.f};
    const __bf16* w0 = a.w1p + (size_t)(n0 + c) * a.K1p + 8 * g;
    const __bf16* w1 = w0 + (size_t)16 * a.K1p;
    // four K steps per trip, their loads issued together: a step's gather is two dependent round trips (run pointer, then the series), and one step per trip left
    // the launch waiting on 254 of them in a row at K = 8100 (K1p is a multiple of 128: the pack's zero columns and mlp_fetch8's zeros fill the last trip)
    for (int ks = 0; ks < a.K1p; ks += 128) {
        u32x4 x0[4], x1[4], wa[4], wb[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k0 = ks + 32 * u + 8 * g;
            x0[u] = mlp_fetch8<SERIES>(a.in, rr[0], k0); x1[u] = mlp_fetch8<SERIES>(a.in, rr[1], k0);
            wa[u] = *reinterpret_cast<const u32x4*>(w0 + ks + 32 * u); wb[u] = *reinterpret_cast<const u32x4*>(w1 + ks + 32 * u);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            acc[0][0] = mfma_bf16(wa[u], x0[u], acc[0][0]); acc[0][1] = mfma_bf16(wa[u], x1[u], acc[0][1]);
            acc[1][0] = mfma_bf16(wb[u], x0[u], acc[1][0]); acc[1][1] = mfma_bf16(wb[u], x1[u], acc[1][1]);
        }
    }
#pragma unroll
    for (int fb = 0; fb < 2; ++fb) {
        const int f = n0 + fb * 16 + 4 * g;
        const f32x4 bv = f32x4{a.bias[f], a.bias[f + 1], a.bias[f + 2], a.bias[f + 3]};
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) {
            const int64_t b = b0 + rb * 16 + c;
            f32x4 v;
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = b < a.in.B ? fmaxf(acc[fb][rb][i] + bv[i], 0.f) : 0.f;
            *reinterpret_cast<u32x2*>(a.act1 + (size_t)b * a.H + f) = pack4_bf16(v);
        }
    }
}

// ---- stack ----
struct StackArgs {
    int H, out, L, mode, loss_kind; int64_t B; float inv;
    const float* params; int64_t off_b[MLP_MAXL + 1];      // bias of layer l = 1 .. L
    const __bf16* wp[MLP_MAXL + 1]; const __bf16* wtp[MLP_MAXL + 1]; __bf16* act[MLP_MAXL + 1]; __bf16* dz[MLP_MAXL + 1];
    float* out_p; const float* y; const int32_t* labels; const float* gout; float* loss_part;
};
// D[n][row] = sum_k W[n][k] X[row][k] over the tile's 32 rows: W global bf16 [N][Kw] (N a multiple of 16, Kw of 32), X in LDS at stride xs.
// epi(first of 4 consecutive features, row in the tile, the 4 sums); the (feature, row) -> thread map depends on N alone.
template <typename Epi> __device__ __forceinline__ void mlp_layer(const __bf16* W, int N, int Kw, const __bf16* X, int xs, int wave, int lane, Epi epi) {
    const int g = lane >> 4, c = lane & 15;
    for (int fb = wave; fb < N / 16; fb += 4) {
        f32x4 a0 = f32x4{0.f, 0.f, 0.f, 0.f}, a1 = a0;
        const __bf16* wr = W + (size_t)(fb * 16 + c) * Kw + 8 * g;
        const __bf16* x0 = X + c * xs + 8 * g;
        const __bf16* x1 = x0 + 16 * xs;
        for (int k = 0; k < Kw; k += 32) {
            const u32x4 wf = *reinterpret_cast<const u32x4*>(wr + k);
            const u32x4 f0 = *reinterpret_cast<const u32x4*>(x0 + k), f1 = *reinterpret_cast<const u32x4*>(x1 + k);
            a0 = mfma_bf16(wf, f0, a0); a1 = mfma_bf16(wf, f1, a1);
        }
        epi(fb * 16 + 4 * g, c, a0); epi(fb * 16 + 4 * g, 16 + c, a1);
    }
}

__global__ __launch_bounds__(256) void k_mlp_stack(StackArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int H = a.H, xs = H + 8, L = a.L;
    __bf16* buf0 = reinterpret_cast<__bf16*>(smem);
    __bf16* buf1 = buf0 + MLP_TILE * xs;
    float* obuf = reinterpret_cast<float*>(buf1 + MLP_TILE * xs);
    float* red = obuf + MLP_TILE * MLP_OPAD;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t b0 = (int64_t)blockIdx.x * MLP_TILE;
    __bf16* cur = buf0; __bf16* nxt = buf1;
    const bool stash = a.mode != MODE_INFER;
    if (a.mode != MODE_BWD) {
        // A_1 of the tile (rows past the batch: the zeros k_mlp_in wrote)
        const int cpr = H / 8;
        for (int i = tid; i < MLP_TILE * cpr; i += 256) {
            const int row = i / cpr, ch = i - row * cpr;
            *reinterpret_cast<u32x4*>(cur + row * xs + ch * 8) = *reinterpret_cast<const u32x4*>(a.act[1] + (size_t)(b0 + row) * H + ch * 8);
        }
        __syncthreads();
        for (int l = 2; l < L; ++l) {
            const float* bias = a.params + a.off_b[l];
            __bf16* st = a.act[l];
            mlp_layer(a.wp[l], H, H, cur, xs, wave, lane, [&](int f, int row, f32x4 s) {
                const bool live = b0 + row < a.B;
                f32x4 v;
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = live ? fmaxf(s[i] + bias[f + i], 0.f) : 0.f;
                const u32x2 pk = pack4_bf16(v);
                *reinterpret_cast<u32x2*>(nxt + row * xs + f) = pk;
                if (stash) *reinterpret_cast<u32x2*>(st + (size_t)(b0 + row) * H + f) = pk;
            });
            __syncthreads();
            __bf16* t = cur; cur = nxt; nxt = t;
        }
        {
            const float* bias = a.params + a.off_b[L];
            mlp_layer(a.wp[L], MLP_OPAD, H, cur, xs, wave, lane, [&](int f, int row, f32x4 s) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float v = f + i < a.out ? s[i] + bias[f + i] : 0.f;
                    obuf[row * MLP_OPAD + f + i] = v;
                    if (f + i < a.out && b0 + row < a.B) a.out_p[(size_t)(b0 + row) * a.out + f + i] = v;
                }
            });
        }
        __syncthreads();
        if (a.mode != MODE_STEP) return;
    }
    // dZ_L: the loss tail (step) or the caller's gout (backward); thread = (row, logit pair)
    {
        const int row = tid >> 3, p = tid & 7, f0 = 2 * p;
        const int64_t b = b0 + row;
        float g0 = 0.f, g1 = 0.f, term = 0.f;
        if (b < a.B) {
            if (a.mode == MODE_STEP) {
                const float o0 = obuf[row * MLP_OPAD + f0], o1 = obuf[row * MLP_OPAD + f0 + 1];
                if (a.loss_kind == 0) {
                    if (f0 < a.out) { const float d = o0 - a.y[(size_t)b * a.out + f0]; g0 = 2.0f * d * a.inv; term = d * d; }
                    if (f0 + 1 < a.out) { const float d = o1 - a.y[(size_t)b * a.out + f0 + 1]; g1 = 2.0f * d * a.inv; term += d * d; }
                } else if (f0 + 1 < a.out) {
                    const int cls = a.labels[(size_t)b * (a.out / 2) + p] != 0;
                    const float m = fmaxf(o0, o1), e0 = expf(o0 - m), e1 = expf(o1 - m), s = e0 + e1;
                    term = logf(s) + m - (cls ? o1 : o0);
                    g0 = (e0 / s - (cls ? 0.f : 1.f)) * a.inv; g1 = (e1 / s - (cls ? 1.f : 0.f)) * a.inv;
                }
            } else {
                if (f0 < a.out) g0 = a.gout[(size_t)b * a.out + f0];
                if (f0 + 1 < a.out) g1 = a.gout[(size_t)b * a.out + f0 + 1];
            }
        }
        union { unsigned u; __bf16 e[2]; } pk;
        pk.e[0] = (__bf16)g0; pk.e[1] = (__bf16)g1;
        *reinterpret_cast<unsigned*>(nxt + row * xs + f0) = pk.u;
        *reinterpret_cast<unsigned*>(nxt + row * xs + MLP_OPAD + f0) = 0u;      // K columns 16 .. 31 of the first backward product
        *reinterpret_cast<unsigned*>(a.dz[L] + (size_t)b * MLP_OPAD + f0) = pk.u;
        if (a.mode == MODE_STEP) {
            red[tid] = term;
            __syncthreads();
            for (int s = 128; s > 0; s >>= 1) {
                if (tid < s) red[tid] += red[tid + s];
                __syncthreads();
            }
            if (tid == 0) a.loss_part[blockIdx.x] = red[0];
        }
    }
    __syncthreads();
    { __bf16* t = cur; cur = nxt; nxt = t; }
    // backward sweep: dZ_{l-1} = (dZ_l W_l) . [A_{l-1} > 0]
    int Kw = MLP_GK;
    for (int l = L; l >= 2; --l) {
        const __bf16* am = a.act[l - 1];
        __bf16* dzo = a.dz[l - 1];
        mlp_layer(a.wtp[l], H, Kw, cur, xs, wave, lane, [&](int f, int row, f32x4 s) {
            const f32x4 av = load_quad(am + (size_t)(b0 + row) * H + f);
            f32x4 v;
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = av[i] > 0.f ? s[i] : 0.f;
            const u32x2 pk = pack4_bf16(v);
            *reinterpret_cast<u32x2*>(nxt + row * xs + f) = pk;
            *reinterpret_cast<u32x2*>(dzo + (size_t)(b0 + row) * H + f) = pk;
        });
        __syncthreads();
        __bf16* t = cur; cur = nxt; nxt = t;
        Kw = H;
    }
}

// ---- weight gradients ----
struct WgArgs {
    int L, H, in, out, nslab; int64_t B, slab_rows, n_flat;
    int prefix[MLP_MAXL + 2];      // workgroups (dW tiles) of layer l = 1 .. L start at prefix[l]; prefix[L + 1] = all
    int itiles[MLP_MAXL + 1];
    const __bf16* dz[MLP_MAXL + 1]; const __bf16* act[MLP_MAXL + 1];
    int64_t off_w[MLP_MAXL + 1], off_b[MLP_MAXL + 1];
    float* slabs; MlpIn xin;
};
template <bool SERIES> __global__ __launch_bounds__(256) void k_mlp_wgrad(WgArgs a) {
    __shared__ __attribute__((aligned(16))) __bf16 sdz[MLP_TILE * WG_LD];
    __shared__ __attribute__((aligned(16))) __bf16 sx[MLP_TILE * WG_LD];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, c = lane & 15;
    const int per_slab = a.prefix[a.L + 1];
    const int slab = (int)(blockIdx.x / per_slab), r = (int)(blockIdx.x - (unsigned)slab * per_slab);
    int l = 1;
    while (l < a.L && r >= a.prefix[l + 1]) ++l;
    const int local = r - a.prefix[l];
    const int jt = local / a.itiles[l], it = local - jt * a.itiles[l];
    const int Jd = l == a.L ? a.out : a.H, zs = l == a.L ? MLP_OPAD : a.H, Id = l == 1 ? a.in : a.H;
    const __bf16* dz = a.dz[l];
    const __bf16* ap = a.act[l - 1];      // (l == 1: null, the rows come from xin)
    const int64_t r0 = (int64_t)slab * a.slab_rows, r1 = min(r0 + a.slab_rows, a.B);
    const int srow = tid >> 3, ch = tid & 7;
    const int jcol = jt * WG_T + ch * 8, icol = it * WG_T + ch * 8;
    f32x4 acc[4];
#pragma unroll
    for (int ib = 0; ib < 4; ++ib) acc[ib] = f32x4{0.f, 0.f, 0.f, 0.f};
    float bsum = 0.f;
    for (int64_t rb = r0; rb < r1; rb += MLP_TILE) {
        const int64_t b = rb + srow;
        u32x4 vz = u32x4{0, 0, 0, 0}, vx = u32x4{0, 0, 0, 0};
        if (b < r1) {
            if (jcol < zs) vz = *reinterpret_cast<const u32x4*>(dz + (size_t)b * zs + jcol);
            if (l == 1) vx = mlp_fetch8<SERIES>(a.xin, mlp_row<SERIES>(a.xin, b), icol);
            else if (icol < a.H) vx = *reinterpret_cast<const u32x4*>(ap + (size_t)b * a.H + icol);
        }
        __syncthreads();      // the previous step's reads are done
        *reinterpret_cast<u32x2*>(sdz + srow * WG_LD + ch * 8) = u32x2{vz[0], vz[1]};
        *reinterpret_cast<u32x2*>(sdz + srow * WG_LD + ch * 8 + 4) = u32x2{vz[2], vz[3]};
        *reinterpret_cast<u32x2*>(sx + srow * WG_LD + ch * 8) = u32x2{vx[0], vx[1]};
        *reinterpret_cast<u32x2*>(sx + srow * WG_LD + ch * 8 + 4) = u32x2{vx[2], vx[3]};
        __syncthreads();
        // operands of the row-reduction: element e of lane group g is row 8 g + e of the step
        const unsigned short* zz = reinterpret_cast<const unsigned short*>(sdz) + (8 * g) * WG_LD + wave * 16 + c;
        u32x4 zf;
#pragma unroll
        for (int q = 0; q < 4; ++q) zf[q] = (unsigned)zz[(2 * q) * WG_LD] | ((unsigned)zz[(2 * q + 1) * WG_LD] << 16);
#pragma unroll
        for (int ib = 0; ib < 4; ++ib) {
            const unsigned short* xx = reinterpret_cast<const unsigned short*>(sx) + (8 * g) * WG_LD + ib * 16 + c;
            u32x4 xf;
#pragma unroll
            for (int q = 0; q < 4; ++q) xf[q] = (unsigned)xx[(2 * q) * WG_LD] | ((unsigned)xx[(2 * q + 1) * WG_LD] << 16);
            acc[ib] = mfma_bf16(zf, xf, acc[ib]);
        }
        if (it == 0 && tid < WG_T) {
#pragma unroll 8
            for (int rw = 0; rw < MLP_TILE; ++rw) bsum += (float)sdz[rw * WG_LD + tid];
        }
    }
    float* sl = a.slabs + (size_t)slab * a.n_flat;
#pragma unroll
    for (int ib = 0; ib < 4; ++ib) {
        const int i = it * WG_T + ib * 16 + c;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int j = jt * WG_T + wave * 16 + 4 * g + q;
            if (j < Jd && i < Id) sl[a.off_w[l] + (int64_t)j * Id + i] = acc[ib][q];
        }
    }
    if (it == 0 && tid < WG_T && jt * WG_T + tid < Jd) sl[a.off_b[l] + jt * WG_T + tid] = bsum;
}

// ---- the split plan: the four launches above on hi / lo pairs (k_mlp_reduce is shared) ----
__device__ __forceinline__ f32x4 widen4_bf16(u32x2 r) {
    return f32x4{__builtin_bit_cast(float, r[0] << 16), __builtin_bit_cast(float, r[0] & 0xffff0000u), __builtin_bit_cast(float, r[1] << 16), __builtin_bit_cast(float, r[1] & 0xffff0000u)};
}
__device__ __forceinline__ void split_quad(f32x4 v, u32x2& hi, u32x2& lo) {      // split_oct (mshgnn_device.hpp) on four values
    hi = pack4_bf16(v);
    lo = pack4_bf16(v - widen4_bf16(hi));
}
// elements [k0, k0 + 8) of a dense fp32 row as a hi and a lo oct (k0 a multiple of 8); elements at or beyond `in` are zeros, whatever the pad columns hold
__device__ __forceinline__ void mlp_fetch8_x3(const float* row, int in, int k0, u32x4& hi, u32x4& lo) {
    f32x4 a = f32x4{0.f, 0.f, 0.f, 0.f}, b = a;
    const int nvalid = in - k0;
    if (nvalid > 0) {      // (the pitch covers `in` rounded up to 8: both loads stay inside the row)
        a = load_quad(row + k0); b = load_quad(row + k0 + 4);
        if (nvalid < 8) {
#pragma unroll
            for (int i = 0; i < 4; ++i) { if (i >= nvalid) a[i] = 0.f; if (4 + i >= nvalid) b[i] = 0.f; }
        }
    }
    split_oct(a, b, hi, lo);
}

__global__ __launch_bounds__(256) void k_mlp_pack_x3(PackArgs a, const float* params) {      // k_mlp_pack; region i: the hi image [rows][cols], the lo image behind it
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= a.prefix[a.n]) return;
    int i = 0;
    while (i + 1 < a.n && idx >= a.prefix[i + 1]) ++i;
    const PackRegion& g = a.r[i];
    const int64_t local = idx - a.prefix[i];
    const int row = (int)(local / g.cols), col = (int)(local - (int64_t)row * g.cols);
    const int sr = g.transposed ? col : row, sc = g.transposed ? row : col;
    float v = 0.f;
    if (sr < g.srows && sc < g.scols) v = params[g.src + (int64_t)sr * g.scols + sc];
    const __bf16 hi = (__bf16)v;
    g.dst[local] = hi;
    g.dst[(int64_t)g.rows * g.cols + local] = (__bf16)(v - (float)hi);
}

// k_mlp_in's tile and thread map; two K steps per trip (the fp32 rows and both weight images of four steps would not fit the registers of two waves per SIMD)
__global__ __launch_bounds__(256) void k_mlp_in_x3(InArgs a) {
    const int tid = threadIdx.x;
    const int nh = a.H / 128;
    const int64_t tile = blockIdx.x / nh; const int hc = (int)(blockIdx.x - tile * nh);
    const int wave = tid >> 6, lane = tid & 63, g = lane >> 4, c = lane & 15;
    const int n0 = hc * 128 + wave * 32;
    const int64_t b0 = tile * MLP_TILE;
    const float* xr[2];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) xr[rb] = reinterpret_cast<const float*>(a.in.x) + min(b0 + rb * 16 + c, a.in.B - 1) * a.in.pitch;
    f32x4 acc[2][2];
#pragma unroll
    for (int fb = 0; fb < 2; ++fb)
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) acc[fb][rb] = f32x4{0.f, 0.f, 0.f, 0.f};
    const size_t wlo = (size_t)a.H * a.K1p;      // the lo image
    const __bf16* wr[2];
    wr[0] = a.w1p + (size_t)(n0 + c) * a.K1p + 8 * g; wr[1] = wr[0] + (size_t)16 * a.K1p;
    for (int ks = 0; ks < a.K1p; ks += 64) {
        u32x4 xh[2][2], xl[2][2], wh[2][2], wl[2][2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int k0 = ks + 32 * u + 8 * g;
#pragma unroll
            for (int rb = 0; rb < 2; ++rb) mlp_fetch8_x3(xr[rb], a.in.in, k0, xh[u][rb], xl[u][rb]);
#pragma unroll
            for (int fb = 0; fb < 2; ++fb) {
                wh[u][fb] = *reinterpret_cast<const u32x4*>(wr[fb] + ks + 32 * u); wl[u][fb] = *reinterpret_cast<const u32x4*>(wr[fb] + wlo + ks + 32 * u);
            }
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
#pragma unroll
            for (int fb = 0; fb < 2; ++fb)
#pragma unroll
                for (int rb = 0; rb < 2; ++rb) acc[fb][rb] = mfma_bf16(wh[u][fb], xh[u][rb], acc[fb][rb]);
#pragma unroll
            for (int fb = 0; fb < 2; ++fb)
#pragma unroll
                for (int rb = 0; rb < 2; ++rb) acc[fb][rb] = mfma_bf16(wl[u][fb], xh[u][rb], acc[fb][rb]);
#pragma unroll
            for (int fb = 0; fb < 2; ++fb)
#pragma unroll
                for (int rb = 0; rb < 2; ++rb) acc[fb][rb] = mfma_bf16(wh[u][fb], xl[u][rb], acc[fb][rb]);
        }
    }
#pragma unroll
    for (int fb = 0; fb < 2; ++fb) {
        const int f = n0 + fb * 16 + 4 * g;
        const f32x4 bv = f32x4{a.bias[f], a.bias[f + 1], a.bias[f + 2], a.bias[f + 3]};
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) {
            const int64_t b = b0 + rb * 16 + c;
            f32x4 v;
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = b < a.in.B ? fmaxf(acc[fb][rb][i] + bv[i], 0.f) : 0.f;
            u32x2 hi, lo;
            split_quad(v, hi, lo);
            __bf16* dst = a.act1 + (size_t)b * (2 * a.H) + f;
            *reinterpret_cast<u32x2*>(dst) = hi; *reinterpret_cast<u32x2*>(dst + a.H) = lo;
        }
    }
}

// mlp_layer on pairs: W = the hi image [N][Kw] with the lo image behind it, X = the hi plane in LDS with the lo plane `plane` elements further; per K step
// W_hi X_hi + W_lo X_hi + W_hi X_lo, the two row blocks alternating
template <typename Epi> __device__ __forceinline__ void mlp_layer_x3(const __bf16* W, int N, int Kw, const __bf16* X, int xs, int plane, int wave, int lane, Epi epi) {
    const int g = lane >> 4, c = lane & 15;
    const size_t wlo = (size_t)N * Kw;
    for (int fb = wave; fb < N / 16; fb += 4) {
        f32x4 a0 = f32x4{0.f, 0.f, 0.f, 0.f}, a1 = a0;
        const __bf16* wr = W + (size_t)(fb * 16 + c) * Kw + 8 * g;
        const __bf16* x0 = X + c * xs + 8 * g;
        const __bf16* x1 = x0 + 16 * xs;
        for (int k = 0; k < Kw; k += 32) {
            const u32x4 wh = *reinterpret_cast<const u32x4*>(wr + k), wl = *reinterpret_cast<const u32x4*>(wr + wlo + k);
            const u32x4 h0 = *reinterpret_cast<const u32x4*>(x0 + k), h1 = *reinterpret_cast<const u32x4*>(x1 + k);
            const u32x4 l0 = *reinterpret_cast<const u32x4*>(x0 + plane + k), l1 = *reinterpret_cast<const u32x4*>(x1 + plane + k);
            a0 = mfma_bf16(wh, h0, a0); a1 = mfma_bf16(wh, h1, a1);
            a0 = mfma_bf16(wl, h0, a0); a1 = mfma_bf16(wl, h1, a1);
            a0 = mfma_bf16(wh, l0, a0); a1 = mfma_bf16(wh, l1, a1);
        }
        epi(fb * 16 + 4 * g, c, a0); epi(fb * 16 + 4 * g, 16 + c, a1);
    }
}

// k_mlp_stack on pairs.  LDS: two activation buffers, each a hi plane [32][H + 8] and a lo plane behind it (a row shifts the 16-byte reads of a lane group by
// four banks, as in k_mlp_stack; the planes are read by separate instructions, so the plane stride adds no conflict), then the output and reduction buffers.
__global__ __launch_bounds__(256) void k_mlp_stack_x3(StackArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int H = a.H, xs = H + 8, L = a.L, plane = MLP_TILE * xs, H2 = 2 * H;
    __bf16* buf0 = reinterpret_cast<__bf16*>(smem);
    __bf16* buf1 = buf0 + 2 * plane;
    float* obuf = reinterpret_cast<float*>(buf1 + 2 * plane);
    float* red = obuf + MLP_TILE * MLP_OPAD;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t b0 = (int64_t)blockIdx.x * MLP_TILE;
    __bf16* cur = buf0; __bf16* nxt = buf1;
    const bool stash = a.mode != MODE_INFER;
    if (a.mode != MODE_BWD) {
        // A_1 of the tile, both halves (rows past the batch: the zeros k_mlp_in_x3 wrote)
        const int cpr = H2 / 8;
        for (int i = tid; i < MLP_TILE * cpr; i += 256) {
            const int row = i / cpr, ch = i - row * cpr;
            const int col = ch * 8 < H ? ch * 8 : plane + ch * 8 - H;
            *reinterpret_cast<u32x4*>(cur + row * xs + col) = *reinterpret_cast<const u32x4*>(a.act[1] + (size_t)(b0 + row) * H2 + ch * 8);
        }
        __syncthreads();
        for (int l = 2; l < L; ++l) {
            const float* bias = a.params + a.off_b[l];
            __bf16* st = a.act[l];
            mlp_layer_x3(a.wp[l], H, H, cur, xs, plane, wave, lane, [&](int f, int row, f32x4 s) {
                const bool live = b0 + row < a.B;
                f32x4 v;
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = live ? fmaxf(s[i] + bias[f + i], 0.f) : 0.f;
                u32x2 hi, lo;
                split_quad(v, hi, lo);
                *reinterpret_cast<u32x2*>(nxt + row * xs + f) = hi; *reinterpret_cast<u32x2*>(nxt + plane + row * xs + f) = lo;
                if (stash) {
                    __bf16* dst = st + (size_t)(b0 + row) * H2 + f;
                    *reinterpret_cast<u32x2*>(dst) = hi; *reinterpret_cast<u32x2*>(dst + H) = lo;
                }
            });
            __syncthreads();
            __bf16* t = cur; cur = nxt; nxt = t;
        }
        {
            const float* bias = a.params + a.off_b[L];
            mlp_layer_x3(a.wp[L], MLP_OPAD, H, cur, xs, plane, wave, lane, [&](int f, int row, f32x4 s) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float v = f + i < a.out ? s[i] + bias[f + i] : 0.f;
                    obuf[row * MLP_OPAD + f + i] = v;
                    if (f + i < a.out && b0 + row < a.B) a.out_p[(size_t)(b0 + row) * a.out + f + i] = v;
                }
            });
        }
        __syncthreads();
        if (a.mode != MODE_STEP) return;
    }
    // dZ_L: the loss tail (step) or the caller's gout (backward), k_mlp_stack's arithmetic; thread = (row, logit pair)
    {
        const int row = tid >> 3, p = tid & 7, f0 = 2 * p;
        const int64_t b = b0 + row;
        float g0 = 0.f, g1 = 0.f, term = 0.f;
        if (b < a.B) {
            if (a.mode == MODE_STEP) {
                const float o0 = obuf[row * MLP_OPAD + f0], o1 = obuf[row * MLP_OPAD + f0 + 1];
                if (a.loss_kind == 0) {
                    if (f0 < a.out) { const float d = o0 - a.y[(size_t)b * a.out + f0]; g0 = 2.0f * d * a.inv; term = d * d; }
                    if (f0 + 1 < a.out) { const float d = o1 - a.y[(size_t)b * a.out + f0 + 1]; g1 = 2.0f * d * a.inv; term += d * d; }
                } else if (f0 + 1 < a.out) {
                    const int cls = a.labels[(size_t)b * (a.out / 2) + p] != 0;
                    const float m = fmaxf(o0, o1), e0 = expf(o0 - m), e1 = expf(o1 - m), s = e0 + e1;
                    term = logf(s) + m - (cls ? o1 : o0);
                    g0 = (e0 / s - (cls ? 0.f : 1.f)) * a.inv; g1 = (e1 / s - (cls ? 1.f : 0.f)) * a.inv;
                }
            } else {
                if (f0 < a.out) g0 = a.gout[(size_t)b * a.out + f0];
                if (f0 + 1 < a.out) g1 = a.gout[(size_t)b * a.out + f0 + 1];
            }
        }
        union { unsigned u; __bf16 e[2]; } ph, pl;
        ph.e[0] = (__bf16)g0; ph.e[1] = (__bf16)g1;
        pl.e[0] = (__bf16)(g0 - (float)ph.e[0]); pl.e[1] = (__bf16)(g1 - (float)ph.e[1]);
        *reinterpret_cast<unsigned*>(nxt + row * xs + f0) = ph.u; *reinterpret_cast<unsigned*>(nxt + plane + row * xs + f0) = pl.u;
        *reinterpret_cast<unsigned*>(nxt + row * xs + MLP_OPAD + f0) = 0u;      // K columns 16 .. 31 of the first backward product
        *reinterpret_cast<unsigned*>(nxt + plane + row * xs + MLP_OPAD + f0) = 0u;
        *reinterpret_cast<unsigned*>(a.dz[L] + (size_t)b * (2 * MLP_OPAD) + f0) = ph.u;
        *reinterpret_cast<unsigned*>(a.dz[L] + (size_t)b * (2 * MLP_OPAD) + MLP_OPAD + f0) = pl.u;
        if (a.mode == MODE_STEP) {
            red[tid] = term;
            __syncthreads();
            for (int s = 128; s > 0; s >>= 1) {
                if (tid < s) red[tid] += red[tid + s];
                __syncthreads();
            }
            if (tid == 0) a.loss_part[blockIdx.x] = red[0];
        }
    }
    __syncthreads();
    { __bf16* t = cur; cur = nxt; nxt = t; }
    // backward sweep: dZ_{l-1} = (dZ_l W_l) . [A_{l-1} > 0], the mask from the hi half (hi == 0 implies lo == 0: both roundings are to nearest)
    int Kw = MLP_GK;
    for (int l = L; l >= 2; --l) {
        const __bf16* am = a.act[l - 1];
        __bf16* dzo = a.dz[l - 1];
        mlp_layer_x3(a.wtp[l], H, Kw, cur, xs, plane, wave, lane, [&](int f, int row, f32x4 s) {
            const f32x4 av = load_quad(am + (size_t)(b0 + row) * H2 + f);
            f32x4 v;
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = av[i] > 0.f ? s[i] : 0.f;
            u32x2 hi, lo;
            split_quad(v, hi, lo);
            *reinterpret_cast<u32x2*>(nxt + row * xs + f) = hi; *reinterpret_cast<u32x2*>(nxt + plane + row * xs + f) = lo;
            __bf16* dst = dzo + (size_t)(b0 + row) * H2 + f;
            *reinterpret_cast<u32x2*>(dst) = hi; *reinterpret_cast<u32x2*>(dst + H) = lo;
        });
        __syncthreads();
        __bf16* t = cur; cur = nxt; nxt = t;
        Kw = H;
    }
}

// k_mlp_wgrad on pairs: the hi and lo planes of both operands in LDS (4 x 4352 B), dZ_hi A_hi + dZ_lo A_hi + dZ_hi A_lo per block; db = the column sums of hi + lo
// (exact in fp32) in row order; layer 1's A operand is the fp32 rows, split as k_mlp_in_x3 split them
__global__ __launch_bounds__(256) void k_mlp_wgrad_x3(WgArgs a) {
    __shared__ __attribute__((aligned(16))) __bf16 sdz[2][MLP_TILE * WG_LD];      // [hi, lo]
    __shared__ __attribute__((aligned(16))) __bf16 sx[2][MLP_TILE * WG_LD];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, c = lane & 15;
    const int per_slab = a.prefix[a.L + 1];
    const int slab = (int)(blockIdx.x / per_slab), r = (int)(blockIdx.x - (unsigned)slab * per_slab);
    int l = 1;
    while (l < a.L && r >= a.prefix[l + 1]) ++l;
    const int local = r - a.prefix[l];
    const int jt = local / a.itiles[l], it = local - jt * a.itiles[l];
    const int Jd = l == a.L ? a.out : a.H, zs = l == a.L ? MLP_OPAD : a.H, Id = l == 1 ? a.in : a.H;
    const __bf16* dz = a.dz[l];
    const __bf16* ap = a.act[l - 1];      // (l == 1: null, the rows come from xin)
    const float* xf = reinterpret_cast<const float*>(a.xin.x);
    const int64_t r0 = (int64_t)slab * a.slab_rows, r1 = min(r0 + a.slab_rows, a.B);
    const int srow = tid >> 3, ch = tid & 7;
    const int jcol = jt * WG_T + ch * 8, icol = it * WG_T + ch * 8;
    f32x4 acc[4];
#pragma unroll
    for (int ib = 0; ib < 4; ++ib) acc[ib] = f32x4{0.f, 0.f, 0.f, 0.f};
    float bsum = 0.f;
    for (int64_t rb = r0; rb < r1; rb += MLP_TILE) {
        const int64_t b = rb + srow;
        u32x4 vz[2], vx[2];
        vz[0] = vz[1] = vx[0] = vx[1] = u32x4{0, 0, 0, 0};
        if (b < r1) {
            if (jcol < zs) { vz[0] = *reinterpret_cast<const u32x4*>(dz + (size_t)b * (2 * zs) + jcol); vz[1] = *reinterpret_cast<const u32x4*>(dz + (size_t)b * (2 * zs) + zs + jcol); }
            if (l == 1) mlp_fetch8_x3(xf + b * a.xin.pitch, a.in, icol, vx[0], vx[1]);
            else if (icol < a.H) { vx[0] = *reinterpret_cast<const u32x4*>(ap + (size_t)b * (2 * a.H) + icol); vx[1] = *reinterpret_cast<const u32x4*>(ap + (size_t)b * (2 * a.H) + a.H + icol); }
        }
        __syncthreads();      // the previous step's reads are done
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            *reinterpret_cast<u32x2*>(sdz[h] + srow * WG_LD + ch * 8) = u32x2{vz[h][0], vz[h][1]};
            *reinterpret_cast<u32x2*>(sdz[h] + srow * WG_LD + ch * 8 + 4) = u32x2{vz[h][2], vz[h][3]};
            *reinterpret_cast<u32x2*>(sx[h] + srow * WG_LD + ch * 8) = u32x2{vx[h][0], vx[h][1]};
            *reinterpret_cast<u32x2*>(sx[h] + srow * WG_LD + ch * 8 + 4) = u32x2{vx[h][2], vx[h][3]};
        }
        __syncthreads();
        // operands of the row-reduction: element e of lane group g is row 8 g + e of the step
        u32x4 zf[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const unsigned short* zz = reinterpret_cast<const unsigned short*>(sdz[h]) + (8 * g) * WG_LD + wave * 16 + c;
#pragma unroll
            for (int q = 0; q < 4; ++q) zf[h][q] = (unsigned)zz[(2 * q) * WG_LD] | ((unsigned)zz[(2 * q + 1) * WG_LD] << 16);
        }
#pragma unroll
        for (int ib = 0; ib < 4; ++ib) {
            u32x4 xq[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const unsigned short* xx = reinterpret_cast<const unsigned short*>(sx[h]) + (8 * g) * WG_LD + ib * 16 + c;
#pragma unroll
                for (int q = 0; q < 4; ++q) xq[h][q] = (unsigned)xx[(2 * q) * WG_LD] | ((unsigned)xx[(2 * q + 1) * WG_LD] << 16);
            }
            acc[ib] = mfma_bf16(zf[0], xq[0], acc[ib]);
            acc[ib] = mfma_bf16(zf[1], xq[0], acc[ib]);
            acc[ib] = mfma_bf16(zf[0], xq[1], acc[ib]);
        }
        if (it == 0 && tid < WG_T) {
#pragma unroll 8
            for (int rw = 0; rw < MLP_TILE; ++rw) bsum += (float)sdz[0][rw * WG_LD + tid] + (float)sdz[1][rw * WG_LD + tid];
        }
    }
    float* sl = a.slabs + (size_t)slab * a.n_flat;
#pragma unroll
    for (int ib = 0; ib < 4; ++ib) {
        const int i = it * WG_T + ib * 16 + c;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int j = jt * WG_T + wave * 16 + 4 * g + q;
            if (j < Jd && i < Id) sl[a.off_w[l] + (int64_t)j * Id + i] = acc[ib][q];
        }
    }
    if (it == 0 && tid < WG_T && jt * WG_T + tid < Jd) sl[a.off_b[l] + jt * WG_T + tid] = bsum;
}

// ---- fixed-order sums: the slabs into the gradient, the tiles' loss terms into the loss ----
__global__ __launch_bounds__(256) void k_mlp_reduce(const float* slabs, int nslab, int64_t n_flat, float* grad, int grad_blocks, const float* loss_part, int64_t ntiles,
                                                    float denom, float* loss_out) {
    __shared__ float red[256];
    const int tid = threadIdx.x;
    if ((int)blockIdx.x < grad_blocks) {
        const int64_t p = (int64_t)blockIdx.x * 256 + tid;
        if (p >= n_flat) return;
        float s = slabs[p];
        for (int k = 1; k < nslab; ++k) s += slabs[(size_t)k * n_flat + p];
        grad[p] = s;
        return;
    }
    float s = 0.f;
    for (int64_t t = tid; t < ntiles; t += 256) s += loss_part[t];
    red[tid] = s;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if (tid < k) red[tid] += red[tid + k];
        __syncthreads();
    }
    if (tid == 0) loss_out[0] = red[0] / denom;
}

}  // namespace

struct mshgnn_mlp_plan { mshgnn_mlp_desc d; mshgnn_mlp_info info; };

extern "C" int mshgnn_mlp_compile_host(const mshgnn_mlp_desc* desc, int loss_kind, mshgnn_mlp_info* info) {
    if (!info) return set_err(MSHGNN_EINVAL, "null argument to mshgnn_mlp_compile_host");
    if (int rc = mlp_check_desc(desc, loss_kind, "mshgnn_mlp_compile_host")) return rc;
    mlp_fill_info(*desc, *info);
    return MSHGNN_OK;
}

extern "C" int mshgnn_mlp_create(const mshgnn_mlp_desc* desc, mshgnn_mlp_plan** plan_out) {
    if (!plan_out) return set_err(MSHGNN_EINVAL, "null argument to mshgnn_mlp_create");
    if (int rc = mlp_check_desc(desc, -1, "mshgnn_mlp_create")) return rc;
    mshgnn_mlp_plan* p = new (std::nothrow) mshgnn_mlp_plan;
    if (!p) return set_err(MSHGNN_ENOMEM, "mshgnn_mlp_create: out of memory");
    p->d = *desc;
    mlp_fill_info(p->d, p->info);
    const void* stack = desc->dtype == MSHGNN_BF16X3 ? reinterpret_cast<const void*>(k_mlp_stack_x3) : reinterpret_cast<const void*>(k_mlp_stack);
    hipError_t e = hipFuncSetAttribute(stack, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p->info.lds_bytes);
    if (e != hipSuccess) { delete p; return set_err(MSHGNN_EHIP, std::string("mshgnn_mlp_create: hipFuncSetAttribute: ") + hipGetErrorString(e)); }
    *plan_out = p;
    return MSHGNN_OK;
}
extern "C" void mshgnn_mlp_destroy(mshgnn_mlp_plan* plan) { delete plan; }
extern "C" int mshgnn_mlp_info_get(const mshgnn_mlp_plan* plan, mshgnn_mlp_info* info) {
    if (!plan || !info) return set_err(MSHGNN_EINVAL, "null argument to mshgnn_mlp_info_get");
    *info = plan->info;
    return MSHGNN_OK;
}
extern "C" size_t mshgnn_mlp_workspace_bytes(const mshgnn_mlp_plan* plan, int64_t batch, int training) {
    if (!plan || batch < 1 || batch > (1 << 24)) return 0;
    return mlp_layout(plan->d, plan->info.n_flat, batch, training != 0).total;
}
extern "C" size_t mshgnn_mlp_stash_offset(const mshgnn_mlp_plan* plan, int64_t batch, int layer) {
    if (!plan || batch < 1 || batch > (1 << 24) || layer < 1 || layer >= plan->d.num_layers) return 0;
    return mlp_layout(plan->d, plan->info.n_flat, batch, true).act[layer];
}

namespace {

// the caller's mshgnn_mlp_input, checked; fills the kernels' description of the rows and (series form) launches the run-pointer resolve
int mlp_prepare_input(const mshgnn_mlp_plan* p, const mshgnn_mlp_input* in, int64_t batch, bool want_labels, int loss_kind, const char* who, hipStream_t st,
                      MlpIn& mi, LabelArgs& lab, bool& series) {
    memset(&mi, 0, sizeof(mi)); memset(&lab, 0, sizeof(lab));
    mi.in = p->d.in_channels; mi.B = batch;
    series = in->x == nullptr;
    if (series && p->d.dtype == MSHGNN_BF16X3)
        return set_err(MSHGNN_EUNSUPPORTED, std::string(who) + ": the split plan has no series form; assemble the windows (fp32 rows) and use the dense form");
    if (!series) {
        const int need = (p->d.in_channels + 7) / 8 * 8;
        if (((uintptr_t)in->x & 15) || in->pitch % 8 || in->pitch < need)
            return set_err(MSHGNN_EINVAL, std::string(who) + ": dense rows must be 16-byte aligned at a pitch that is a multiple of 8 and >= in_channels rounded up to 8");
        mi.x = reinterpret_cast<const __bf16*>(in->x); mi.pitch = in->pitch;
        return MSHGNN_OK;
    }
    const mshgnn_window_desc* d = in->desc;
    if (!d || !in->src || !in->src_bf16 || !in->src_cstride || !in->src_rows || !in->starts || !in->run_ptrs)
        return set_err(MSHGNN_EINVAL, std::string("null argument to ") + who + " (series form)");
    if (d->dtype != MSHGNN_BF16 || !d->fast_layout || d->normalize || (d->sign_flags & 1) || desc_elements(d) > 1 || d->n_types != 1 || d->type_nodes[0] != 1 || d->n_rows != 1)
        return set_err(MSHGNN_EUNSUPPORTED, std::string(who) + ": the series form takes a bf16, fast_layout, unstandardised, unsigned recipe of one node type holding one node "
                                                                "and one group element; assemble the windows and use the dense form");
    if (d->type_width[0] != p->d.in_channels || d->history < 1 || d->n_runs < 1 || (int64_t)d->n_runs * d->history != p->d.in_channels || !d->runs)
        return set_err(MSHGNN_EINVAL, std::string(who) + ": the recipe's row is not in_channels wide (n_runs x history)");
    if (d->n_src < 1 || d->n_src > WIN_MAX_SRC) return set_err(MSHGNN_EINVAL, std::string(who) + ": bad number of source arrays");
    MlpSrc ms; memset(&ms, 0, sizeof(ms));
    for (int i = 0; i < d->n_src; ++i) {
        if (!in->src[i] || !in->src_bf16[i] || in->src_rows[i] < d->history || in->src_cstride[i] < in->src_rows[i] + 8 || in->src_rows[i] >= (1ll << 31))
            return set_err(MSHGNN_EINVAL, "bad source array (the gather needs cstride >= rows + 8)");
        ms.src16[i] = in->src_bf16[i]; ms.cstride[i] = in->src_cstride[i];
    }
    if (want_labels || in->y_out) {
        const bool ce = loss_kind == 1;
        if (!in->y_out || (ce && want_labels && !in->labels_out)) return set_err(MSHGNN_EINVAL, std::string(who) + ": the window labels need y_out (and labels_out for the cross entropy)");
        if (d->n_label < 1 || !d->label_cols || d->label_src < 0 || d->label_src >= d->n_src) return set_err(MSHGNN_EINVAL, "bad label description");
        if (d->label_rotate && (d->n_label % 3 != 0 || d->quat_src < 0 || d->quat_src >= d->n_src)) return set_err(MSHGNN_EINVAL, "label rotation needs 3-D labels and a quaternion source");
        if (in->labels_out && d->label_rotate) return set_err(MSHGNN_EINVAL, std::string(who) + ": contact labels are not rotated");
        if (want_labels && d->n_label != (ce ? p->d.out_channels / 2 : p->d.out_channels))
            return set_err(MSHGNN_EINVAL, std::string(who) + ": window recipe: label count differs from the model's targets");
        lab.lab = in->src[d->label_src]; lab.lab_cs = in->src_cstride[d->label_src];
        const bool q = d->quat_src >= 0 && d->quat_src < d->n_src && (in->quat_out || d->label_rotate);
        lab.quat_src = q ? in->src[d->quat_src] : nullptr; lab.quat_cs = q ? in->src_cstride[d->quat_src] : 0;
        lab.starts = in->starts; lab.B = batch; lab.T = d->history; lab.label_cols = d->label_cols; lab.n_label = d->n_label; lab.label_rotate = d->label_rotate;
        lab.y = in->y_out; lab.quat = in->quat_out; lab.labels_int = in->labels_out; lab.sign = 0;
    }
    if (!d->run_ptrs_ready)
        hipLaunchKernelGGL(k_mlp_run_ptrs, dim3((d->n_runs + 255) / 256), dim3(256), 0, st, d->runs, d->n_runs, ms, reinterpret_cast<unsigned long long*>(in->run_ptrs));
    mi.run_ptr = reinterpret_cast<const unsigned long long*>(in->run_ptrs); mi.starts = in->starts; mi.T = d->history;
    return MSHGNN_OK;
}

int mlp_run(const mshgnn_mlp_plan* p, const mshgnn_mlp_input* in, int mode, int loss_kind, const void* targets, const float* gout, const float* params, float* out,
            float* loss_out, float* grad, void* workspace, int64_t batch, void* stream, const char* who) {
    if (batch < 1 || batch > (1 << 24)) return set_err(MSHGNN_EINVAL, "batch must be in [1, 2^24]");
    if ((uintptr_t)workspace & 15) return set_err(MSHGNN_EINVAL, std::string(who) + ": the workspace must be 16-byte aligned");
    const mshgnn_mlp_desc& d = p->d;
    const mshgnn_mlp_info& info = p->info;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const bool training = mode != MODE_INFER, x3 = d.dtype == MSHGNN_BF16X3;
    const MlpWs w = mlp_layout(d, info.n_flat, batch, training);
    char* ws = reinterpret_cast<char*>(workspace);
    const int L = d.num_layers, H = d.hidden;
    const bool want_labels = mode == MODE_STEP && targets == nullptr;
    MlpIn mi; LabelArgs lab; bool series;
    if (mode == MODE_STEP && in->x != nullptr && !targets) return set_err(MSHGNN_EINVAL, std::string(who) + ": dense rows come with targets");
    if (int rc = mlp_prepare_input(p, in, batch, want_labels, loss_kind, who, st, mi, lab, series)) return rc;
    if (mode == MODE_BWD) lab.B = 0;      // (the forward gathered them)

    if (mode != MODE_BWD) {
        // weight pack
        PackArgs pa; memset(&pa, 0, sizeof(pa));
        int n = 0; int64_t tot = 0;
        auto region = [&](size_t dst, int rows, int cols, int layer /* 1-based */, int transposed) {
            PackRegion& g = pa.r[n];
            g.dst = reinterpret_cast<__bf16*>(ws + dst); g.src = info.off_w[layer - 1]; g.rows = rows; g.cols = cols;
            g.srows = out_f(d, layer - 1); g.scols = in_f(d, layer - 1); g.transposed = transposed;
            pa.prefix[n] = tot; tot += (int64_t)rows * cols; ++n;
        };
        region(w.w1p, H, w.K1p, 1, 0);
        for (int l = 2; l <= L; ++l) {
            region(w.wp[l], l == L ? MLP_OPAD : H, H, l, 0);
            if (training) region(w.wtp[l], H, l == L ? MLP_GK : H, l, 1);
        }
        pa.prefix[n] = tot; pa.n = n;
        if (x3) hipLaunchKernelGGL(k_mlp_pack_x3, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, pa, params);
        else hipLaunchKernelGGL(k_mlp_pack, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, pa, params);
        // input layer
        InArgs ia; memset(&ia, 0, sizeof(ia));
        ia.in = mi; ia.w1p = reinterpret_cast<const __bf16*>(ws + w.w1p); ia.K1p = w.K1p; ia.bias = params + info.off_b[0];
        ia.act1 = reinterpret_cast<__bf16*>(ws + w.act[1]); ia.H = H; ia.lab = lab;
        ia.lab_blocks = series ? (int)((lab.B + 255) / 256) : 0;
        const unsigned grid = (unsigned)(w.ntiles * (H / 128) + ia.lab_blocks);
        if (x3) hipLaunchKernelGGL(k_mlp_in_x3, dim3(grid), dim3(256), 0, st, ia);
        else if (series) hipLaunchKernelGGL(k_mlp_in<true>, dim3(grid), dim3(256), 0, st, ia);
        else hipLaunchKernelGGL(k_mlp_in<false>, dim3(grid), dim3(256), 0, st, ia);
    }
    // stack
    {
        StackArgs sa; memset(&sa, 0, sizeof(sa));
        sa.H = H; sa.out = d.out_channels; sa.L = L; sa.mode = mode; sa.loss_kind = loss_kind; sa.B = batch;
        const int64_t n_terms = loss_kind == 1 ? batch * (d.out_channels / 2) : batch * d.out_channels;
        sa.inv = 1.0f / (float)n_terms;
        sa.params = params;
        for (int l = 1; l <= L; ++l) {
            sa.off_b[l] = info.off_b[l - 1];
            sa.wp[l] = l >= 2 ? reinterpret_cast<const __bf16*>(ws + w.wp[l]) : nullptr;
            sa.wtp[l] = l >= 2 && training ? reinterpret_cast<const __bf16*>(ws + w.wtp[l]) : nullptr;
            sa.act[l] = l < L && (l == 1 || training) ? reinterpret_cast<__bf16*>(ws + w.act[l]) : nullptr;
            sa.dz[l] = training ? reinterpret_cast<__bf16*>(ws + w.dz[l]) : nullptr;
        }
        sa.out_p = out; sa.gout = gout;
        if (mode == MODE_STEP) {
            if (loss_kind == 0) sa.y = targets ? reinterpret_cast<const float*>(targets) : in->y_out;
            else sa.labels = targets ? reinterpret_cast<const int32_t*>(targets) : in->labels_out;
        }
        sa.loss_part = training ? reinterpret_cast<float*>(ws + w.loss_part) : nullptr;
        if (x3) hipLaunchKernelGGL(k_mlp_stack_x3, dim3((unsigned)w.ntiles), dim3(256), (size_t)info.lds_bytes, st, sa);
        else hipLaunchKernelGGL(k_mlp_stack, dim3((unsigned)w.ntiles), dim3(256), (size_t)info.lds_bytes, st, sa);
    }
    if (mode == MODE_STEP || mode == MODE_BWD) {
        WgArgs wa; memset(&wa, 0, sizeof(wa));
        wa.L = L; wa.H = H; wa.in = d.in_channels; wa.out = d.out_channels; wa.nslab = w.nslab; wa.B = batch; wa.slab_rows = w.slab_rows; wa.n_flat = info.n_flat;
        int tot = 0;
        for (int l = 1; l <= L; ++l) {
            const int Jd = out_f(d, l - 1), Id = in_f(d, l - 1);
            wa.prefix[l] = tot; wa.itiles[l] = (Id + WG_T - 1) / WG_T;
            tot += wa.itiles[l] * ((Jd + WG_T - 1) / WG_T);
            wa.dz[l] = reinterpret_cast<const __bf16*>(ws + w.dz[l]);
            wa.act[l] = l < L ? reinterpret_cast<const __bf16*>(ws + w.act[l]) : nullptr;
            wa.off_w[l] = info.off_w[l - 1]; wa.off_b[l] = info.off_b[l - 1];
        }
        wa.prefix[L + 1] = tot;
        wa.slabs = reinterpret_cast<float*>(ws + w.slabs); wa.xin = mi;
        const unsigned grid = (unsigned)tot * (unsigned)w.nslab;
        if (x3) hipLaunchKernelGGL(k_mlp_wgrad_x3, dim3(grid), dim3(256), 0, st, wa);
        else if (series) hipLaunchKernelGGL(k_mlp_wgrad<true>, dim3(grid), dim3(256), 0, st, wa);
        else hipLaunchKernelGGL(k_mlp_wgrad<false>, dim3(grid), dim3(256), 0, st, wa);
        const int grad_blocks = (int)((info.n_flat + 255) / 256);
        const bool with_loss = mode == MODE_STEP;
        const int64_t n_terms = loss_kind == 1 ? batch * (d.out_channels / 2) : batch * d.out_channels;
        hipLaunchKernelGGL(k_mlp_reduce, dim3((unsigned)(grad_blocks + (with_loss ? 1 : 0))), dim3(256), 0, st, wa.slabs, w.nslab, info.n_flat, grad, grad_blocks,
                           reinterpret_cast<const float*>(ws + w.loss_part), w.ntiles, (float)n_terms, loss_out);
    }
    HIPCHK(hipGetLastError());
    return MSHGNN_OK;
}

}  // namespace

extern "C" int mshgnn_mlp_forward(const mshgnn_mlp_plan* plan, const mshgnn_mlp_input* input, const float* params, float* out, void* workspace, int64_t batch,
                                  int training, void* stream) {
    if (!plan || !input || !params || !out || !workspace) return set_err(MSHGNN_EINVAL, "null argument to mshgnn_mlp_forward");
    return mlp_run(plan, input, training ? MODE_TRAIN_FWD : MODE_INFER, -1, nullptr, nullptr, params, out, nullptr, nullptr, workspace, batch, stream, "mshgnn_mlp_forward");
}
extern "C" int mshgnn_mlp_backward(const mshgnn_mlp_plan* plan, const mshgnn_mlp_input* input, const float* params, const float* gout, float* grad_params,
                                   void* workspace, int64_t batch, void* stream) {
    if (!plan || !input || !params || !gout || !grad_params || !workspace) return set_err(MSHGNN_EINVAL, "null argument to mshgnn_mlp_backward");
    return mlp_run(plan, input, MODE_BWD, -1, nullptr, gout, params, nullptr, nullptr, grad_params, workspace, batch, stream, "mshgnn_mlp_backward");
}
extern "C" int mshgnn_mlp_step(const mshgnn_mlp_plan* plan, const mshgnn_mlp_input* input, int loss_kind, const void* targets, const float* params, float* out,
                               float* loss_out, float* grad_params, void* workspace, int64_t batch, void* stream) {
    if (!plan || !input || !params || !out || !loss_out || !grad_params || !workspace) return set_err(MSHGNN_EINVAL, "null argument to mshgnn_mlp_step");
    if (loss_kind != 0 && loss_kind != 1) return set_err(MSHGNN_EINVAL, "mshgnn_mlp_step: loss_kind must be 0 (MSE) or 1 (cross entropy)");
    if (int rc = mlp_check_desc(&plan->d, loss_kind, "mshgnn_mlp_step")) return rc;
    return mlp_run(plan, input, MODE_STEP, loss_kind, targets, nullptr, params, out, loss_out, grad_params, workspace, batch, stream, "mshgnn_mlp_step");
}
