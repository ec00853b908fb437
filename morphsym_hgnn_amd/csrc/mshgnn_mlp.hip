// MLP baselines (include/mshgnn.h, "MLP baselines"): y = W_L relu(... relu(W_1 x + b_1) ...) + b_L, the reference's nn.Sequential (gnnLightning.py:391-405),
// on bf16 MFMA operands with fp32 accumulation.  Launches of one step, all on the caller's stream; every kernel that touches an operand is one template over the
// plan (<X3>: false the bf16 plan, true the split plan below; <X3, SERIES> where the batch's rows are read), so a kernel trace shows k_mlp_stack<true> next to
// k_mlp_stack<false>:
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
// Split plan (dtype MSHGNN_BF16X3, the arithmetic of mshgnn_x3.hip): the same kernels at X3 = true, with every operand of a product as hi = bf16(v),
// lo = bf16(v - hi) and every product as hi hi + lo hi + hi lo (the lo half of the weight, or of dZ in the weight gradient, first), fp32 accumulation.  X: dense
// fp32 rows, split in registers while they are staged (no series form: <true, true> is never instantiated).  Every packed weight region is a hi image followed
// by a lo image; every stash and dZ row is [hi | lo] (A_l, dZ_l: 2 H bf16, dZ_L: 2 x 16).  Rounding points: the second rounding (lo) of X, every weight, A_l and
// dZ_l; the ReLU mask of the backward sweep is [hi > 0].
// What differs between the plans lives in four primitives: mlp_fetch8 (8 K elements of a row as NP octs), mlp_store4 / mlp_store2 (values rounded to one quad or
// pair, or to the hi and the lo one), mlp_mma (one MFMA, or the three); the kernel bodies name the plan only in strides written NP * ... and, in k_mlp_in, in the
// spelling of one statement (see there).
#include <algorithm>
#include <new>
#include <type_traits>

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

// ---- the plan's primitives: every kernel below is one template over the plan (X3: the split plan) and reads the same for both; NP operands per product ----
template <bool X3> constexpr int mlp_np = X3 ? 2 : 1;      // planes per operand: hi alone, or hi and lo
template <int NP> struct Octs { u32x4 v[NP]; };             // 8 K elements of one operand, per plane

__device__ __forceinline__ u32x2 pack4_bf16(f32x4 v) {
    union { u32x2 r; __bf16 e[4]; } u;
#pragma unroll
    for (int i = 0; i < 4; ++i) u.e[i] = (__bf16)v[i];
    return u.r;
}
__device__ __forceinline__ f32x4 widen4_bf16(u32x2 r) {
    return f32x4{__builtin_bit_cast(float, r[0] << 16), __builtin_bit_cast(float, r[0] & 0xffff0000u), __builtin_bit_cast(float, r[1] << 16), __builtin_bit_cast(float, r[1] & 0xffff0000u)};
}
// four consecutive values rounded to bf16 at dst; split plan: the hi quad there and the lo quad (split_oct of mshgnn_device.hpp on four values) `lo_off` elements
// further -- H in the rows of a stash, the plane stride in LDS
template <int NP> __device__ __forceinline__ void mlp_store4(__bf16* dst, size_t lo_off, f32x4 v) {
    const u32x2 hi = pack4_bf16(v);
    *reinterpret_cast<u32x2*>(dst) = hi;
    if constexpr (NP == 2) *reinterpret_cast<u32x2*>(dst + lo_off) = pack4_bf16(v - widen4_bf16(hi));
}
template <int NP> __device__ __forceinline__ void mlp_store2(__bf16* dst, size_t lo_off, float v0, float v1) {      // the same for a pair
    union { unsigned u; __bf16 e[2]; } hi;
    hi.e[0] = (__bf16)v0; hi.e[1] = (__bf16)v1;
    *reinterpret_cast<unsigned*>(dst) = hi.u;
    if constexpr (NP == 2) {
        union { unsigned u; __bf16 e[2]; } lo;
        lo.e[0] = (__bf16)(v0 - (float)hi.e[0]); lo.e[1] = (__bf16)(v1 - (float)hi.e[1]);
        *reinterpret_cast<unsigned*>(dst + lo_off) = lo.u;
    }
}
__device__ __forceinline__ f32x4 mfma_bf16(u32x4 a, u32x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
// c += w x over one K step (w: the weight, or dZ in the weight gradient); split plan: w_hi x_hi, then w_lo x_hi, then w_hi x_lo
template <int NP> __device__ __forceinline__ f32x4 mlp_mma(const u32x4 (&w)[NP], const u32x4 (&x)[NP], f32x4 c) {
    c = mfma_bf16(w[0], x[0], c);
    if constexpr (NP == 2) { c = mfma_bf16(w[1], x[0], c); c = mfma_bf16(w[0], x[1], c); }
    return c;
}

// ---- the batch's rows: dense rows (bf16; split plan: fp32, split in registers while they are staged), or windows of the resident bf16 series ----
struct MlpIn {
    const void* x; int64_t pitch;                                     // dense: bf16 rows, or fp32 rows on the split plan (pitch in elements of either)
    const unsigned long long* run_ptr; const int64_t* starts; int T;  // series
    int in; int64_t B;
};
template <bool X3> struct RowRef { const std::conditional_t<X3, float, __bf16>* p; int64_t s; };
template <bool X3, bool SERIES> __device__ __forceinline__ RowRef<X3> mlp_row(const MlpIn& a, int64_t b) {      // b < B
    static_assert(!(X3 && SERIES), "the split plan has no series form (the host refuses it): X3 && SERIES is never instantiated");
    RowRef<X3> r; r.p = nullptr; r.s = 0;
    if constexpr (SERIES) r.s = a.starts[b]; else r.p = static_cast<decltype(r.p)>(a.x) + b * a.pitch;
    return r;
}
// elements [k0, k0 + 8) of a row as 8 bf16 per plane (k0 a multiple of 8); elements at or beyond `in` are zeros, whatever the pad columns hold
template <bool X3, bool SERIES> __device__ __forceinline__ Octs<mlp_np<X3>> mlp_fetch8(const MlpIn& a, const RowRef<X3>& r, int k0) {
    const int nvalid = a.in - k0;
    if constexpr (X3) {
        Octs<2> o;
        f32x4 q0 = f32x4{0.f, 0.f, 0.f, 0.f}, q1 = q0;
        if (nvalid > 0) {      // (the pitch covers `in` rounded up to 8: both loads stay inside the row)
            q0 = load_quad(r.p + k0); q1 = load_quad(r.p + k0 + 4);
            if (nvalid < 8) {
#pragma unroll
                for (int i = 0; i < 4; ++i) { if (i >= nvalid) q0[i] = 0.f; if (4 + i >= nvalid) q1[i] = 0.f; }
            }
        }
        split_oct(q0, q1, o.v[0], o.v[1]);
        return o;
    } else {
        u32x4 v = u32x4{0, 0, 0, 0};
        if (nvalid <= 0) return Octs<1>{{v}};
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
        return Octs<1>{{v}};
    }
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
template <bool X3> __global__ __launch_bounds__(256) void k_mlp_pack(PackArgs a, const float* params) {
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
    if constexpr (X3) g.dst[(int64_t)g.rows * g.cols + local] = (__bf16)(v - (float)hi);      // the lo image, behind the hi image [rows][cols]
}

// ---- input layer ----
struct InArgs {
    MlpIn in; const __bf16* w1p; int K1p; const float* bias; __bf16* act1; int H; int lab_blocks; LabelArgs lab;
};
// K steps per trip of the input layer's K loop, their loads issued together.  bf16, four: a step's gather is two dependent round trips (run pointer, then the
// series), and one step per trip left the launch waiting on 254 of them in a row at K = 8100.  Split plan, two: the fp32 rows and both weight images of four
// steps would not fit the registers of two waves per SIMD.  (K1p is a multiple of 128: the pack's zero columns and mlp_fetch8's zeros fill the last trip)
template <bool X3> constexpr int mlp_in_steps = X3 ? 2 : 4;
template <bool X3, bool SERIES> __global__ __launch_bounds__(256) void k_mlp_in(InArgs a) {
    constexpr int NP = mlp_np<X3>, NU = mlp_in_steps<X3>;
    const int tid = threadIdx.x;
    if constexpr (SERIES) {
        if ((int)blockIdx.x < a.lab_blocks) {
            const int64_t b = (int64_t)blockIdx.x * 256 + tid;
            if (b < a.lab.B) window_labels_one<false>(a.lab, b);
            return;
        }
    }
    const unsigned bid = blockIdx.x - (SERIES ? a.lab_blocks : 0);
    const int nh = a.H / 128;
    const int64_t tile = bid / nh; const int hc = (int)(bid - (unsigned)tile * nh);
    const int wave = tid >> 6, lane = tid & 63, g = lane >> 4, c = lane & 15;
    const int n0 = hc * 128 + wave * 32;
    const int64_t b0 = tile * MLP_TILE;
    RowRef<X3> rr[2];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) rr[rb] = mlp_row<X3, SERIES>(a.in, min(b0 + rb * 16 + c, a.in.B - 1));
    f32x4 acc[2][2];
#pragma unroll
    for (int fb = 0; fb < 2; ++fb)
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) acc[fb][rb] = f32x4{0.f, 0.f, 0.f, 0.f};
    const size_t wimg = (size_t)a.H * a.K1p;      // one image of W_1
    const __bf16* wr[2];
    wr[0] = a.w1p + (size_t)(n0 + c) * a.K1p + 8 * g; wr[1] = wr[0] + (size_t)16 * a.K1p;
    for (int ks = 0; ks < a.K1p; ks += 32 * NU) {
        Octs<NP> x[NU][2], w[NU][2];
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int k0 = ks + 32 * u + 8 * g;
            // The one statement spelled per plan, for the compiler alone: the two row blocks' fetches written out (bf16) or as a loop (split plan).  Either
            // spelling costs the other plan about twenty instructions per trip in this latency-bound loop, 1 - 2 % of the launch ("One template").
            if constexpr (X3) {
#pragma unroll
                for (int rb = 0; rb < 2; ++rb) x[u][rb] = mlp_fetch8<X3, SERIES>(a.in, rr[rb], k0);
            } else { x[u][0] = mlp_fetch8<X3, SERIES>(a.in, rr[0], k0); x[u][1] = mlp_fetch8<X3, SERIES>(a.in, rr[1], k0); }
#pragma unroll
            for (int fb = 0; fb < 2; ++fb)
#pragma unroll
                for (int h = 0; h < NP; ++h) w[u][fb].v[h] = *reinterpret_cast<const u32x4*>(wr[fb] + h * wimg + ks + 32 * u);
        }
#pragma unroll
        for (int u = 0; u < NU; ++u)
#pragma unroll
            for (int fb = 0; fb < 2; ++fb)
#pragma unroll
                for (int rb = 0; rb < 2; ++rb) acc[fb][rb] = mlp_mma<NP>(w[u][fb].v, x[u][rb].v, acc[fb][rb]);
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
            mlp_store4<NP>(a.act1 + (size_t)b * (NP * a.H) + f, a.H, v);
        }
    }
}

// ---- stack ----
struct StackArgs {
    int H, out, L, mode, loss_kind; int64_t B; float inv;
    int reg_kind; float reg_delta;      // loss_kind 0: the plan's regression loss when the call was made (MSHGNN_REG_LOSS_*; 0 = MSE) and Huber's delta
    const float* params; int64_t off_b[MLP_MAXL + 1];      // bias of layer l = 1 .. L
    const __bf16* wp[MLP_MAXL + 1]; const __bf16* wtp[MLP_MAXL + 1]; __bf16* act[MLP_MAXL + 1]; __bf16* dz[MLP_MAXL + 1];
    float* out_p; const float* y; const int32_t* labels; const float* gout; float* loss_part;
};
// D[n][row] = sum_k W[n][k] X[row][k] over the tile's 32 rows: W global bf16 [N][Kw] (N a multiple of 16, Kw of 32), X in LDS at stride xs; split plan: the lo
// image of W behind its hi image, the lo plane of X `plane` elements behind its hi plane.
// epi(first of 4 consecutive features, row in the tile, the 4 sums); the (feature, row) -> thread map depends on N alone.
template <int NP, typename Epi> __device__ __forceinline__ void mlp_layer(const __bf16* W, int N, int Kw, const __bf16* X, int xs, int plane, int wave, int lane, Epi epi) {
    const int g = lane >> 4, c = lane & 15;
    const size_t wimg = (size_t)N * Kw;
    for (int fb = wave; fb < N / 16; fb += 4) {
        f32x4 a0 = f32x4{0.f, 0.f, 0.f, 0.f}, a1 = a0;
        const __bf16* wr = W + (size_t)(fb * 16 + c) * Kw + 8 * g;
        const __bf16* x0 = X + c * xs + 8 * g;
        const __bf16* x1 = x0 + 16 * xs;
        for (int k = 0; k < Kw; k += 32) {
            u32x4 wf[NP], f0[NP], f1[NP];
#pragma unroll
            for (int h = 0; h < NP; ++h) {
                wf[h] = *reinterpret_cast<const u32x4*>(wr + h * wimg + k);
                f0[h] = *reinterpret_cast<const u32x4*>(x0 + h * plane + k); f1[h] = *reinterpret_cast<const u32x4*>(x1 + h * plane + k);
            }
            a0 = mlp_mma<NP>(wf, f0, a0); a1 = mlp_mma<NP>(wf, f1, a1);
        }
        epi(fb * 16 + 4 * g, c, a0); epi(fb * 16 + 4 * g, 16 + c, a1);
    }
}

// LDS: two activation buffers of NP planes [32][H + 8] each (a row shifts the 16-byte reads of a lane group by four banks; the planes are read by separate
// instructions, so the plane stride adds no conflict), then the output and reduction buffers.  Rows of the stashes and of dZ: NP halves, [hi | lo].
template <bool X3> __global__ __launch_bounds__(256) void k_mlp_stack(StackArgs a) {
    constexpr int NP = mlp_np<X3>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int H = a.H, xs = H + 8, L = a.L, plane = MLP_TILE * xs;
    __bf16* buf0 = reinterpret_cast<__bf16*>(smem);
    __bf16* buf1 = buf0 + NP * plane;
    float* obuf = reinterpret_cast<float*>(buf1 + NP * plane);
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
#pragma unroll
            for (int h = 0; h < NP; ++h)
                *reinterpret_cast<u32x4*>(cur + h * plane + row * xs + ch * 8) = *reinterpret_cast<const u32x4*>(a.act[1] + (size_t)(b0 + row) * (NP * H) + h * H + ch * 8);
        }
        __syncthreads();
        for (int l = 2; l < L; ++l) {
            const float* bias = a.params + a.off_b[l];
            __bf16* st = a.act[l];
            mlp_layer<NP>(a.wp[l], H, H, cur, xs, plane, wave, lane, [&](int f, int row, f32x4 s) {
                const bool live = b0 + row < a.B;
                f32x4 v;
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = live ? fmaxf(s[i] + bias[f + i], 0.f) : 0.f;
                mlp_store4<NP>(nxt + row * xs + f, plane, v);
                if (stash) mlp_store4<NP>(st + (size_t)(b0 + row) * (NP * H) + f, H, v);
            });
            __syncthreads();
            __bf16* t = cur; cur = nxt; nxt = t;
        }
        {
            const float* bias = a.params + a.off_b[L];
            mlp_layer<NP>(a.wp[L], MLP_OPAD, H, cur, xs, plane, wave, lane, [&](int f, int row, f32x4 s) {
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
                if (a.loss_kind == 0 && a.reg_kind == MSHGNN_REG_LOSS_MSE) {
                    if (f0 < a.out) { const float d = o0 - a.y[(size_t)b * a.out + f0]; g0 = 2.0f * d * a.inv; term = d * d; }
                    if (f0 + 1 < a.out) { const float d = o1 - a.y[(size_t)b * a.out + f0 + 1]; g1 = 2.0f * d * a.inv; term += d * d; }
                } else if (a.loss_kind == 0) {      // L1 / Huber: the plan's regression loss (reg_loss_terms, mshgnn_device.hpp)
                    float t1 = 0.f;
                    if (f0 < a.out) reg_loss_terms(o0 - a.y[(size_t)b * a.out + f0], a.inv, a.reg_kind, a.reg_delta, g0, term);
                    if (f0 + 1 < a.out) { reg_loss_terms(o1 - a.y[(size_t)b * a.out + f0 + 1], a.inv, a.reg_kind, a.reg_delta, g1, t1); term += t1; }
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
        mlp_store2<NP>(nxt + row * xs + f0, plane, g0, g1);
        mlp_store2<NP>(nxt + row * xs + MLP_OPAD + f0, plane, 0.f, 0.f);      // K columns 16 .. 31 of the first backward product
        mlp_store2<NP>(a.dz[L] + (size_t)b * (NP * MLP_OPAD) + f0, MLP_OPAD, g0, g1);
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
        mlp_layer<NP>(a.wtp[l], H, Kw, cur, xs, plane, wave, lane, [&](int f, int row, f32x4 s) {
            const f32x4 av = load_quad(am + (size_t)(b0 + row) * (NP * H) + f);
            f32x4 v;
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = av[i] > 0.f ? s[i] : 0.f;
            mlp_store4<NP>(nxt + row * xs + f, plane, v);
            mlp_store4<NP>(dzo + (size_t)(b0 + row) * (NP * H) + f, H, v);
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
// LDS: NP planes of 4352 B per operand; per block of the tile dZ A over the step's rows (mlp_mma); db = the column sums of dZ (split plan: of hi + lo, exact in
// fp32) in row order; layer 1's A operand is the batch's rows, fetched as k_mlp_in fetched them
template <bool X3, bool SERIES> __global__ __launch_bounds__(256) void k_mlp_wgrad(WgArgs a) {
    constexpr int NP = mlp_np<X3>;
    __shared__ __attribute__((aligned(16))) __bf16 sdz[NP][MLP_TILE * WG_LD];
    __shared__ __attribute__((aligned(16))) __bf16 sx[NP][MLP_TILE * WG_LD];
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
        Octs<NP> vz, vx;
#pragma unroll
        for (int h = 0; h < NP; ++h) vz.v[h] = vx.v[h] = u32x4{0, 0, 0, 0};
        if (b < r1) {
            if (jcol < zs) {
#pragma unroll
                for (int h = 0; h < NP; ++h) vz.v[h] = *reinterpret_cast<const u32x4*>(dz + (size_t)b * (NP * zs) + h * zs + jcol);
            }
            if (l == 1) vx = mlp_fetch8<X3, SERIES>(a.xin, mlp_row<X3, SERIES>(a.xin, b), icol);
            else if (icol < a.H) {
#pragma unroll
                for (int h = 0; h < NP; ++h) vx.v[h] = *reinterpret_cast<const u32x4*>(ap + (size_t)b * (NP * a.H) + h * a.H + icol);
            }
        }
        __syncthreads();      // the previous step's reads are done
#pragma unroll
        for (int h = 0; h < NP; ++h) {
            *reinterpret_cast<u32x2*>(sdz[h] + srow * WG_LD + ch * 8) = u32x2{vz.v[h][0], vz.v[h][1]};
            *reinterpret_cast<u32x2*>(sdz[h] + srow * WG_LD + ch * 8 + 4) = u32x2{vz.v[h][2], vz.v[h][3]};
            *reinterpret_cast<u32x2*>(sx[h] + srow * WG_LD + ch * 8) = u32x2{vx.v[h][0], vx.v[h][1]};
            *reinterpret_cast<u32x2*>(sx[h] + srow * WG_LD + ch * 8 + 4) = u32x2{vx.v[h][2], vx.v[h][3]};
        }
        __syncthreads();
        // operands of the row-reduction: element e of lane group g is row 8 g + e of the step
        u32x4 zf[NP];
#pragma unroll
        for (int h = 0; h < NP; ++h) {
            const unsigned short* zz = reinterpret_cast<const unsigned short*>(sdz[h]) + (8 * g) * WG_LD + wave * 16 + c;
#pragma unroll
            for (int q = 0; q < 4; ++q) zf[h][q] = (unsigned)zz[(2 * q) * WG_LD] | ((unsigned)zz[(2 * q + 1) * WG_LD] << 16);
        }
#pragma unroll
        for (int ib = 0; ib < 4; ++ib) {
            u32x4 xf[NP];
#pragma unroll
            for (int h = 0; h < NP; ++h) {
                const unsigned short* xx = reinterpret_cast<const unsigned short*>(sx[h]) + (8 * g) * WG_LD + ib * 16 + c;
#pragma unroll
                for (int q = 0; q < 4; ++q) xf[h][q] = (unsigned)xx[(2 * q) * WG_LD] | ((unsigned)xx[(2 * q + 1) * WG_LD] << 16);
            }
            acc[ib] = mlp_mma<NP>(zf, xf, acc[ib]);
        }
        if (it == 0 && tid < WG_T) {
#pragma unroll 8
            for (int rw = 0; rw < MLP_TILE; ++rw) {
                float z = (float)sdz[0][rw * WG_LD + tid];
#pragma unroll
                for (int h = 1; h < NP; ++h) z += (float)sdz[h][rw * WG_LD + tid];
                bsum += z;
            }
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

// the kernels of a plan, chosen once where the plan is created; [series]
struct MlpKernels { void (*pack)(PackArgs, const float*); void (*in[2])(InArgs); void (*stack)(StackArgs); void (*wgrad[2])(WgArgs); };
const MlpKernels MLP_BF16 = {k_mlp_pack<false>, {k_mlp_in<false, false>, k_mlp_in<false, true>}, k_mlp_stack<false>, {k_mlp_wgrad<false, false>, k_mlp_wgrad<false, true>}};
const MlpKernels MLP_X3 = {k_mlp_pack<true>, {k_mlp_in<true, false>, nullptr}, k_mlp_stack<true>, {k_mlp_wgrad<true, false>, nullptr}};      // (no series form: mlp_prepare_input refuses it)

}  // namespace

struct mshgnn_mlp_plan { mshgnn_mlp_desc d; mshgnn_mlp_info info; const MlpKernels* k; int reg_kind = MSHGNN_REG_LOSS_MSE; float reg_delta = 1.0f; };      // reg_*: what mshgnn_mlp_step(loss_kind 0) computes

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
    p->k = desc->dtype == MSHGNN_BF16X3 ? &MLP_X3 : &MLP_BF16;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(p->k->stack), hipFuncAttributeMaxDynamicSharedMemorySize, (int)p->info.lds_bytes);
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
        mi.x = in->x; mi.pitch = in->pitch;
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
    const MlpKernels& k = *p->k;
    const bool training = mode != MODE_INFER;
    const int64_t n_terms = loss_kind == 1 ? batch * (d.out_channels / 2) : batch * d.out_channels;
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
        hipLaunchKernelGGL(k.pack, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, pa, params);
        // input layer
        InArgs ia; memset(&ia, 0, sizeof(ia));
        ia.in = mi; ia.w1p = reinterpret_cast<const __bf16*>(ws + w.w1p); ia.K1p = w.K1p; ia.bias = params + info.off_b[0];
        ia.act1 = reinterpret_cast<__bf16*>(ws + w.act[1]); ia.H = H; ia.lab = lab;
        ia.lab_blocks = series ? (int)((lab.B + 255) / 256) : 0;
        const unsigned grid = (unsigned)(w.ntiles * (H / 128) + ia.lab_blocks);
        hipLaunchKernelGGL(k.in[series], dim3(grid), dim3(256), 0, st, ia);
    }
    // stack
    {
        StackArgs sa; memset(&sa, 0, sizeof(sa));
        sa.H = H; sa.out = d.out_channels; sa.L = L; sa.mode = mode; sa.loss_kind = loss_kind; sa.B = batch;
        if (mode == MODE_STEP && loss_kind == 0) { sa.reg_kind = p->reg_kind; sa.reg_delta = p->reg_delta; }      // (read now, by value: a captured graph keeps it)
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
        hipLaunchKernelGGL(k.stack, dim3((unsigned)w.ntiles), dim3(256), (size_t)info.lds_bytes, st, sa);
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
        hipLaunchKernelGGL(k.wgrad[series], dim3(grid), dim3(256), 0, st, wa);
        const int grad_blocks = (int)((info.n_flat + 255) / 256);
        const bool with_loss = mode == MODE_STEP;
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
extern "C" int mshgnn_mlp_set_regression_loss(mshgnn_mlp_plan* plan, int kind, float delta) {
    if (!plan) return set_err(MSHGNN_EINVAL, "null argument to mshgnn_mlp_set_regression_loss");
    if (const int rc = check_regression_loss(kind, delta, "mshgnn_mlp_set_regression_loss")) return rc;
    plan->reg_kind = kind; plan->reg_delta = kind == MSHGNN_REG_LOSS_HUBER ? delta : 1.0f;
    return MSHGNN_OK;
}
extern "C" int mshgnn_mlp_get_regression_loss(const mshgnn_mlp_plan* plan, int32_t* kind_out, float* delta_out) {
    if (!plan || !kind_out || !delta_out) return set_err(MSHGNN_EINVAL, "null argument to mshgnn_mlp_get_regression_loss");
    *kind_out = plan->reg_kind; *delta_out = plan->reg_delta;
    return MSHGNN_OK;
}

extern "C" int mshgnn_mlp_step(const mshgnn_mlp_plan* plan, const mshgnn_mlp_input* input, int loss_kind, const void* targets, const float* params, float* out,
                               float* loss_out, float* grad_params, void* workspace, int64_t batch, void* stream) {
    if (!plan || !input || !params || !out || !loss_out || !grad_params || !workspace) return set_err(MSHGNN_EINVAL, "null argument to mshgnn_mlp_step");
    if (loss_kind != 0 && loss_kind != 1) return set_err(MSHGNN_EINVAL, "mshgnn_mlp_step: loss_kind must be 0 (MSE) or 1 (cross entropy)");
    if (int rc = mlp_check_desc(&plan->d, loss_kind, "mshgnn_mlp_step")) return rc;
    return mlp_run(plan, input, MODE_STEP, loss_kind, targets, nullptr, params, out, loss_out, grad_params, workspace, batch, stream, "mshgnn_mlp_step");
}
