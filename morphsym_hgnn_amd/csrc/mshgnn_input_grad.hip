// Gradients with respect to the model's INPUTS (mshgnn_input_grad, include/mshgnn.h).
//
// The encoder is y = W_enc[t] (m_t . x) + b per node of type t (m_t: the +-1 symmetry mask, apply_symmetry hgnn_c2.py:191-231), so
//     dx[w, node i of type t, f] = m_t[i, f] . sum_j dY_enc[node][w][j] W_enc[t][j][f]
// where dY_enc = relu'(X_0) . (G_1 + D_0) is what the layer-0 backward group leaves in the workspace's dX_0 stash -- the P operand the encoder's
// weight-gradient items read (mshgnn_plan.hpp, GF_ENC_MASK; the generic engine's layer-0 jobs carry JF_GATE_BITS and store the gated row alike).
// Nodes the encoder does not compute (their rows cannot reach the output at this depth) get exact zeros: what the reference's autograd gives them.
// Which (node, sign offset) pairs exist is read from the plan's own encoder weight-gradient items, never recomputed here.
//
// One launch writes dx for every requested type.  Workgroup = 4 waves = (type, 16..64-column chunk of the caller's row pitch, a run of 16-window
// row tiles of one node at a time).  The column chunk of W_enc[t] (all K = hidden rows) is converted once into the plan's operand form and kept in
// LDS as [column][k]; a wave then streams 16-window tiles of dY_enc rows and multiplies D[f][w] = W^T[f][:] . dY^T[:][w] on the MFMA:
//   f32  plan: v_mfma_f32_16x16x4_f32 on fp32 rows
//   bf16 plan: v_mfma_f32_16x16x32_bf16, bf16 W (round to nearest even), fp32 accumulation
//   split plan (and the generic engine's split arithmetic): rows [hi | lo], W as hi + lo bf16, hi.hi + lo.hi + hi.lo, fp32 accumulation
// Every output element is one full K sum inside one wave (no atomics, no cross-workgroup sums): two runs give the same bits.
// The output is written in the caller's dtype (fp32 or fp64) at the caller's pitch; pad columns and rows of nodes the plan does not compute are 0.
#include <mutex>
#include "mshgnn_device.hpp"
#include "mshgnn_gen_plan.hpp"

using namespace mshgnn;

namespace {

struct IgType {
    const float* w;      // W_enc[t]: [K][F] fp32 in the flat parameter buffer
    void* dx;            // caller's gradient rows [batch * n][pitch]
    int64_t pitch;
    int F, n, ncc, rgs, blk0, node0, vec;      // ncc: column chunks, rgs: row-tile groups, blk0: first workgroup, node0: first entry of this type in the node table, vec: 16-byte stores
};
struct IgArgs {
    const char* dy;      // dX_0 stash (dY_enc): row (node, w) at element (node * B + w) * dy_row
    int64_t dy_row;
    const int* nodes;    // per (type, node i): {plan node, sign offset | -1: not computed}
    const uint8_t* signs;
    int K, B, nwb, CW, tpb, n_req;
    IgType ty[MSHGNN_MAX_TYPES];
};

enum { IG_F32 = 0, IG_BF16 = 1, IG_X3 = 2 };

__device__ __forceinline__ unsigned short bf16_rne(float v) {
    unsigned u = __builtin_bit_cast(unsigned, v);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (unsigned short)(u >> 16);
}

template <int MODE> constexpr int ig_kpad() { return MODE == IG_F32 ? 4 : 8; }

template <int MODE, typename OT> __global__ __launch_bounds__(256) void k_input_grad(IgArgs a) {
    extern __shared__ __align__(16) char smem[];
    int q = 0;
#pragma unroll
    for (int r = 1; r < MSHGNN_MAX_TYPES; ++r) if (r < a.n_req && (int)blockIdx.x >= a.ty[r].blk0) q = r;
    const float* W = a.ty[q].w;
    OT* dx = reinterpret_cast<OT*>(a.ty[q].dx);
    const int64_t pitch = a.ty[q].pitch;
    const int F = a.ty[q].F, n = a.ty[q].n, ncc = a.ty[q].ncc, node0 = a.ty[q].node0, vec = a.ty[q].vec;
    const int local = (int)blockIdx.x - a.ty[q].blk0, rg = local / ncc, cc = local % ncc;
    const int K = a.K, CW = a.CW, KP = K + ig_kpad<MODE>(), c0 = cc * CW;

    // W_enc[t][:, c0 .. c0 + CW) -> LDS [column][k] in the plan's operand form (columns past F: zero)
    for (int e = threadIdx.x; e < K * CW; e += 256) {
        const int k = e / CW, c = e - k * CW, f = c0 + c;
        const float v = f < F ? W[(size_t)k * F + f] : 0.f;
        if constexpr (MODE == IG_F32) {
            reinterpret_cast<float*>(smem)[c * KP + k] = v;
        } else {
            const unsigned short hi = bf16_rne(v);
            reinterpret_cast<unsigned short*>(smem)[c * KP + k] = hi;
            if constexpr (MODE == IG_X3)
                reinterpret_cast<unsigned short*>(smem)[(CW + c) * KP + k] = bf16_rne(v - __builtin_bit_cast(float, (unsigned)hi << 16));
        }
    }
    __syncthreads();

    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, l16 = lane & 15, g = lane >> 4;
    const int NCT = CW >> 4;
    const int t_end = min(n * a.nwb, (rg + 1) * a.tpb);
    for (int tile = rg * a.tpb + wv; tile < t_end; tile += 4) {
        const int i = tile / a.nwb, wb = tile - i * a.nwb;
        const int gnode = a.nodes[2 * (node0 + i)], sb = a.nodes[2 * (node0 + i) + 1];
        const int w = wb * 16 + l16;
        f32x4 acc[4];
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (sb >= 0) {
            for (int kc = 0; kc < K; kc += 128) {
                if constexpr (MODE == IG_F32) {
                    const float* row = reinterpret_cast<const float*>(a.dy) + ((size_t)gnode * a.B + w) * a.dy_row + kc + 4 * g;
                    f32x4 bq[8];
#pragma unroll
                    for (int s = 0; s < 8; ++s) bq[s] = w < a.B ? *reinterpret_cast<const f32x4*>(row + 16 * s) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int ct = 0; ct < 4; ++ct) {
                        if (ct >= NCT) break;
                        const float* wl = reinterpret_cast<const float*>(smem) + (ct * 16 + l16) * KP + kc + 4 * g;
#pragma unroll
                        for (int s = 0; s < 8; ++s) {
                            const f32x4 av = *reinterpret_cast<const f32x4*>(wl + 16 * s);
#pragma unroll
                            for (int e = 0; e < 4; ++e) acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e], bq[s][e], acc[ct], 0, 0, 0);
                        }
                    }
                } else {
                    const unsigned short* row = reinterpret_cast<const unsigned short*>(a.dy) + ((size_t)gnode * a.B + w) * a.dy_row + kc + 8 * g;
                    u32x4 bh[4], bl[4];
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        bh[s] = w < a.B ? *reinterpret_cast<const u32x4*>(row + 32 * s) : u32x4{0u, 0u, 0u, 0u};
                        if constexpr (MODE == IG_X3) bl[s] = w < a.B ? *reinterpret_cast<const u32x4*>(row + K + 32 * s) : u32x4{0u, 0u, 0u, 0u};
                    }
#pragma unroll
                    for (int ct = 0; ct < 4; ++ct) {
                        if (ct >= NCT) break;
                        const unsigned short* wl = reinterpret_cast<const unsigned short*>(smem) + (ct * 16 + l16) * KP + kc + 8 * g;
#pragma unroll
                        for (int s = 0; s < 4; ++s) {
                            const bf16x8 ah = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(wl + 32 * s));
                            acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, __builtin_bit_cast(bf16x8, bh[s]), acc[ct], 0, 0, 0);
                            if constexpr (MODE == IG_X3) {
                                const bf16x8 al = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(wl + CW * KP + 32 * s));
                                acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, __builtin_bit_cast(bf16x8, bl[s]), acc[ct], 0, 0, 0);
                                acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, __builtin_bit_cast(bf16x8, bh[s]), acc[ct], 0, 0, 0);
                            }
                        }
                    }
                }
            }
        }
        if (w >= a.B) continue;
        // lane holds D[f = 4 g + j][w = l16] of each 16-column tile: four consecutive columns of one output row
        OT* out = dx + ((size_t)w * n + i) * pitch;
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
            if (ct >= NCT) break;
            const int f0 = c0 + ct * 16 + 4 * g;
            OT v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int f = f0 + j;
                const float s = (sb >= 0 && f < F && a.signs[sb + f]) ? -acc[ct][j] : acc[ct][j];
                v[j] = (OT)s;
            }
            if (vec && f0 + 3 < pitch) {
                if constexpr (sizeof(OT) == 4) {
                    *reinterpret_cast<f32x4*>(out + f0) = f32x4{v[0], v[1], v[2], v[3]};
                } else {
                    typedef double f64x2 __attribute__((ext_vector_type(2)));
                    *reinterpret_cast<f64x2*>(out + f0) = f64x2{v[0], v[1]};
                    *reinterpret_cast<f64x2*>(out + f0 + 2) = f64x2{v[2], v[3]};
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) if (f0 + j < pitch) out[f0 + j] = v[j];
            }
        }
    }
}

template <int MODE, typename OT> int launch_ig(const IgArgs& a, unsigned grid, int lds, hipStream_t st) {
    static std::once_flag attr;
    static int rc = MSHGNN_OK;
    std::call_once(attr, [] { rc = set_lds_attr(k_input_grad<MODE, OT>, 160 * 1024); });
    if (rc) return rc;
    hipLaunchKernelGGL((k_input_grad<MODE, OT>), dim3(grid), dim3(256), lds, st, a);
    HIPCHK(hipGetLastError());
    return MSHGNN_OK;
}

std::mutex g_ig_mutex;

// {plan node, sign offset} of every (type, node) from the encoder's weight-gradient items (-1: the encoder does not compute that node), uploaded on first use
int ig_node_table(const mshgnn_plan* pc, const int** out) {
    mshgnn_plan* p = const_cast<mshgnn_plan*>(pc);
    std::lock_guard<std::mutex> lock(g_ig_mutex);
    if (p->d_ig_nodes) { *out = p->d_ig_nodes; return MSHGNN_OK; }
    const mshgnn_desc& d = p->gen ? gen_plan(p)->d : p->hp.d;
    int base[MSHGNN_MAX_TYPES + 1] = {0};
    for (int t = 0; t < d.n_types; ++t) base[t + 1] = base[t] + d.type_nodes[t];
    std::vector<int> tab(2 * (size_t)base[d.n_types], -1);
    if (p->gen) {
        const gen::GenPlan& gp = *gen_plan(p);
        const int n_items = (gp.fin_off - gp.item_off) / gen::GITEM_INTS;
        for (int k = 0; k < n_items; ++k) {
            const int* it = gp.tables.data() + gp.item_off + (size_t)k * gen::GITEM_INTS;
            if (it[gen::I_KIND] != 1 || it[gen::I_PBUF] != BUF_DX + 0 || it[gen::I_NSRC] != 1) continue;
            const int* s = gp.tables.data() + gp.src_off + (size_t)it[gen::I_SRC0] * gen::SRC_INTS;
            const int t = s[gen::S_BUF], i = s[gen::S_NODE];
            tab[2 * (base[t] + i)] = it[gen::I_PNODE];
            tab[2 * (base[t] + i) + 1] = s[gen::S_MASK];
        }
    } else {
        const HostPlan& hp = p->hp;
        for (int k = 0; k < hp.n_items; ++k) {
            const int* it = hp.tables.data() + hp.item_off + (size_t)k * ITEM_INTS;
            if (it[0] != BUF_DX + 0 || it[3] < BUF_IN || it[3] >= BUF_IN + MSHGNN_MAX_TYPES || it[4] != -1 || it[6] != 0) continue;      // the K chunk at column 0 of a raw-input item
            const int t = it[3] - BUF_IN, i = it[5];
            tab[2 * (base[t] + i)] = it[2];
            tab[2 * (base[t] + i) + 1] = it[8];
        }
    }
    int* dtab = nullptr;
    HIPCHK(hipMalloc(&dtab, tab.size() * sizeof(int)));
    if (hipMemcpy(dtab, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(dtab);
        return set_err(MSHGNN_EHIP, "hipMemcpy of the input-gradient node table failed");
    }
    p->d_ig_nodes = dtab;
    *out = dtab;
    return MSHGNN_OK;
}

}  // namespace

extern "C" int mshgnn_input_grad(const mshgnn_plan* p, const float* params, void* const* dx, const int64_t* dx_pitch, int dx_bytes,
                                 const void* workspace, int64_t batch, void* stream) {
    if (!p || !params || !dx || !workspace) return set_err(MSHGNN_EINVAL, "null argument to mshgnn_input_grad");
    if (batch < 1 || batch > (1 << 24)) return set_err(MSHGNN_EINVAL, "batch must be in [1, 2^24]");
    if (dx_bytes != 4 && dx_bytes != 8) return set_err(MSHGNN_EUNSUPPORTED, "mshgnn_input_grad writes fp32 (dx_bytes 4) or fp64 (dx_bytes 8) gradients");
    const bool gen = p->gen != nullptr;
    const mshgnn_desc& d = gen ? gen_plan(p)->d : p->hp.d;
    const int K = d.hidden;
    const int mode = gen ? (gen_plan(p)->split ? IG_X3 : IG_BF16) : (d.dtype == MSHGNN_F32 ? IG_F32 : d.dtype == MSHGNN_BF16 ? IG_BF16 : IG_X3);
    const int ebytes = mode == IG_F32 ? 4 : (mode == IG_X3 ? 4 : 2);      // LDS bytes per (column, k) of the staged weights
    int CW = 64;
    while (CW > 16 && (size_t)CW * (K + 8) * ebytes > 65536) CW >>= 1;
    const int lds = CW * (K + (mode == IG_F32 ? 4 : 8)) * ebytes;
    if (lds > 160 * 1024) return set_err(MSHGNN_EUNSUPPORTED, "hidden width too large for mshgnn_input_grad");
    const int* nodes = nullptr;
    if (int rc = ig_node_table(p, &nodes)) return rc;
    mshgnn_ws_layout lay;
    if (int rc = mshgnn_workspace_layout(p, batch, 1, &lay)) return rc;

    IgArgs a{};
    a.dy = reinterpret_cast<const char*>(workspace) + lay.dx[0];
    a.dy_row = (int64_t)K * (mode == IG_X3 ? 2 : 1);
    a.nodes = nodes; a.signs = gen ? gen_signs(p) : p->d_signs;
    a.K = K; a.B = (int)batch; a.nwb = (int)((batch + 15) / 16); a.CW = CW;
    int64_t units = 0;
    int node0 = 0;
    struct Req { int t; int64_t pitch; int ncc, tiles; };
    std::vector<Req> req;
    for (int t = 0; t < d.n_types; ++t) {
        if (dx[t]) {
            const int64_t pitch = dx_pitch ? dx_pitch[t] : d.type_width[t];
            if (pitch < d.type_width[t]) return set_err(MSHGNN_EINVAL, "dx_pitch below the input width");
            const int ncc = (int)((pitch + CW - 1) / CW), tiles = d.type_nodes[t] * a.nwb;
            req.push_back({t, pitch, ncc, tiles});
            units += (int64_t)ncc * tiles;
        }
    }
    if (req.empty()) return MSHGNN_OK;
    a.tpb = (int)std::max<int64_t>(4, ((units + 2047) / 2048 + 3) / 4 * 4);      // row tiles per workgroup: ~2048 workgroups in all
    int blk = 0;
    for (size_t r = 0; r < req.size(); ++r) {
        const int t = req[r].t;
        node0 = 0;
        for (int u = 0; u < t; ++u) node0 += d.type_nodes[u];
        IgType& ty = a.ty[r];
        ty.w = params + d.off_enc_w[t]; ty.dx = dx[t]; ty.pitch = req[r].pitch; ty.F = d.type_width[t]; ty.n = d.type_nodes[t];
        ty.ncc = req[r].ncc; ty.rgs = (req[r].tiles + a.tpb - 1) / a.tpb; ty.blk0 = blk; ty.node0 = node0;
        ty.vec = (((uintptr_t)dx[t] | (uintptr_t)(req[r].pitch * dx_bytes)) & 15) == 0;
        blk += ty.ncc * ty.rgs;
    }
    a.n_req = (int)req.size();
    hipStream_t st = (hipStream_t)stream;
    if (dx_bytes == 4) {
        if (mode == IG_F32) return launch_ig<IG_F32, float>(a, blk, lds, st);
        if (mode == IG_BF16) return launch_ig<IG_BF16, float>(a, blk, lds, st);
        return launch_ig<IG_X3, float>(a, blk, lds, st);
    }
    if (mode == IG_F32) return launch_ig<IG_F32, double>(a, blk, lds, st);
    if (mode == IG_BF16) return launch_ig<IG_BF16, double>(a, blk, lds, st);
    return launch_ig<IG_X3, double>(a, blk, lds, st);
}
