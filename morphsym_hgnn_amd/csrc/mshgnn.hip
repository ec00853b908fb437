// libmshgnn: MI355X (gfx950 / CDNA4) MS-HGNN message-passing engine -- HIP kernels + C-ABI (include/mshgnn.h).
//
// Design (DESIGN.md has the long form):
//   * every window graph shares one tiny topology  => a minibatch is a dense [B][NN][128] tensor per layer;
//   * a workgroup owns a tile of ROWS windows (16 for fp32, 32 for bf16): all NN node blocks (ROWS x 128, 8 KB
//     each, XOR-swizzled) are staged into LDS once per layer, and every per-relation linear of the layer is an
//     MFMA block-GEMM  acc[dst node] += X_lds[src node] . W  with the weight fragment held in registers and reused
//     for every destination node of the relation (root weights pre-summed per destination type);
//   * wave w of the workgroup owns output columns [32w, 32w+32) of every node; MFMA operands use a K-permutation
//     (lane group g owns a contiguous K range) so each lane's A and B data are 128 contiguous bytes;
//   * bias, ReLU, base_transform MLP, residual, ReLU-bit stash fused in the epilogue; backward reuses the same
//     engine on the transposed graph with transposed weight images; weight gradients are one split-K MFMA launch
//     over all layers with deterministic slab reduction (no float atomics).
//
// This file, top to bottom: (1) the kernels of the fp32 / bf16 plans -- prep, per-layer (the encoder: mshgnn_enc.hpp), 8-wave stack, the slab interpreters (the slab templates
// themselves: mshgnn_slab.hpp), decoder, weight gradient, finalize; (2) kernel selection; (3) plan lifecycle; (4) forward_impl / backward_impl; (5) the dispatch
// over plans and chunks; (6) the entry points, the series routes last.  Elsewhere: the split plan (mshgnn_x3.hip), the generic-width engine (mshgnn_gen.hip),
// the compile-time programs' kernels (mshgnn_spec_shard.hip), the plan-independent entry points (mshgnn_train_ops.hip) and window assembly (mshgnn_windows.hip).
//
// No CPU fallback exists: every entry point launches HIP kernels or fails loudly.
#include "mshgnn_slab.hpp"
#include "mshgnn_enc.hpp"
#include "mshgnn_launch.hpp"
extern "C" const char* mshgnn_last_error(void) { return g_err.c_str(); }
extern "C" const char* mshgnn_version(void) { return "mshgnn 0.5 (gfx950)"; }
extern "C" int mshgnn_abi_version(void) { return MSHGNN_ABI_VERSION; }
extern "C" size_t mshgnn_struct_size(int which) {
    switch (which) {
        case 0: return sizeof(mshgnn_desc);
        case 1: return sizeof(mshgnn_info);
        case 2: return sizeof(mshgnn_ws_layout);
        case 3: return sizeof(mshgnn_window_desc);
        case 4: return sizeof(mshgnn_kernel_stat);
        case 5: return sizeof(mshgnn_mlp_desc);
        case 6: return sizeof(mshgnn_mlp_info);
        case 7: return sizeof(mshgnn_mlp_input);
        default: return 0;
    }
}

// (k_prep / k_prep_tiled, the weight-image packing of every plan: mshgnn_device.hpp)
// (k_enc_fwd, the encoder of these plans, and splice8: defined in mshgnn_enc.hpp, beside the split plan's k_enc_x3)

// ------------------------------------------------------------------------------------------------------
// k_layer_fwd: one HeteroConv layer + activation / base_transform + residual  (hgnn_c2.py:150-166)
// ------------------------------------------------------------------------------------------------------
struct LayerArgs {
    const void* x_in;      // fwd: X_l                    bwd: G_{l+1} = dX_{l+1} (read; written when it is materialised here)
    void* x_out;           // fwd: X_{l+1}                bwd: layer 0 only: dX_0 = relu'(X_0) . (G_1 + D_0)
    unsigned* maskbits;    // relu bits of this layer [NN][4][B]
    void* hb; void* t1;    // base_transform stash of this layer [B][n_mlp][128]
    void* dh; void* du;    // bwd: dH_l [B][NN][128], dU_l [B][n_mlp][128]
    const void* x_act;     // bwd layer 0: X_0 (encoder relu mask)
    const void* wpack; const float* bias; const int* prog;
    int B, NN, n_mlp;
    int dbg;               // ablation switches for timing experiments (MSHGNN_DBG): 1 no stage-in, 2 no MACs, 4 no W loads, 8 no group epilogues,
                           // backward: 16 no stage-1 loads/stores, 32 no base_transform chain, 64 no stage-2 epilogues
};

template <typename T>
__device__ __forceinline__ void store_relu_bits(const typename Prec<T>::Acc& acc, unsigned* maskbits, int NN, int n, int w0, int B, int wn, int lane) {
    unsigned bits = 0;
#pragma unroll
    for (int fb = 0; fb < 2; ++fb)
#pragma unroll
        for (int j = 0; j < 4; ++j) bits |= (acc.c[fb][j] > 0.f ? 1u : 0u) << (4 * fb + j);
    // rows past the batch inside the last tile land in the buffer's padding (it is sized for whole tiles)
    reinterpret_cast<uint8_t*>(maskbits)[relu_byte(n, B, w0 + c_win(lane), wn * 32 + c_oct(lane))] = (uint8_t)bits;
}

// The wave's MAC program of a group lives in two VGPRs (entry i in lane i); entries are fetched with v_readlane.
struct WaveProg {
    int p0, p1, pc;
    __device__ __forceinline__ WaveProg(const int* prog, int lane) : p0(prog[lane]), p1(prog[64 + lane]), pc(0) {}
    __device__ __forceinline__ int next() {
        const int i = pc++;
        return i < 64 ? __builtin_amdgcn_readlane(p0, i) : __builtin_amdgcn_readlane(p1, i - 64);
    }
};

// run every segment of the group for this wave: per segment load the packed weight fragment once, then walk the
// accumulators in static order, each with its run-time list of source blocks
template <typename T>
__device__ __forceinline__ void run_segments(WaveProg& wp, int pc0, typename Prec<T>::Acc (&acc)[Prec<T>::HS], const char* smem,
                                             const T* wpack, int wn, int lane, int dbg) {
    using P = Prec<T>;
    wp.pc = pc0;
    const int nseg = wp.next();
    typename P::BFrag bf;
    typename P::AFrag af;
    for (int s = 0; s < nseg; ++s) {
        const int pack = wp.next();
        if (!ABL(dbg & 4) || s == 0) load_bfrag<T>(bf, wpack, pack, wn, lane);
#pragma unroll
        for (int u = 0; u < P::HS; ++u) {
            const int cnt = wp.next();
            for (int k = 0; k < cnt; ++k) {
                const int blk = wp.next();
                if (!ABL(dbg & 2)) {
                    load_afrag<T>(af, smem, blk, lane);
                    mac(acc[u], af, bf);
                }
            }
        }
    }
}

// one extra block-GEMM of the base_transform chain: acc[u] = bias + LDS[blk(slot)] . W(pack) for this wave's slots
template <typename T>
__device__ __forceinline__ void mlp_gemm(typename Prec<T>::Acc (&acc)[Prec<T>::HS], const char* smem, const int* blks, int ns,
                                         const T* wpack, int pack, const float* bias, int wn, int wh, int lane) {
    using P = Prec<T>;
    typename P::BFrag bf;
    typename P::AFrag af;
    load_bfrag<T>(bf, wpack, pack, wn, lane);
#pragma unroll
    for (int u = 0; u < P::HS; ++u) {
        const int slot = 2 * u + wh;
        if (slot < ns) {
            acc_init_bias<T>(acc[u], bias, wn, lane);
            load_afrag<T>(af, smem, blks[slot], lane);
            mac(acc[u], af, bf);
        }
    }
}

template <typename T> __global__ __launch_bounds__(LAYER_THREADS, Prec<T>::WPS) void k_layer_fwd(LayerArgs a) {
    using P = Prec<T>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wn = wv & 3, wh = wv >> 2;
    const int w0 = blockIdx.x * P::ROWS, B = a.B, NN = a.NN;
    const T* xin = reinterpret_cast<const T*>(a.x_in);
    T* xout = reinterpret_cast<T*>(a.x_out);
    const T* wpack = reinterpret_cast<const T*>(a.wpack);
    const int win = c_win(lane), w = w0 + win;
    const bool w_ok = w < B;

    const int* pg = a.prog;
    const int ngroups = pg[0];
    WaveProg wp(pg + 1 + ngroups * GH_SIZE + wh * WPROG_LEN, lane);   // the whole layer's MAC program of this wave, loaded once
    if (!ABL(a.dbg & 1)) stage_nodes<T>(smem, xin, NN, w0, B, tid);
    __syncthreads();

    typename P::Acc acc[P::HS];
    const int* gh = pg + 1;
    for (int g = 0; g < ngroups; ++g, gh += GH_SIZE) {
        const int kind = gh[GH_KIND], ns = gh[GH_NSLOTS], flags = gh[GH_FLAGS];
        const BiasQ bq = load_bias(a.bias + (size_t)gh[GH_BIAS] * H, wn, lane);
#pragma unroll
        for (int u = 0; u < P::HS; ++u) acc_fill(acc[u], 0.f);
        run_segments<T>(wp, gh[GH_PC0 + wh], acc, smem, wpack, wn, lane, a.dbg);
        if ABL(a.dbg & 8) continue;
#pragma unroll
        for (int u = 0; u < P::HS; ++u) { acc[u].c[0] += bq.b[0]; acc[u].c[1] += bq.b[1]; }
        if (kind == KIND_RELU) {
            const bool lds_epi = (flags & GF_LDS_EPI) != 0;
            // last group: every source block is dead once all waves are past their MACs -> X_new goes into the nodes'
            // own LDS blocks (residual read in place) and is then stored as whole rows
            if (lds_epi) __syncthreads();
#pragma unroll
            for (int u = 0; u < P::HS; ++u) {
                const int slot = 2 * u + wh;
                if (slot < ns) {
                    const int n = gh[GH_NODES + slot];
                    if (flags & GF_STORE_MASK) store_relu_bits<T>(acc[u], a.maskbits, NN, n, w0, B, wn, lane);
                    const int col = wn * 32 + c_oct(lane);
                    f32x4 y0 = relu4(acc[u].c[0]), y1 = relu4(acc[u].c[1]);
                    if (flags & GF_RESIDUAL) {
                        f32x4 r0, r1;
                        lds_load_oct<T>(smem, n, win, col, r0, r1);
                        y0 += r0; y1 += r1;
                    }
                    if (lds_epi) lds_store_oct<T>(smem, n, win, col, y0, y1);
                    else if (w_ok) store_oct(xout + act_idx(w, n, B) + col, y0, y1);
                }
            }
            if (lds_epi) {
                __syncthreads();
                const RowMap<T> m(tid);
                if (w0 + m.row < B)
                    for (int sl = m.sub; sl < ns; sl += RowMap<T>::NPB) {
                        const int n = gh[GH_NODES + sl];
                        const u32x4 v = *reinterpret_cast<const u32x4*>(smem + lds_chunk<T>(n, m.row, m.c));
                        *reinterpret_cast<u32x4*>(xout + act_idx(w0 + m.row, n, B) + m.c * P::EPC) = v;
                    }
            }
        } else {
            // base_transform: Y = W2 relu(W1 H + b1) + b2, X <- Y + X   (hgnn_c2.py:117-121,156,161-166)
            T* hb = reinterpret_cast<T*>(a.hb);
            T* t1 = reinterpret_cast<T*>(a.t1);
            const int* scr = gh + GH_SCR;
            const bool own = scr[0] == gh[GH_NODES];   // scratch aliases the nodes' own blocks (no spare LDS)
            __syncthreads();   // every wave is done reading the group's source blocks
#pragma unroll
            for (int u = 0; u < P::HS; ++u) {
                const int slot = 2 * u + wh;
                if (slot < ns) {
                    const int mi = gh[GH_MLPIDX + slot], col = wn * 32 + c_oct(lane);
                    lds_store_oct<T>(smem, scr[slot], win, col, acc[u].c[0], acc[u].c[1]);
                    if (w_ok) store_oct(hb + act_idx(w, mi, B) + col, acc[u].c[0], acc[u].c[1]);
                }
            }
            __syncthreads();
            mlp_gemm<T>(acc, smem, scr, ns, wpack, gh[GH_W1], a.bias + (size_t)gh[GH_B1] * H, wn, wh, lane);
            __syncthreads();   // all reads of H done before T1 overwrites the blocks
#pragma unroll
            for (int u = 0; u < P::HS; ++u) {
                const int slot = 2 * u + wh;
                if (slot < ns) {
                    const int mi = gh[GH_MLPIDX + slot], col = wn * 32 + c_oct(lane);
                    const f32x4 t0 = relu4(acc[u].c[0]), t1v = relu4(acc[u].c[1]);
                    lds_store_oct<T>(smem, scr[slot], win, col, t0, t1v);
                    if (w_ok) store_oct(t1 + act_idx(w, mi, B) + col, t0, t1v);
                }
            }
            __syncthreads();
            mlp_gemm<T>(acc, smem, scr, ns, wpack, gh[GH_W2], a.bias + (size_t)gh[GH_B2] * H, wn, wh, lane);
#pragma unroll
            for (int u = 0; u < P::HS; ++u) {
                const int slot = 2 * u + wh;
                if (slot < ns && w_ok) {
                    const int n = gh[GH_NODES + slot], col = wn * 32 + c_oct(lane);
                    f32x4 y0 = acc[u].c[0], y1 = acc[u].c[1];
                    if (flags & GF_RESIDUAL) {
                        f32x4 r0, r1;
                        if (own) load_oct(xin + act_idx(w, n, B) + col, r0, r1);
                        else lds_load_oct<T>(smem, n, win, col, r0, r1);
                        y0 += r0; y1 += r1;
                    }
                    store_oct(xout + act_idx(w, n, B) + col, y0, y1);
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------
// k_layer_bwd: G_{l+1} = G_{l+2} + D_{l+1} (coalesced, materialised), dH_l from it (relu bits / base_transform
// chain), then D_l on the transposed graph.  Layer 0 finishes dX_0 = relu'(X_0) . (G_1 + D_0) itself.
// ------------------------------------------------------------------------------------------------------
template <typename T> __global__ __launch_bounds__(LAYER_THREADS, Prec<T>::WPS) void k_layer_bwd(LayerArgs a) {
    using P = Prec<T>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wn = wv & 3, wh = wv >> 2;
    const int w0 = blockIdx.x * P::ROWS, B = a.B, NN = a.NN;
    const T* gtop = reinterpret_cast<const T*>(a.x_in);   // dX_{l+1}
    T* dxo = reinterpret_cast<T*>(a.x_out);               // dX_l
    T* dh = reinterpret_cast<T*>(a.dh);
    const T* xact = reinterpret_cast<const T*>(a.x_act);
    const T* wpack = reinterpret_cast<const T*>(a.wpack);
    const int* pg = a.prog;
    const int ngroups = pg[BH_NGROUPS], nmlp = pg[BH_NMLP], w2pack = pg[BH_W2], w1pack = pg[BH_W1];
    const int* node_kind = pg + BH_KIND;
    const int* mlp_nodes = pg + BH_MLPNODES;
    WaveProg wp(pg + BH_SIZE + ngroups * GH_SIZE + wh * WPROG_LEN, lane);   // this wave's MAC program of the layer, loaded once
    const int win = c_win(lane), w = w0 + win;
    const bool w_ok = w < B;

    // stage 1 (row-major, coalesced): G_{l+1} -> LDS; relu nodes masked (-> dH, also to global for k_gradw)
    {
        constexpr int EPC = P::EPC, NPB = RowMap<T>::NPB, BATCH = 5;
        const RowMap<T> m(tid);
        const int row = m.row, c = m.c, wr = w0 + row;
        for (int nb = m.sub; nb < NN; nb += NPB * BATCH) {
            u32x4 v[BATCH]; unsigned word[BATCH]; int nk[BATCH];
#pragma unroll
            for (int i = 0; i < BATCH; ++i) {       // issue every load of the batch first
                const int n = nb + i * NPB;
                nk[i] = n < NN ? node_kind[n] : NK_DEAD;
                v[i] = u32x4{0, 0, 0, 0}; word[i] = 0;
                if (nk[i] != NK_DEAD && wr < B && !ABL(a.dbg & 16)) {
                    v[i] = *reinterpret_cast<const u32x4*>(gtop + act_idx(wr, n, B) + c * EPC);
                    if (nk[i] == NK_RELU) word[i] = reinterpret_cast<const uint8_t*>(a.maskbits)[relu_byte(n, B, wr, c * EPC)];
                }
            }
#pragma unroll
            for (int i = 0; i < BATCH; ++i) {
                const int n = nb + i * NPB;
                if (nk[i] == NK_DEAD) continue;
                if (nk[i] == NK_RELU) {
                    v[i] = chunk_mask_bits<T>(v[i], word[i] >> ((c * EPC) % 8));   // dH (k_gradw recomputes it the same way)
                }
                *reinterpret_cast<u32x4*>(smem + lds_chunk<T>(n, row, c)) = v[i];
            }
        }
    }
    __syncthreads();

    typename P::Acc acc[P::HS];

    if (nmlp > 0 && !ABL(a.dbg & 32)) {
        // dT1 = dY W2 ; dU = dT1 . (T1 > 0) ; dH = dU W1     (backward of base_transform; re-uses the base blocks)
        const T* t1 = reinterpret_cast<const T*>(a.t1);
        T* du = reinterpret_cast<T*>(a.du);
        mlp_gemm<T>(acc, smem, mlp_nodes, nmlp, wpack, w2pack, nullptr, wn, wh, lane);
        __syncthreads();   // all reads of dY blocks done
#pragma unroll
        for (int u = 0; u < P::HS; ++u) {
            const int slot = 2 * u + wh;
            if (slot < nmlp) {
                const int col = wn * 32 + c_oct(lane);
                f32x4 r0 = f32x4{0, 0, 0, 0}, r1 = f32x4{0, 0, 0, 0};
                if (w_ok) {
                    f32x4 tv0, tv1;
                    load_oct(t1 + act_idx(w, slot, B) + col, tv0, tv1);
#pragma unroll
                    for (int j = 0; j < 4; ++j) { r0[j] = tv0[j] > 0.f ? acc[u].c[0][j] : 0.f; r1[j] = tv1[j] > 0.f ? acc[u].c[1][j] : 0.f; }
                    store_oct(du + act_idx(w, slot, B) + col, r0, r1);
                }
                lds_store_oct<T>(smem, mlp_nodes[slot], win, col, r0, r1);
            }
        }
        __syncthreads();
        mlp_gemm<T>(acc, smem, mlp_nodes, nmlp, wpack, w1pack, nullptr, wn, wh, lane);
        __syncthreads();   // all reads of dU blocks done
#pragma unroll
        for (int u = 0; u < P::HS; ++u) {
            const int slot = 2 * u + wh;
            if (slot < nmlp) {
                const int n = mlp_nodes[slot], col = wn * 32 + c_oct(lane);
                lds_store_oct<T>(smem, n, win, col, acc[u].c[0], acc[u].c[1]);
                if (w_ok) store_oct(dh + act_idx(w, n, B) + col, acc[u].c[0], acc[u].c[1]);
            }
        }
        __syncthreads();
    }

    // stage 2: D_l[j] = dH_j W_rootsum + sum_r sum_{j->i} dH_i W_rel^r
    const int* gh = pg + BH_SIZE;
    for (int g = 0; g < ngroups; ++g, gh += GH_SIZE) {
        const int ns = gh[GH_NSLOTS], flags = gh[GH_FLAGS];
#pragma unroll
        for (int u = 0; u < P::HS; ++u) acc_fill(acc[u], 0.f);
        run_segments<T>(wp, gh[GH_PC0 + wh], acc, smem, wpack, wn, lane, a.dbg);
        if ABL(a.dbg & 64) continue;
        if (flags & GF_LDS_EPI) {
            __syncthreads();   // last group: all dH blocks are dead -> stage D through LDS, store whole rows
#pragma unroll
            for (int u = 0; u < P::HS; ++u) {
                const int slot = 2 * u + wh;
                if (slot < ns) lds_store_oct<T>(smem, gh[GH_NODES + slot], win, wn * 32 + c_oct(lane), acc[u].c[0], acc[u].c[1]);
            }
            __syncthreads();
            const RowMap<T> m(tid);
            const int row = m.row, c = m.c;
            if (w0 + row < B)
                for (int sl0 = m.sub; sl0 < ns; sl0 += 2 * RowMap<T>::NPB) {
                    u32x4 v[2], g1[2], xa[2]; bool ok[2];
#pragma unroll
                    for (int i = 0; i < 2; ++i) {       // two nodes in flight per thread
                        const int sl = sl0 + i * RowMap<T>::NPB;
                        ok[i] = sl < ns;
                        const int n = gh[GH_NODES + (ok[i] ? sl : 0)];
                        const size_t idx = act_idx(w0 + row, n, B) + c * P::EPC;
                        v[i] = *reinterpret_cast<const u32x4*>(smem + lds_chunk<T>(n, row, c));
                        g1[i] = u32x4{0, 0, 0, 0}; xa[i] = u32x4{0, 0, 0, 0};
                        if (ok[i] && (flags & GF_RESIDUAL)) g1[i] = *reinterpret_cast<const u32x4*>(gtop + idx);
                        if (ok[i] && (flags & GF_ENC_MASK)) xa[i] = *reinterpret_cast<const u32x4*>(xact + idx);
                    }
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        if (!ok[i]) continue;
                        const int n = gh[GH_NODES + sl0 + i * RowMap<T>::NPB];
                        const size_t idx = act_idx(w0 + row, n, B) + c * P::EPC;
                        u32x4 r = v[i];
                        if (flags & GF_RESIDUAL) r = chunk_add<T>(r, g1[i]);             // dX_l = dX_{l+1} + D_l
                        if (flags & GF_ENC_MASK) r = chunk_mask_pos<T>(r, xa[i]);        // layer 0: x relu'(X_0)
                        *reinterpret_cast<u32x4*>(dxo + idx) = r;
                    }
                }
        } else {
#pragma unroll
            for (int u = 0; u < P::HS; ++u) {
                const int slot = 2 * u + wh;
                if (slot < ns && w_ok) {
                    const int n = gh[GH_NODES + slot];
                    const size_t idx = act_idx(w, n, B) + wn * 32 + c_oct(lane);
                    f32x4 g1[2] = {f32x4{0, 0, 0, 0}, f32x4{0, 0, 0, 0}}, xa[2] = {f32x4{1, 1, 1, 1}, f32x4{1, 1, 1, 1}};
                    if (flags & GF_RESIDUAL) load_oct(gtop + idx, g1[0], g1[1]);
                    if (flags & GF_ENC_MASK) load_oct(xact + idx, xa[0], xa[1]);
                    f32x4 y[2];
#pragma unroll
                    for (int fb = 0; fb < 2; ++fb) {
                        y[fb] = round_as<T>(acc[u].c[fb]) + g1[fb];
#pragma unroll
                        for (int j = 0; j < 4; ++j) y[fb][j] = xa[fb][j] > 0.f ? y[fb][j] : 0.f;
                    }
                    store_oct(dxo + idx, y[0], y[1]);
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------
// FUSED STACK kernels (bf16 plan): the whole message-passing stack of one 16-window tile in ONE workgroup.
//   k_stack_fwd: X_0 tile -> LDS, L x (HeteroConv + relu / base_transform + residual) in place, decoder -> out.
//   k_stack_bwd: dX_L tile -> LDS, L x (relu' / base_transform backward, transposed HeteroConv, residual) in place.
// Every node owns one accumulator per wave for the whole layer (node n -> wave half n & 1, accumulator n >> 1), so a
// layer's epilogue runs once, after every wave has finished reading the previous activations, and overwrites them in
// place; the stashes the backward pass / k_gradw need are written on the side and never read back by this kernel.
// One workgroup of 8 waves per CU (<= 256 VGPRs per wave): all accumulators live + double-buffered weight fragments.

// STEP: part of k_stack_step -- the decoder tail leaves dX_L in the out-type nodes' LDS blocks for the backward sweep that follows in the same launch
template <typename T, bool STEP> __device__ __forceinline__ void stack_fwd_body(const StackArgs& a, char* smem) {
    using P = Prec<T>;
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wn = wv & 3, wh = wv >> 2;
    const int w0 = blockIdx.x * P::ROWS, B = a.B, NN = a.NN;
    const T* wpack = reinterpret_cast<const T*>(a.wpack);
    const int win = c_win(lane), w = w0 + win, col = wn * 32 + c_oct(lane);
    const bool w_ok = w < B, train = a.training != 0;

    FS_STAMP(0);
    stage_nodes<T>(smem, reinterpret_cast<const T*>(a.tile_in), NN, w0, B, tid);
    __syncthreads();
    FS_STAMP(1);

    typename P::Acc acc[FS_HS];
    FHdr fhn(a.tables + a.prog_off[0], lane);
    FProg wpn(a.tables + a.prog_off[0] + FH_SIZE + wh * FPROG_LEN, lane);
    fhn.settle(); wpn.settle();
    for (int l = 0; l < a.L; ++l) {
        const FHdr fh = fhn;
        const FProg wp = wpn;
        if (l + 1 < a.L) {    // the next layer's header and wave program stream in under this layer's MACs
            fhn = FHdr(a.tables + a.prog_off[l + 1], lane);
            wpn = FProg(a.tables + a.prog_off[l + 1] + FH_SIZE + wh * FPROG_LEN, lane);
        }
        const int nmlp = fh[FH_NMLP], flags = fh[FH_FLAGS];
        // accumulators start at the bias row of their node's type (the loads hide under the first weight fragment)
#pragma unroll
        for (int u = 0; u < FS_HS; ++u) {
            const int n = 2 * u + wh;
            if (n < NN && fh[FH_KIND + n] != NK_DEAD) acc_init_bias<T>(acc[u], a.bias + (size_t)fh[FH_BIAS + n] * H, wn, lane);
            else acc_fill(acc[u], 0.f);
        }
        FS_STAMP(2 + 4 * l);
#ifdef MSHGNN_SEG_STAMPS
        // per-wave clock at every segment start of every layer: [layer][wave][16] in LDS behind the node blocks, dumped at the end
        long long* segclk = a.stamps ? reinterpret_cast<long long*>(smem + (NN + 4) * P::BLK) + (l * 8 + wv) * 16 : nullptr;
        fs_run<T>(wp, acc, smem, wpack, wn, lane, a.dbg, segclk);
#else
        if (!ABL(a.dbg & 2)) fs_run<T>(wp, acc, smem, wpack, wn, lane, a.dbg);
#endif
        FS_STAMP(3 + 4 * l);
        __syncthreads();   // every wave is done reading X_l: the node blocks may be overwritten
        FS_STAMP(4 + 4 * l);
        if ABL(a.dbg & 8) continue;

        u32x4 hpk[2] = {}, tpk[2] = {};
        if (nmlp > 0 && !ABL(a.dbg & 64)) {
            // base_transform: Y = W2 relu(W1 H + b1) + b2 on the first nmlp nodes (hgnn_c2.py:117-121,156); scratch blocks NN + i.
            // The H and T1 stashes are kept packed in registers and stored after the chain: a load waited for while stores are in
            // flight costs a full drain of those stores.
            static_assert(sizeof(T) == 2, "fused stack kernels are bf16");
            typename P::BFrag bf, bf2;
            typename P::AFrag af;
            load_bfrag<T>(bf, wpack, fh[FH_W1], wn, lane);
            load_bfrag<T>(bf2, wpack, fh[FH_W2], wn, lane);
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int n = 2 * u + wh;
                if (n < nmlp) {
                    hpk[u] = pack_oct(acc[u].c[0], acc[u].c[1]);
                    *reinterpret_cast<u32x4*>(smem + lds_chunk<T>(NN + n, win, col / P::EPC)) = hpk[u];
                    acc_init_bias<T>(acc[u], a.bias + (size_t)fh[FH_B1] * H, wn, lane);
                }
            }
            __syncthreads();
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int n = 2 * u + wh;
                if (n < nmlp) {
                    load_afrag<T>(af, smem, NN + n, lane);
                    mac(acc[u], af, bf);
                }
            }
            __syncthreads();   // all reads of H done before T1 overwrites the scratch blocks
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int n = 2 * u + wh;
                if (n < nmlp) {
                    tpk[u] = pack_oct(relu4(acc[u].c[0]), relu4(acc[u].c[1]));
                    *reinterpret_cast<u32x4*>(smem + lds_chunk<T>(NN + n, win, col / P::EPC)) = tpk[u];
                    acc_init_bias<T>(acc[u], a.bias + (size_t)fh[FH_B2] * H, wn, lane);
                }
            }
            __syncthreads();
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int n = 2 * u + wh;
                if (n < nmlp) {
                    load_afrag<T>(af, smem, NN + n, lane);
                    mac(acc[u], af, bf2);
                }
            }
        }
        FS_STAMP(16 + l);
        // every load issued so far (chain operands, the next layer's header and program) has landed before the first store of
        // the epilogue goes out: from here to the next layer's first weight fragment nothing waits on a load
        __builtin_amdgcn_s_waitcnt((7 << 4) | (15 << 8));
        fhn.settle(); wpn.settle();      // (and the compiler stops tracking them as pending: no vmcnt(0) at the top of the next layer, FProg::settle)
        if (nmlp > 0 && train && w_ok) {
            T* hb = reinterpret_cast<T*>(a.ws + a.hb_off[l]);
            T* t1 = reinterpret_cast<T*>(a.ws + a.t1_off[l]);
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int n = 2 * u + wh;
                if (n < nmlp) {
                    *reinterpret_cast<u32x4*>(hb + act_idx(w, n, B) + col) = hpk[u];
                    *reinterpret_cast<u32x4*>(t1 + act_idx(w, n, B) + col) = tpk[u];
                }
            }
        }

        // X_{l+1}[n] = f(H[n]) (+ X_l[n]) for every live node, in place; stash + relu bits on the side
        T* xo = reinterpret_cast<T*>(a.ws + a.x_off[l + 1]);
        unsigned* maskbits = reinterpret_cast<unsigned*>(a.ws + a.mask_off[l]);
        u32x4 resv[FS_HS]; int kindv[FS_HS];     // the residual octets of every node, all LDS reads in flight together
#pragma unroll
        for (int u = 0; u < FS_HS; ++u) {
            const int n = 2 * u + wh;
            kindv[u] = n < NN ? fh[FH_KIND + n] : NK_DEAD;
            resv[u] = u32x4{0, 0, 0, 0};
            if (kindv[u] != NK_DEAD && (flags & FF_RESIDUAL)) resv[u] = *reinterpret_cast<const u32x4*>(smem + lds_chunk<T>(n, win, col / P::EPC));
        }
#pragma unroll
        for (int u = 0; u < FS_HS; ++u) {
            const int n = 2 * u + wh;
            if (n < NN) {
                const int kind = kindv[u];
                if (kind != NK_DEAD) {
                    f32x4 y0 = acc[u].c[0], y1 = acc[u].c[1];
                    if (kind == NK_RELU) {
                        const unsigned bits = relu_with_bits<T>(acc[u]);
                        if (train) reinterpret_cast<uint8_t*>(maskbits)[relu_byte(n, B, w, col)] = (uint8_t)bits;
                        y0 = acc[u].c[0]; y1 = acc[u].c[1];
                    }
                    if (flags & FF_RESIDUAL) {
                        const u32x4 r = resv[u];
                        y0 += f32x4{__builtin_bit_cast(float, r[0] << 16), __builtin_bit_cast(float, r[0] & 0xffff0000u),
                                    __builtin_bit_cast(float, r[1] << 16), __builtin_bit_cast(float, r[1] & 0xffff0000u)};
                        y1 += f32x4{__builtin_bit_cast(float, r[2] << 16), __builtin_bit_cast(float, r[2] & 0xffff0000u),
                                    __builtin_bit_cast(float, r[3] << 16), __builtin_bit_cast(float, r[3] & 0xffff0000u)};
                    }
                    lds_store_oct<T>(smem, n, win, col, y0, y1);
                    if (train && w_ok && !ABL(a.dbg & 16) && !(STEP && l + 1 == a.L)) store_oct(xo + act_idx(w, n, B) + col, y0, y1);      // (X_L of a one-launch step is read by nobody: the decoder's gradients come from the tile in LDS)
                }
            }
        }
        __syncthreads();
        FS_STAMP(5 + 4 * l);
    }

    decoder_tail<T, LAYER_THREADS, false, STEP>(a, smem, tid, lane, wv, w0, B);
    FS_STAMP(30);
#ifdef MSHGNN_SEG_STAMPS
    if (a.stamps) {
        __syncthreads();
        const long long* sc = reinterpret_cast<const long long*>(smem + (NN + 4) * P::BLK);
        if (tid < 3 * 8 * 16) a.stamps[(size_t)gridDim.x * 32 + (size_t)blockIdx.x * 384 + tid] = sc[tid];
    }
#endif
}
template <typename T> __global__ __launch_bounds__(LAYER_THREADS, 2) void k_stack_fwd(StackArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    stack_fwd_body<T, false>(a, smem);
}

// STEP: part of k_stack_step -- the forward's decoder tail of the same launch left the dX_L tile in LDS; the layers' programs are a.prog_off_b
template <typename T, bool STEP> __device__ __forceinline__ void stack_bwd_body(const StackArgs& a, char* smem) {
    using P = Prec<T>;
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wn = wv & 3, wh = wv >> 2;
    const int w0 = blockIdx.x * P::ROWS, B = a.B, NN = a.NN;
    const T* wpack = reinterpret_cast<const T*>(a.wpack);
    auto prog_of = [&](int l) { return STEP ? a.prog_off_b[l] : a.prog_off[l]; };

    FS_STAMP(0);
    // dX_L tile: only the nodes that are live in the last layer carry a gradient
    if constexpr (!STEP) {
        const FHdr bh(a.tables + prog_of(a.L - 1), lane);
        const T* src = reinterpret_cast<const T*>(a.tile_in);
        const RowMap<T> m(tid);
        for (int n = m.sub; n < NN; n += RowMap<T>::NPB) {
            if (bh[FH_KIND + n] == NK_DEAD) continue;
            u32x4 v = u32x4{0, 0, 0, 0};
            if (w0 + m.row < B) v = *reinterpret_cast<const u32x4*>(src + act_idx(w0 + m.row, n, B) + m.c * P::EPC);
            *reinterpret_cast<u32x4*>(smem + lds_chunk<T>(n, m.row, m.c)) = v;
        }
    }
    __syncthreads();
    FS_STAMP(1);

    typename P::Acc acc[FS_HS];
    FHdr bhn(a.tables + prog_of(a.L - 1), lane);
    FProg wpn(a.tables + prog_of(a.L - 1) + FH_SIZE + wh * FPROG_LEN, lane);
    bhn.settle(); wpn.settle();
    for (int l = a.L - 1; l >= 0; --l) {
        const FHdr bh = bhn;
        const FProg wp = wpn;
        if (l > 0) {          // the next layer's header and wave program stream in under this layer's MACs
            bhn = FHdr(a.tables + prog_of(l - 1), lane);
            wpn = FProg(a.tables + prog_of(l - 1) + FH_SIZE + wh * FPROG_LEN, lane);
        }
        const int nmlp = bh[FH_NMLP], flags = bh[FH_FLAGS];
        const unsigned* maskbits = reinterpret_cast<const unsigned*>(a.ws + a.mask_off[l]);
        // lane constants rebuilt per layer from an opaque copy of the lane id: the per-node 64-bit addresses derived from them were hoisted out of the
        // layer loop and spilled, and a scratch reload next to the epilogue's pending stores is a full vmcnt(0) drain
        const int lq = opaque(lane);
        const int win = c_win(lq), w = w0 + win, col = wn * 32 + c_oct(lq), g8 = (lq >> 4) << 3;
        const bool w_ok = w < B;

        // phase 1 (each lane on the octets it owns): the accumulator of node n starts at its residual term
        // G_{l+1}[n]; relu nodes are then masked in place -> dH_l[n].  Every relu-bit word and every LDS read is issued
        // before the first use: one memory latency per layer, not one per node.
        {
            unsigned mword[FS_HS]; u32x4 rawv[FS_HS]; int kindv[FS_HS];
#pragma unroll
            for (int u = 0; u < FS_HS; ++u) {
                const int n = 2 * u + wh;
                kindv[u] = n < NN ? bh[FH_KIND + n] : NK_DEAD;
                mword[u] = 0u; rawv[u] = u32x4{0, 0, 0, 0};
                if (kindv[u] == NK_RELU && w_ok) mword[u] = reinterpret_cast<const uint8_t*>(maskbits)[relu_byte(n, B, w, wn * 32 + g8)];
                if (kindv[u] != NK_DEAD) rawv[u] = *reinterpret_cast<const u32x4*>(smem + lds_chunk<T>(n, win, col / P::EPC));
            }
#pragma unroll
            for (int u = 0; u < FS_HS; ++u) {
                const int n = 2 * u + wh;
                acc_fill(acc[u], 0.f);
                if (kindv[u] != NK_DEAD) {
                    const u32x4 raw = rawv[u];
                    if (bh[FH_RES + n]) {
                        acc[u].c[0] = f32x4{__builtin_bit_cast(float, raw[0] << 16), __builtin_bit_cast(float, raw[0] & 0xffff0000u),
                                            __builtin_bit_cast(float, raw[1] << 16), __builtin_bit_cast(float, raw[1] & 0xffff0000u)};
                        acc[u].c[1] = f32x4{__builtin_bit_cast(float, raw[2] << 16), __builtin_bit_cast(float, raw[2] & 0xffff0000u),
                                            __builtin_bit_cast(float, raw[3] << 16), __builtin_bit_cast(float, raw[3] & 0xffff0000u)};
                    }
                    if (kindv[u] == NK_RELU)
                        *reinterpret_cast<u32x4*>(smem + lds_chunk<T>(n, win, col / P::EPC)) = chunk_mask_bits<T>(raw, mword[u]);
                }
            }
        }
        __syncthreads();
        FS_STAMP(2 + 5 * (a.L - 1 - l));

        if (nmlp > 0) {
            // dT1 = dY W2 ; dU = dT1 . (T1 > 0) ; dH = dU W1     (backward of base_transform, in place on nodes 0..nmlp-1)
            const T* t1 = reinterpret_cast<const T*>(a.ws + a.t1_off[l]);
            T* du = reinterpret_cast<T*>(a.ws + a.du_off[l]);
            T* dh = reinterpret_cast<T*>(a.ws + a.dh_off[l]);
            typename P::BFrag bf;
            typename P::AFrag af;
            typename P::Acc tm[2];
            f32x4 tv0[2], tv1[2];
            load_bfrag<T>(bf, wpack, bh[FH_W2], wn, lane);
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int n = 2 * u + wh;
                tv0[u] = f32x4{0, 0, 0, 0}; tv1[u] = f32x4{0, 0, 0, 0};
                if (n < nmlp) {
                    if (w_ok) load_oct(t1 + act_idx(w, n, B) + col, tv0[u], tv1[u]);
                    acc_fill(tm[u], 0.f);
                    load_afrag<T>(af, smem, n, lane);
                    mac(tm[u], af, bf);
                }
            }
            load_bfrag<T>(bf, wpack, bh[FH_W1], wn, lane);
            __syncthreads();   // all reads of the dY blocks done
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int n = 2 * u + wh;
                if (n < nmlp) {
                    f32x4 r0, r1;
#pragma unroll
                    for (int j = 0; j < 4; ++j) { r0[j] = tv0[u][j] > 0.f ? tm[u].c[0][j] : 0.f; r1[j] = tv1[u][j] > 0.f ? tm[u].c[1][j] : 0.f; }
                    if (w_ok) store_oct(du + act_idx(w, n, B) + col, r0, r1);
                    lds_store_oct<T>(smem, n, win, col, r0, r1);
                }
            }
            __syncthreads();
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int n = 2 * u + wh;
                if (n < nmlp) {
                    acc_fill(tm[u], 0.f);
                    load_afrag<T>(af, smem, n, lane);
                    mac(tm[u], af, bf);
                }
            }
            __syncthreads();   // all reads of the dU blocks done
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int n = 2 * u + wh;
                if (n < nmlp) {
                    lds_store_oct<T>(smem, n, win, col, tm[u].c[0], tm[u].c[1]);
                    if (w_ok) store_oct(dh + act_idx(w, n, B) + col, tm[u].c[0], tm[u].c[1]);
                }
            }
            __syncthreads();
        }

        // phase 2: dX_l[j] = (residual) + dH_j W_rootsum + sum_r sum_{j->i} dH_i W_rel^r
        FS_STAMP(3 + 5 * (a.L - 1 - l));
        fs_run<T>(wp, acc, smem, wpack, wn, lane);
        FS_STAMP(4 + 5 * (a.L - 1 - l));
        __syncthreads();   // every wave is done reading dH_l
        FS_STAMP(5 + 5 * (a.L - 1 - l));

        T* dxo = reinterpret_cast<T*>(a.ws + a.dx_off[l]);
        const T* xact = reinterpret_cast<const T*>(a.ws + a.x_off[0]);
        bhn.settle(); wpn.settle();      // next header / program landed before the stores go out (FProg::settle)
        // layer 0: the encoder's relu bytes of every node are requested before the first store of the epilogue (a load waited for while stores are
        // in flight drains them all: one round trip instead of one per node)
        unsigned xbv[FS_HS];
#pragma unroll
        for (int u = 0; u < FS_HS; ++u) {
            const int n = 2 * u + wh;
            xbv[u] = 0xffu;
            if ((flags & FF_ENC_MASK) && w_ok && a.mask0_off && n < NN && bh[FH_OUT + n])
                xbv[u] = reinterpret_cast<const uint8_t*>(a.ws + a.mask0_off)[relu_byte(n, B, w, wn * 32 + g8)];
        }
#pragma unroll
        for (int u = 0; u < FS_HS; ++u) {
            const int n = 2 * u + wh;
            if (n < NN && bh[FH_OUT + n]) {
                f32x4 y0 = acc[u].c[0], y1 = acc[u].c[1];
                if ((flags & FF_ENC_MASK) && w_ok) {   // layer 0: x relu'(X_0)  (encoder activation)
                    if (a.mask0_off) {      // the encoder's relu byte of this lane
                        const unsigned xb = xbv[u];
#pragma unroll
                        for (int j = 0; j < 4; ++j) { y0[j] = ((xb >> j) & 1u) ? y0[j] : 0.f; y1[j] = ((xb >> (4 + j)) & 1u) ? y1[j] : 0.f; }
                    } else {
                        f32x4 x0, x1;
                        load_oct(xact + act_idx(w, n, B) + col, x0, x1);
#pragma unroll
                        for (int j = 0; j < 4; ++j) { y0[j] = x0[j] > 0.f ? y0[j] : 0.f; y1[j] = x1[j] > 0.f ? y1[j] : 0.f; }
                    }
                }
                if (l > 0) lds_store_oct<T>(smem, n, win, col, y0, y1);
                if (w_ok) store_oct(dxo + act_idx(w, n, B) + col, y0, y1);
            }
        }
        __syncthreads();
        FS_STAMP(6 + 5 * (a.L - 1 - l));
    }
}
template <typename T> __global__ __launch_bounds__(LAYER_THREADS, 2) void k_stack_bwd(StackArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    stack_bwd_body<T, false>(a, smem);
}
// the one-call steps below the slab kernels' batch size: both sweeps of a tile in one launch (k_slab_step's scheme on the 8-wave kernels)
template <typename T> __global__ __launch_bounds__(LAYER_THREADS, 2) void k_stack_step(StackArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    stack_fwd_body<T, true>(a, smem);
    __syncthreads();
    stack_bwd_body<T, true>(a, smem);
}

// ------------------------------------------------------------------------------------------------------
// The slab stack kernels (mshgnn_slab.hpp: 4 waves per workgroup, two workgroups per CU) over the plan's run-time tables: the interpreters.
// Those over the compile-time programs are mshgnn_spec_shard.hip's.
// ------------------------------------------------------------------------------------------------------
template <typename T, int NM, int HB> __global__ __launch_bounds__(SL_THREADS, 2) void k_slab_fwd(StackArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    slab_fwd_body<T, NM, HB, false>(a, smem);
}
template <typename T, int NM, int HB> __global__ __launch_bounds__(SL_THREADS, 2) void k_slab_bwd(StackArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    slab_bwd_body<T, NM, HB, false>(a, smem);
}

// ------------------------------------------------------------------------------------------------------
// decoder forward / backward (hgnn_c2.py:176-189) and the wrapper's MSE (gnnLightning.py:633-639)
// ------------------------------------------------------------------------------------------------------
template <typename T> __global__ __launch_bounds__(256) void k_dec_fwd(DecArgs a) {
    const int c = threadIdx.x & 15;
    const int64_t row = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    const int64_t rows = (int64_t)a.B * a.n_out;
    const bool ok = row < rows;
    const int w = ok ? (int)(row / a.n_out) : 0, f = ok ? (int)(row % a.n_out) : 0;
    float x[8];
    load8<T>(reinterpret_cast<const T*>(a.xl) + act_idx(w, a.node0 + f, a.B) + c * 8, x);
    const float* W = a.params + a.off_w;
    for (int d = 0; d < a.dout; ++d) {
        float s = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) s += x[e] * W[d * H + c * 8 + e];
#pragma unroll
        for (int m = 8; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
        if (c == 0 && ok) a.out[row * a.dout + d] = (s + a.params[a.off_b + d]) * a.out_mask[f * a.dout + d];
    }
}

// (k_dec_bwd<T, false>, the decoder backward of these plans: mshgnn_device.hpp, beside the split plan's instantiation)

// ------------------------------------------------------------------------------------------------------
// k_gradw: all weight gradients of the step as one split-K MFMA launch.  dW[o][k] = sum_w P[w][o] Q[w][k]
// workgroup = (lane, part): the lane's <= GW_IPL items over window part `part`; slab index = blockIdx.x
// ------------------------------------------------------------------------------------------------------
constexpr int GW_KW = 32;       // fp32: windows per staged chunk
constexpr int GW_PITCH = 144;   // fp32: floats per LDS row (bank-conflict-free column reads)

__global__ __launch_bounds__(256) void k_gradw_f32(GradwArgs a) {
    using T = float;
    __shared__ __attribute__((aligned(16))) float Ps[GW_KW * GW_PITCH];
    __shared__ __attribute__((aligned(16))) float Qs[GW_KW * GW_PITCH];
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wv >> 1, wc = wv & 1;
    // blocks b and b+8 share an XCD (round-robin dispatch; speed only): lane_order puts the lanes that read the same
    // dH / X rows on one XCD so they share its L2
    const int ln = a.lane_order[blockIdx.x % a.n_pad], part = blockIdx.x / a.n_pad;
    if (ln < 0) return;
    const int* lh = a.lanes + ln * LANE_INTS;
    const int it0 = lh[0], it1 = lh[1], bias_flag = lh[3];
    const int nchunks = (a.B + GW_KW - 1) / GW_KW;
    const int ch0 = (int)((int64_t)part * nchunks / a.n_parts), ch1 = (int)((int64_t)(part + 1) * nchunks / a.n_parts);
    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0, 0, 0, 0};
    f32x4 bsum = f32x4{0, 0, 0, 0};
    const int c = tid & 31, r0 = tid >> 5;   // staging: 32 chunks of 4 floats per row, 8 rows per pass
    for (int ch = ch0; ch < ch1; ++ch) {
        const int w0 = ch * GW_KW;
        for (int it = it0; it < it1; ++it) {
            const int* im = a.items + it * ITEM_INTS;
            const T* pb = reinterpret_cast<const T*>(a.ws + a.buf_off[im[0]]);
            const int ps = im[1], po = im[2], qbuf = im[3], qs = im[4], qo = im[5], qc0 = im[6], qn = im[7], so = im[8];
            f32x4 pv[4], qv[4];
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int row = r0 + 8 * p, w = w0 + row;
                pv[p] = f32x4{0, 0, 0, 0}; qv[p] = f32x4{0, 0, 0, 0};
                if (w < a.B) {
                    pv[p] = *reinterpret_cast<const f32x4*>(pb + act_idx(w, po, a.B) + c * 4);
                    if (im[9] >= 0) {   // P = dX_{l+1} . relu bits
                        const unsigned word = reinterpret_cast<const uint8_t*>(a.ws + a.buf_off[im[9]])[relu_byte(po, a.B, w, c * 4)];
                        pv[p] = __builtin_bit_cast(f32x4, chunk_mask_bits<float>(__builtin_bit_cast(u32x4, pv[p]), word >> ((c * 4) % 8)));
                    }
                    if (qs >= 0) {
                        qv[p] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const T*>(a.ws + a.buf_off[qbuf]) + act_idx(w, qo, a.B) + c * 4);
                    } else {
                        const int t = qbuf - BUF_IN;
                        const T* qq = reinterpret_cast<const T*>(a.x[t]) + ((size_t)w * a.nodes[t] + qo) * a.pitch[t] + qc0 + c * 4;
                        const u32x4 raw = load_chunk<T>(qq, qn - c * 4, a.vb[t]) ^ sign_xor<T>(a.signs + so + c * 4);
                        qv[p] = __builtin_bit_cast(f32x4, raw);
                    }
                }
            }
            __syncthreads();   // previous MFMA phase finished reading Ps/Qs
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int row = r0 + 8 * p;
                *reinterpret_cast<f32x4*>(&Ps[row * GW_PITCH + c * 4]) = pv[p];
                *reinterpret_cast<f32x4*>(&Qs[row * GW_PITCH + c * 4]) = qv[p];
                if (bias_flag) bsum += pv[p];
            }
            __syncthreads();
#pragma unroll
            for (int ks = 0; ks < GW_KW / 4; ++ks) {
                const int row = 4 * ks + (lane >> 4);
                float af[4], bq[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    af[i] = Ps[row * GW_PITCH + wr * 64 + i * 16 + (lane & 15)];
                    bq[i] = Qs[row * GW_PITCH + wc * 64 + i * 16 + (lane & 15)];
                }
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i], bq[j], acc[i][j], 0, 0, 0);
            }
        }
    }
    float* slab = a.slabs + (size_t)(part * a.n_lanes + ln) * SLAB_FLOATS;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int o = wr * 64 + i * 16 + ((lane >> 4) << 2) + q, k = wc * 64 + j * 16 + (lane & 15);
                slab[o * H + k] = acc[i][j][q];
            }
    if (bias_flag) {
        __syncthreads();
        *reinterpret_cast<f32x4*>(&Ps[r0 * GW_PITCH + c * 4]) = bsum;
        __syncthreads();
        if (tid < H) {
            float s = 0.f;
#pragma unroll
            for (int r = 0; r < 8; ++r) s += Ps[r * GW_PITCH + tid];
            slab[H * H + tid] = s;
        }
    }
}

#ifndef GW_WPS
#define GW_WPS 3
#endif

// k_gradw_bf16_lean: all weight gradients of the step as one split-K MFMA launch, dW[o][k] = sum_w P[w][o] Q[w][k] over 64-window steps staged through LDS (GWB_KW,
// tr_frag), with a hot path that issues almost nothing but loads, LDS traffic and MFMAs.  Its predecessor of rounds 1-3 (one thread per row, 64-bit row addresses, bound
// checks and per-row mask bytes) spent ~300 VALU instructions per wave and 64-window step on those (SQ counters: 29 M VALU instructions per launch against 1.4 M MFMAs);
// its shallow pipeline at 3 workgroups per CU (132 us) beat a two-stage one at 2 (153 us), hence GW_WPS.  Here a thread owns FOUR CONSECUTIVE windows of one 16-byte
// column chunk, so that
//   * every global address is  wave-uniform stream pointer (SGPRs, advanced by scalar adds)  +  per-thread 32-bit offset  +  immediate (256 p),
//   * the relu bytes of its four rows are ONE aligned 32-bit load (the byte layout keeps 16 consecutive windows together),
//   * full chunks (all but the last one of the batch) carry no bound checks.
// A lane holds up to GW_IPL items (all of one target: same operand kinds, same input column chunk), interleaved chunk by chunk into the same
// accumulators -- chunk-major, so that every workgroup of the launch sweeps the batch at the same pace and rows shared between lanes still meet in
// L2 (item-major order was measured: 109 -> 160 us, the sharing is lost; more than two items per lane lose it too, see GW_IPL_MAX).  The items'
// stream bases and sign masks sit in a small LDS table; a step reads its three 64-bit bases from it (broadcast reads, moved to scalar
// registers).  ALIGNED: raw inputs in the engine's own 16-byte-aligned layout; the other instantiation reads them element-wise.  32x32x16 bf16 MFMA,
// wave = 64x64 of the 128x128 tile.
// SERIES (with ALIGNED): a raw Q operand is gathered from the sequence's series like the encoder's input (k_enc_fwd<.., SERIES>): element k of a
// node row = element starts[w] + k % T of run k / T -- one unaligned 16-byte load per (window, chunk), two and a splice where the chunk straddles
// two runs; the four window starts of a thread are fetched one step ahead.  No materialised windows are read.
template <bool ALIGNED, bool SERIES = false> __global__ __launch_bounds__(256, GW_WPS) void k_gradw_bf16_lean(GradwArgs a) {
    static_assert(!SERIES || ALIGNED, "the series gather replaces the aligned raw loads");
    using T = __bf16;
    __shared__ __attribute__((aligned(16))) __bf16 Ps[GWB_KW * GWB_PITCH];
    __shared__ __attribute__((aligned(16))) __bf16 Qs[GWB_KW * GWB_PITCH];
    __shared__ __attribute__((aligned(16))) u32x4 mlut[256];       // relu byte -> AND mask of 8 bf16
    __shared__ __attribute__((aligned(16))) u32x4 qkeep_t[16];            // raw Q: keep mask (pad columns) of column chunk c (registers are short)
    __shared__ __attribute__((aligned(16))) u32x4 qsign_t[GW_IPL][16];    // raw Q: symmetry sign XOR of (item, column chunk)
    __shared__ unsigned long long sbase[GW_IPL][4];                       // per item: stream bases of P, relu bytes, Q at the part's first window
    __shared__ unsigned long long sser[SERIES ? GW_IPL : 1][16][2];       // SERIES, raw Q: per (item, column chunk) the run pointers (at the chunk's time offset) of its two pieces
    // extra workgroups carry the finalize ops that read no slab (zero fills, decoder sums, loss: GwSide): first in the grid, so that they run under the launch's body
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
    const int nchunks = (a.B + GWB_KW - 1) / GWB_KW;
    const int ch0 = (int)((int64_t)part * nchunks / a.n_parts), ch1 = (int)((int64_t)(part + 1) * nchunks / a.n_parts);
    const int nsteps = ch1 - ch0, total = nsteps * nit;
    const int c = tid & 15, r4 = (tid >> 4) * 4;      // rows r4 .. r4 + 3 of the 64-window step, columns [8c, 8c + 8)

    // what every item of the lane shares (one target): operand kinds, the input type and column chunk of a raw Q
    const bool p_masked = im0[9] >= 0, q_raw = im0[4] < 0;
    const int ntile = (a.B + 15) >> 4;
    const unsigned voffP = (unsigned)(r4 * H + c * 8) * (unsigned)sizeof(T);
    const unsigned voffM = (unsigned)(((c >> 2) * ntile + (r4 >> 4)) * 64 + (c & 3) * 16 + (r4 & 15));
    const int qt = q_raw ? im0[3] - BUF_IN : 0;
    const unsigned qsb = q_raw ? (unsigned)(a.nodes[qt] * a.pitch[qt]) * (unsigned)sizeof(T) : (unsigned)(H * sizeof(T));
    const int qn = q_raw ? im0[7] - c * 8 : 8, qvb = q_raw ? a.vb[qt] : 16;
    const unsigned voffQ0 = (unsigned)r4 * qsb + (unsigned)c * 16u;
    unsigned ldsw[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) ldsw[p] = (unsigned)gwb_elem(r4 + p, c * 8);
    if (tid < 16) qkeep_t[tid] = chunk_keep_first<T>(u32x4{0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu}, qn);      // (tid == c)
    if (tid < nit) {     // thread k resolves item k's stream bases (at the part's first window)
        const int* im = a.items + (it0 + tid) * ITEM_INTS;
        sbase[tid][0] = (unsigned long long)(a.ws + a.buf_off[im[0]] + (act_idx(0, im[2], a.B) + (size_t)ch0 * GWB_KW * H) * sizeof(T));
        sbase[tid][1] = p_masked ? (unsigned long long)(a.ws + a.buf_off[im[9]] + relu_byte(im[2], a.B, 0, 0) + (size_t)ch0 * (GWB_KW / 16) * 64) : 0ull;
        sbase[tid][2] = q_raw ? (unsigned long long)(reinterpret_cast<const char*>(a.x[qt]) + ((size_t)im[5] * a.pitch[qt] + im[6]) * sizeof(T) + (size_t)ch0 * GWB_KW * qsb)
                              : (unsigned long long)(a.ws + a.buf_off[im[3]] + (act_idx(0, im[5], a.B) + (size_t)ch0 * GWB_KW * H) * sizeof(T));
    }
    if (q_raw && tid < nit * 16) {
        const int* im = a.items + (it0 + (tid >> 4)) * ITEM_INTS;
        qsign_t[tid >> 4][c] = sign_xor<T>(a.signs + im[8] + c * 8);
        if constexpr (SERIES) {      // elements [k0, k0 + 8) of the node row: n0 from run j at time offset off, the rest from run j + 1 at offset 0
            const int k0 = im[6] + c * 8, j = k0 / a.ser.T, off = k0 - j * a.ser.T, n0 = min(8, a.ser.T - off);
            const int rfirst = a.ser.rows[2 * (a.ser.row0[qt] + im[5])];
            unsigned long long pa = qn > 0 ? a.ser.run_ptr[rfirst + j] : 0ull, pb = min(qn, 8) > n0 ? a.ser.run_ptr[rfirst + j + 1] : 0ull;
            // negated runs (RUN_PTR_SIGN): the chunk's per-element sign mask joins the symmetry mask of (item, chunk) -- nothing changes in the loop
            if ((pa | pb) & RUN_PTR_SIGN) qsign_t[tid >> 4][c] ^= chunk_keep_first<T>(sign_mask8_bf16(n0, (pa & RUN_PTR_SIGN) != 0, (pb & RUN_PTR_SIGN) != 0), qn);
            pa = run_ptr_addr(pa); pb = run_ptr_addr(pb);
            sser[tid >> 4][c][0] = pa ? pa + (unsigned long long)off * sizeof(T) : 0ull;
            sser[tid >> 4][c][1] = pb;
        }
    }
    int s_n0 = 8; bool s_two = false;      // SERIES: this thread's chunk takes n0 elements from its first run; a second piece exists
    if constexpr (SERIES) { if (q_raw) { const int k0 = im0[6] + c * 8, off = k0 % a.ser.T; s_n0 = min(8, a.ser.T - off); s_two = min(qn, 8) > s_n0; } }
    __syncthreads();
    const char* pS = a.ws; const char* mS = a.ws; const char* qS = a.ws;
    auto ubase = [&](int k, int j, size_t off) -> const char* {      // wave-uniform 64-bit pointer out of the LDS table
        const unsigned long long v = sbase[k][j] + off;
        return reinterpret_cast<const char*>(((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32) |
                                             (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v));
    };
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

    u32x4 pv[4], qv[4]; unsigned mw = 0xffffffffu;
    int nk = 0, nc = 0;            // (item, chunk of the part) of the next fetch: items interleaved chunk by chunk
    int wst[SERIES ? 4 : 1];      // SERIES: first series row of the four windows of the NEXT fetch (loaded one step ahead)
    auto load_starts = [&](int chunk) {
        if constexpr (SERIES) {
            if (q_raw) {
#pragma unroll
                for (int p = 0; p < 4; ++p) wst[p] = (int)a.ser.starts[min((ch0 + chunk) * GWB_KW + r4 + p, a.B - 1)];
            }
        }
    };
    auto load_q = [&](int p) -> u32x4 {
        if constexpr (SERIES) {
            if (q_raw) {
                const u32x4 ones = u32x4{0x3f803f80u, 0x3f803f80u, 0x3f803f80u, 0x3f803f80u};      // the constant-1 run (bf16 1.0)
                const unsigned long long pa = sser[nk][c][0];
                u32x4 va = ones;
                if (pa) va = *reinterpret_cast<const u32x4*>(reinterpret_cast<const T*>(pa) + wst[p]);
                if (s_two) {
                    const unsigned long long pb = sser[nk][c][1];
                    u32x4 vb2 = ones;
                    if (pb) vb2 = *reinterpret_cast<const u32x4*>(reinterpret_cast<const T*>(pb) + wst[p]);
                    va = splice8(va, vb2, s_n0);
                }
                return va;
            }
        }
        if constexpr (ALIGNED) return *reinterpret_cast<const u32x4*>(qS + voffQ0 + p * qsb);
        else return q_raw ? load_chunk<T>(reinterpret_cast<const T*>(qS + voffQ0 + p * qsb), qn, qvb) : *reinterpret_cast<const u32x4*>(qS + voffQ0 + p * qsb);
    };
    auto fetch = [&]() {
        pS = ubase(nk, 0, (size_t)nc * GWB_KW * H * sizeof(T));
        if (p_masked) mS = ubase(nk, 1, (size_t)nc * (GWB_KW / 16) * 64);
        qS = ubase(nk, 2, (size_t)nc * GWB_KW * qsb);
        const int w0 = (ch0 + nc) * GWB_KW;
        if (w0 + GWB_KW <= a.B) {
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                pv[p] = *reinterpret_cast<const u32x4*>(pS + voffP + p * (int)(H * sizeof(T)));
                qv[p] = u32x4{0, 0, 0, 0};
                if (qn > 0) qv[p] = load_q(p);
            }
            if (p_masked) mw = *reinterpret_cast<const unsigned*>(mS + voffM);
        } else {                   // last chunk of the batch: rows beyond B are zero
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                pv[p] = u32x4{0, 0, 0, 0}; qv[p] = u32x4{0, 0, 0, 0};
                if (w0 + r4 + p < a.B) {
                    pv[p] = *reinterpret_cast<const u32x4*>(pS + voffP + p * (int)(H * sizeof(T)));
                    if (qn > 0) qv[p] = load_q(p);
                }
            }
            mw = 0xffffffffu;
            if (p_masked && w0 + r4 < a.B) mw = *reinterpret_cast<const unsigned*>(mS + voffM);     // (the 16-window tile of row r4 exists)
        }
        if (++nk == nit) { nk = 0; ++nc; if (nc < nsteps) load_starts(nc); }      // (the next chunk's window starts: used by the fetch after this one)
    };
    int sk = 0;                    // item of the step being staged
    auto stage_to_lds = [&]() {
        u32x4 mk[4], qkeep, sx;
        if (q_raw) { qkeep = qkeep_t[c]; sx = qsign_t[sk][c]; }
        if (++sk == nit) sk = 0;
        if (p_masked) {              // the four table reads go out together (one LDS round trip, not four)
#pragma unroll
            for (int p = 0; p < 4; ++p) mk[p] = mlut[(mw >> (8 * p)) & 0xffu];
        }
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            u32x4 pm = pv[p];
            if (p_masked) pm &= mk[p];                                   // dH = dX . relu bits
            *reinterpret_cast<u32x4*>(&Ps[ldsw[p]]) = pm;
            u32x4 qm = qv[p];
            if (q_raw) qm = (qm & qkeep) ^ sx;                           // drop pad columns, symmetry sign mask of encoder inputs
            *reinterpret_cast<u32x4*>(&Qs[ldsw[p]]) = qm;
            if (bias_flag) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    bsum[2 * e] += __builtin_bit_cast(float, pm[e] << 16);
                    bsum[2 * e + 1] += __builtin_bit_cast(float, pm[e] & 0xffff0000u);
                }
            }
        }
    };
    if (total > 0) { load_starts(0); fetch(); }
    for (int s = 0; s < total; ++s) {
        __syncthreads();             // every wave is done with the previous step's tiles
        stage_to_lds();
        __syncthreads();
        if (s + 1 < total) fetch();
#pragma unroll
        for (int ks = 0; ks < GWB_KW / 16; ++ks) {
            bf16x8 af[2], bq[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                af[i] = tr_frag(Ps, ks * 16, wr * 64 + i * 32, lane);
                bq[i] = tr_frag(Qs, ks * 16, wc * 64 + i * 32, lane);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], bq[j], acc[i][j], 0, 0, 0);
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
        float* red = reinterpret_cast<float*>(Ps);   // 16 x 128 floats = 8 KB <= one tile
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 8; ++e) red[(r4 >> 2) * H + c * 8 + e] = bsum[e];
        __syncthreads();
        if (tid < H) {
            float s2 = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) s2 += red[r * H + tid];
            slab[H * H + tid] = s2;
        }
    }
}

// finalize: sum split-K slabs in fixed order into the flat gradient buffer (every parameter written once)

#ifndef FIN_LB
#define FIN_LB 4       // lanes per load batch of the finalize kernels (x 4 parts = 16 slab loads in flight per thread; 8 / 16 lanes measured on the whole finalize: A1-C2 18.7 ->
                       // 18.6 / 17.9 us, MiniCheetah-K4 L=8 19.3 -> 20.5 / 23.6 us)
#endif
// k_finalize (bf16 / split plans): the slab sums and nothing else -- the ops that read no slab ran in the weight-gradient launch (gw_side_workgroup).  One FSLAB_INTS
// record per workgroup, so the first load behind the record is slab data; a thread owns FOUR CONSECUTIVE columns of one destination row (slab rows are H floats: 16-byte
// loads) and sums each of them exactly as the whole finalize below does: lane-major batches of FIN_LB lanes x 4 parts, (v0 + v1) + (v2 + v3) per lane.
__global__ __launch_bounds__(256) void k_finalize(FinSlabArgs a) {
    const int* f = a.recs + (size_t)blockIdx.x * FSLAB_INTS;
    const int64_t dst = (int64_t)(unsigned)f[0] | ((int64_t)f[1] << 32);
    const int row0 = f[2], rows = f[3], cols = f[4], ld = f[5], l0 = f[6], nl = f[7], kind = f[9];
    const int* more = f[8] ? a.fin0 + f[8] : nullptr;      // further destinations of the same sum: {n, dst_lo, dst_hi, ...}
    const int rr = threadIdx.x >> 5, c0 = (threadIdx.x & 31) * 4;
    if (rr >= rows || c0 >= cols) return;
    const int r = row0 + rr;
    const float* sp = a.slabs + (size_t)l0 * SLAB_FLOATS + (kind == FIN_MATRIX ? r * H : H * H) + c0;
    const size_t pstride = (size_t)a.n_lanes * SLAB_FLOATS;
    float4 s = float4{0.f, 0.f, 0.f, 0.f};
    for (int j0 = 0; j0 < nl; j0 += FIN_LB)
        for (int p0 = 0; p0 < a.n_parts; p0 += 4) {
            float4 v[FIN_LB][4];
#pragma unroll
            for (int jj = 0; jj < FIN_LB; ++jj)
#pragma unroll
                for (int pp = 0; pp < 4; ++pp)
                    v[jj][pp] = (j0 + jj < nl && p0 + pp < a.n_parts) ? *reinterpret_cast<const float4*>(sp + (size_t)(j0 + jj) * SLAB_FLOATS + (size_t)(p0 + pp) * pstride)
                                                                       : float4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int jj = 0; jj < FIN_LB; ++jj) {
                s.x += (v[jj][0].x + v[jj][1].x) + (v[jj][2].x + v[jj][3].x);
                s.y += (v[jj][0].y + v[jj][1].y) + (v[jj][2].y + v[jj][3].y);
                s.z += (v[jj][0].z + v[jj][1].z) + (v[jj][2].z + v[jj][3].z);
                s.w += (v[jj][0].w + v[jj][1].w) + (v[jj][2].w + v[jj][3].w);
            }
        }
    const int64_t at = (int64_t)r * ld + c0;
    float* g = a.grad + dst + at;
    // stores as wide as the destination allows: encoder chunks have widths such as 66 and leading dimension 450 (scalar stores there)
    const bool full = c0 + 4 <= cols;
    float e[4] = {s.x, s.y, s.z, s.w};
    if (a.accumulate) {      // (a later sub-step of a chunked step; the further destinations of a shared sum held the same value)
#pragma unroll
        for (int k = 0; k < 4; ++k) if (c0 + k < cols) e[k] += g[k];
    }
    auto put = [&](float* q) {
        if (full && ((uintptr_t)q & 15) == 0) *reinterpret_cast<float4*>(q) = float4{e[0], e[1], e[2], e[3]};
        else {
#pragma unroll
            for (int k = 0; k < 4; ++k) if (c0 + k < cols) q[k] = e[k];
        }
    };
    put(g);
    if (more) {
        const int nm = more[0];
        for (int m = 0; m < nm; ++m) put(a.grad + (((int64_t)(unsigned)more[1 + 2 * m] | ((int64_t)more[2 + 2 * m] << 32)) + at));
    }
}

// k_finalize_whole (fp32 plan; the loss alone of an activation-only backward on every plan): every op of the fin table, 64 workgroups per op
__global__ __launch_bounds__(256) void k_finalize_whole(FinArgs a) {
    const int* f = a.fin + blockIdx.x * FIN_INTS;
    const int64_t dst = (int64_t)(unsigned)f[0] | ((int64_t)f[1] << 32);
    const int rows = f[2], cols = f[3], ld = f[4], tg = f[5], kind = f[6];
    const int* more = f[7] ? a.fin0 + f[7] : nullptr;      // further destinations of the same sum: {n, dst_lo, dst_hi, ...}
    const int RPB = (rows + gridDim.y - 1) / gridDim.y;
    const int r0 = blockIdx.y * RPB, r1 = min(rows, r0 + RPB);
    const int n = (r1 - r0) * cols;
    if (a.loss && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x < 64) {   // fused MSE: sum the per-block loss partials
        float l = 0.f;
        for (int b = threadIdx.x; b < a.n_dec; b += 64) l += a.dec_slabs[(size_t)b * DEC_SLAB_FLOATS + 8 * H + 8];
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) l += __shfl_xor(l, m, 64);
        if (threadIdx.x == 0) *a.loss = l * a.inv_n + (a.accumulate ? *a.loss : 0.f);      // (accumulate: a later sub-step of a chunked step, mshgnn_device.hpp StepChunk)
    }
    if (!a.grad) return;      // (the loss alone: a backward without parameter gradients)
    const bool is_mat = (kind == FIN_MATRIX || kind == FIN_DEC_W);
    if (kind == FIN_DEC_W || kind == FIN_DEC_B) {
        // decoder partials: NWG_DEC slabs per element -> one WAVE per element, 8 slabs per lane in flight, then a fixed
        // xor-shuffle tree (deterministic); elements are dealt round-robin to the (gridDim.y x 4) waves of this op
        const int lane = threadIdx.x & 63, wave = blockIdx.y * 4 + (threadIdx.x >> 6), nwaves = gridDim.y * 4;
        for (int e = wave; e < rows * cols; e += nwaves) {
            const int r = e / cols, cidx = e % cols;
            const int src = is_mat ? r * H + cidx : 8 * H + cidx;
            float sum = 0.f;
            for (int b0 = 0; b0 < a.n_dec; b0 += 512) {       // 8 slabs per lane in flight; lane-strided, fixed order
                float v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) { const int b = b0 + lane + 64 * u; v[u] = b < a.n_dec ? a.dec_slabs[(size_t)b * DEC_SLAB_FLOATS + src] : 0.f; }
                sum += ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
            }
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) sum += __shfl_xor(sum, m, 64);
            if (lane == 0) { float* gp = a.grad + dst + (int64_t)r * ld + cidx; *gp = a.accumulate ? *gp + sum : sum; }
        }
        return;
    }
    if (n <= 0) return;
    for (int i = threadIdx.x; i < n; i += 256) {
        const int r = r0 + i / cols, cidx = i % cols;
        float s = 0.f;
        if (kind == FIN_MATRIX || kind == FIN_BIAS) {
            const int src = is_mat ? r * H + cidx : H * H + cidx;
            const int l0 = a.targets[tg * TGT_INTS], nl = a.targets[tg * TGT_INTS + 1] - l0;
            // slab(part, j) = part * n_lanes + l0 + j; summed lane-major in batches of 16 loads -- fixed summation order
            const float* sp = a.slabs + (size_t)l0 * SLAB_FLOATS + src;
            const size_t pstride = (size_t)a.n_lanes * SLAB_FLOATS;
            for (int j0 = 0; j0 < nl; j0 += FIN_LB)
                for (int p0 = 0; p0 < a.n_parts; p0 += 4) {
                    float v[FIN_LB][4];
#pragma unroll
                    for (int jj = 0; jj < FIN_LB; ++jj)
#pragma unroll
                        for (int pp = 0; pp < 4; ++pp)
                            v[jj][pp] = (j0 + jj < nl && p0 + pp < a.n_parts) ? sp[(size_t)(j0 + jj) * SLAB_FLOATS + (size_t)(p0 + pp) * pstride] : 0.f;
#pragma unroll
                    for (int jj = 0; jj < FIN_LB; ++jj) s += (v[jj][0] + v[jj][1]) + (v[jj][2] + v[jj][3]);
                }
        }
        if (a.accumulate) s += a.grad[dst + (int64_t)r * ld + cidx];      // (the further destinations of a shared sum held the same value)
        a.grad[dst + (int64_t)r * ld + cidx] = s;
        if (more) {
            const int nm = more[0];
            for (int k = 0; k < nm; ++k) a.grad[((int64_t)(unsigned)more[1 + 2 * k] | ((int64_t)more[2 + 2 * k] << 32)) + (int64_t)r * ld + cidx] = s;
        }
    }
}

// ------------------------------------------------------------------------------------------------------
// Launch tables: row k of a family is what pick_stack / pick_enc (mshgnn_pick.hpp) call k.  Which row a launch takes is decided there and nowhere else.
// ------------------------------------------------------------------------------------------------------
static constexpr StackKernel STACK8_TABLE[pick::STACK8_ROWS] = {k_stack_fwd<__bf16>, k_stack_bwd<__bf16>, k_stack_step<__bf16>};
#define SLAB_ROWS_OF(K) K<__bf16, 2, SL_HB>, K<__bf16, 2, SL_HB_MAX>, K<__bf16, 4, SL_HB>, K<__bf16, 4, SL_HB_MAX>
static constexpr StackKernel SLAB_TABLE[pick::SLAB_ROWS] = {SLAB_ROWS_OF(k_slab_fwd), SLAB_ROWS_OF(k_slab_bwd), SLAB_ROWS_OF(k_slab_step)};      // [what][NM][HB]: pick::slab_row
#undef SLAB_ROWS_OF
static_assert(pick::STACK8_THREADS == LAYER_THREADS, "the pick's block size of the 8-wave kernels");
// the encoder of the fp32 / bf16 plans by pick::EncForm; the fp32 plan has no source routes (plan_traits<float>.src_routes is false: pick_enc never names those rows)
using EncKernel = void (*)(EncArgs, SeriesSrc, WideSrc);
template <typename T> static constexpr EncKernel ENC_TABLE[pick::ENC_FORMS] = {k_enc_fwd<T, false>, k_enc_fwd<T, true>};
template <> constexpr EncKernel ENC_TABLE<__bf16>[pick::ENC_FORMS] = {
    k_enc_fwd<__bf16, false>, k_enc_fwd<__bf16, true>, k_enc_fwd<__bf16, true, false, 4>, k_enc_fwd<__bf16, true, false, 8>,
    k_enc_fwd<__bf16, true, true>, k_enc_fwd<__bf16, true, true, 0, true>, k_enc_fwd<__bf16, true, true, 0, false, true>, k_enc_fwd<__bf16, true, true, 0, true, true>,
    k_enc_fwd<__bf16, true, true, 0, false, true, true>, k_enc_fwd<__bf16, true, true, 0, true, true, true>};
// the kernels over the plan's compile-time program: row `form` (pick::SpecForm) of the table of the shard -- or of the program attached after the build -- whose tables
// are the plan's; name: that program's
using SpecSelector = StackKernel (*)(const HostPlan& hp, int form, const char** name);
static StackKernel spec_kernel(const HostPlan& hp, int form, const char** name = nullptr) {
    const char* nm = nullptr;
    if (hp.jit_prog) {             // a program compiled for this plan after the build
        StackKernel kk = reinterpret_cast<SpecSelector>(hp.jit_prog)(hp, form, &nm);
        if (nm) { if (name) *name = nm; return kk; }
    }
#define SPEC_SHARD_TRY(k) { StackKernel kk = spec_shard##k(hp, form, &nm); if (nm) { if (name) *name = nm; return kk; } }
    SPEC_SHARD_LIST(SPEC_SHARD_TRY)
#undef SPEC_SHARD_TRY
    return nullptr;
}
static StackKernel stack_kernel(const HostPlan& hp, const pick::StackPick& pk) {
    return pk.family == pick::STACK8 ? STACK8_TABLE[pk.k] : pk.family == pick::SLAB ? SLAB_TABLE[pk.k] : pk.family == pick::SLAB_SPEC ? spec_kernel(hp, pk.k) : nullptr;
}
template <typename K, size_t N> static int set_lds_attrs(const K (&table)[N], int bytes) {      // every row a table has
    for (K k : table) if (k) if (int rc = set_lds_attr(k, bytes)) return rc;
    return MSHGNN_OK;
}

// ------------------------------------------------------------------------------------------------------
// plan object + C-ABI
// ------------------------------------------------------------------------------------------------------

// the kernels over this plan's compile-time program, if one exists (built in, or attached): their dynamic-LDS attribute, the program's name; else use_spec = false
static int set_spec_attrs(mshgnn_plan* p, int flds) {
    const char* nm = nullptr;
    for (int form = 0; form < pick::SPEC_FORMS; ++form)
        if (StackKernel k = spec_kernel(p->hp, form, &nm)) { if (int rc = set_lds_attr(k, flds)) return rc; } else if (!nm) break;      // (no program: no form)
    if (!nm) { p->use_spec = false; return MSHGNN_OK; }
    p->spec_name_buf = strncmp(nm, "spec::", 6) == 0 ? nm + 6 : nm;
    p->spec_name = p->spec_name_buf.c_str();
    return MSHGNN_OK;
}

// A program compiled for this plan after the library was built (morphsym_hgnn_amd/jit.py: this source as shard 99 over the plan's own tables): `selector` is that
// library's mshgnn_jit_program.  Only LDS-resident bf16 plans whose slab kernels are in use take one; the tables are compared like a built-in program's.
extern "C" int mshgnn_plan_attach_program(mshgnn_plan* p, void* selector) {
    if (!p || !selector) return set_err(MSHGNN_EINVAL, "plan or selector is null");
    if (!p->gen && p->hp.d.dtype == MSHGNN_BF16X3) return x3_attach_program(p, selector);      // (the split plan: selector = mshgnn_jit_program_x3)
    if (p->gen || p->hp.d.dtype != MSHGNN_BF16 || !p->use_fused || !p->use_slab) return set_err(MSHGNN_EINVAL, "attached programs exist for LDS-resident bf16 / split-bf16 plans (bf16: on the slab kernels) only");
    void* const prev = p->hp.jit_prog;
    p->hp.jit_prog = selector;
    const char* nm = nullptr;
    if (!reinterpret_cast<SpecSelector>(selector)(p->hp, pick::SF_STEP, &nm) || !nm) {
        p->hp.jit_prog = prev;
        return set_err(MSHGNN_EINVAL, "the program's tables are not this plan's");
    }
    p->use_spec = true;
    const int rc = set_spec_attrs(p, (p->hp.fs_blk + FS_EXTRA_BLK) * Prec<__bf16>::BLK);
    if (rc || !p->use_spec) { p->hp.jit_prog = prev; p->use_spec = false; return rc ? rc : set_err(MSHGNN_EINVAL, "no kernel of the attached program could be used"); }
    return MSHGNN_OK;
}

extern "C" int mshgnn_plan_create(const mshgnn_desc* desc, mshgnn_plan** out) {
    if (!out) return set_err(MSHGNN_EINVAL, "plan_out is null");
    *out = nullptr;
    mshgnn_plan* p = new (std::nothrow) mshgnn_plan();
    if (!p) return set_err(MSHGNN_ENOMEM, "out of host memory");
    if (!desc) { delete p; return set_err(MSHGNN_EINVAL, "null descriptor"); }
    p->n_types = desc->n_types;
    if (const char* e = getenv("MSHGNN_STEP_CHUNK")) p->step_chunk = std::max<int64_t>(0, atoll(e));
    if (const char* e = getenv("MSHGNN_STASH_NT")) p->stash_nt_force = atoi(e);      // (read per plan, like MSHGNN_SLAB / SPEC / FUSED)
    // Engine choice: the LDS-resident kernels (hidden == 128, <= 20 nodes, in-degree 1 on mean relations) where they apply, else the
    // generic-width engine of mshgnn_gen.hip.  MSHGNN_ENGINE=generic forces the latter (the GPU tests run the golden cases through both).
    const char* eng_env = getenv("MSHGNN_ENGINE");
    bool want_gen = eng_env && std::string(eng_env) == "generic";
    std::string why;
    if (!want_gen && !compile_plan(desc, p->hp)) {
        why = p->hp.err;
        const bool unsup = why.find("supports") != std::string::npos || why.find("not supported") != std::string::npos || why.find("too many") != std::string::npos;
        if (!unsup) { delete p; return set_err(MSHGNN_EINVAL, why); }
        want_gen = true;
    }
    if (want_gen) {
        int ndev0 = 0;
        if (hipGetDeviceCount(&ndev0) != hipSuccess || ndev0 == 0) { delete p; return set_err(MSHGNN_EHIP, "no HIP device: the MS-HGNN engine has no CPU fallback"); }
        const int rc = gen_create(p, desc);
        if (rc) {
            const std::string m = g_err; gen_destroy(p); delete p;
            return set_err(rc, why.empty() ? m : why + "; generic-width engine: " + m);
        }
#ifdef MSHGNN_ABLATE
        { const char* e = getenv("MSHGNN_DBG"); p->dbg = e ? atoi(e) : 0; }
#endif
        if (!p->hp.d.n_types) {      // forced generic engine: the specialised compiler never ran; entry points read the scalar fields from here
            p->hp.d = *desc;         // (its host pointers belong to the caller and are not read again)
        }
        *out = p;
        return MSHGNN_OK;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        delete p; return set_err(MSHGNN_EHIP, "no HIP device: the MS-HGNN engine has no CPU fallback");
    }
#ifdef MSHGNN_ABLATE
    { const char* e = getenv("MSHGNN_DBG"); p->dbg = e ? atoi(e) : 0; }
#endif
    HostPlan& hp = p->hp;
    auto up = [&](void** dptr, const void* src, size_t bytes) -> int {
        HIPCHK(hipMalloc(dptr, std::max<size_t>(bytes, 16)));
        if (bytes) HIPCHK(hipMemcpy(*dptr, src, bytes, hipMemcpyHostToDevice));
        return MSHGNN_OK;
    };
    int rc;
    if ((rc = up((void**)&p->d_tables, hp.tables.data(), hp.tables.size() * 4)) != 0 ||
        (rc = up((void**)&p->d_signs, hp.signs.data(), hp.signs.size())) != 0 ||
        (rc = up((void**)&p->d_out_mask, hp.out_mask_f.data(), hp.out_mask_f.size() * 4)) != 0 ||
        (rc = up((void**)&p->d_packs, hp.packs.data(), hp.packs.size() * sizeof(PackDesc))) != 0 ||
        (rc = up((void**)&p->d_biases, hp.biases.data(), hp.biases.size() * sizeof(BiasDesc))) != 0) {
        mshgnn_plan_destroy(p); return rc;
    }
    const int lds = hp.n_blk * hp.blk_bytes;
    if (hp.d.dtype == MSHGNN_BF16X3) {
        p->use_fused = true;      // the split plan has only the fused 8-wave stack kernels (mshgnn_x3.hip)
        { const char* et = getenv("MSHGNN_STEP_KERNEL"); p->use_step = !(et && atoi(et) == 0); }      // read per plan, as on the bf16 plan
        if ((rc = x3_set_attrs(p))) { mshgnn_plan_destroy(p); return rc; }
    } else if (hp.d.dtype == MSHGNN_F32) {
        if ((rc = set_lds_attr(k_layer_fwd<float>, lds)) || (rc = set_lds_attr(k_layer_bwd<float>, lds)) ||
            (rc = set_lds_attrs(ENC_TABLE<float>, Prec<float>::ENC_MB * Prec<float>::BLK))) { mshgnn_plan_destroy(p); return rc; }
    } else {
        if ((rc = set_lds_attr(k_layer_fwd<__bf16>, lds)) || (rc = set_lds_attr(k_layer_bwd<__bf16>, lds)) ||
            (rc = set_lds_attrs(ENC_TABLE<__bf16>, Prec<__bf16>::ENC_MB * Prec<__bf16>::BLK))) { mshgnn_plan_destroy(p); return rc; }
        const char* e = getenv("MSHGNN_FUSED");
        p->use_fused = hp.fused && !(e && atoi(e) == 0);
        if (p->use_fused) {
            const int flds = (hp.fs_blk + FS_EXTRA_BLK) * Prec<__bf16>::BLK;
            if ((rc = set_lds_attrs(STACK8_TABLE, flds))) { mshgnn_plan_destroy(p); return rc; }
            const char* es = getenv("MSHGNN_SLAB");
            p->use_slab = hp.slab && !(es && atoi(es) == 0);       // default on where the plan allows it; MSHGNN_SLAB=0 selects the 8-wave kernels
            p->slab_force = es && atoi(es) == 2;                   // MSHGNN_SLAB=2: also for batches that do not fill the chip
            { int dev = 0, cus = 256; if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev); p->n_cu = cus > 0 ? cus : 256; }
            if (p->use_slab && (rc = set_lds_attrs(SLAB_TABLE, flds))) { mshgnn_plan_destroy(p); return rc; }
            { const char* esp = getenv("MSHGNN_SPEC"); p->use_spec = p->use_slab && !(esp && atoi(esp) == 0); }
            if (p->use_spec && (rc = set_spec_attrs(p, flds))) { mshgnn_plan_destroy(p); return rc; }
            { const char* et = getenv("MSHGNN_STEP_KERNEL"); p->use_step = !(et && atoi(et) == 0); }      // one-call steps: forward + backward sweep in one launch

            { const char* eg = TUNE_ENV("MSHGNN_STAGGER"); p->stagger = eg ? atoi(eg) : 0; }
        }
    }
    *out = p;
    return MSHGNN_OK;
}

extern "C" void mshgnn_plan_destroy(mshgnn_plan* p) {
    if (!p) return;
    gen_destroy(p);
    if (p->d_tables) (void)hipFree(p->d_tables);
    if (p->d_signs) (void)hipFree(p->d_signs);
    if (p->d_out_mask) (void)hipFree(p->d_out_mask);
    if (p->d_packs) (void)hipFree(p->d_packs);
    if (p->d_biases) (void)hipFree(p->d_biases);
    if (p->d_ig_nodes) (void)hipFree(p->d_ig_nodes);
    for (ProfRec& r : p->recs) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    for (hipEvent_t e : p->free_events) (void)hipEventDestroy(e);
    delete p;
}

extern "C" int mshgnn_profile_enable(mshgnn_plan* p, int on) {
    if (!p) return set_err(MSHGNN_EINVAL, "null plan");
    p->prof = on != 0;
    return MSHGNN_OK;
}

extern "C" int mshgnn_profile_read(mshgnn_plan* p, mshgnn_kernel_stat* stats, int32_t* n_inout) {
    if (!p || !stats || !n_inout) return set_err(MSHGNN_EINVAL, "null argument");
    std::vector<mshgnn_kernel_stat> ks = p->gen ? *gen_kstats(p) : p->hp.kstats;
    for (const ProfRec& r : p->recs) {
        HIPCHK(hipEventSynchronize(r.b));
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, r.a, r.b));
        if (r.slot >= 0 && r.slot < (int)ks.size()) { ks[r.slot].total_ms += ms; ks[r.slot].launches += 1; }
        p->free_events.push_back(r.a); p->free_events.push_back(r.b);
    }
    p->recs.clear();
    const int n = std::min<int>(*n_inout, (int)ks.size());
    for (int i = 0; i < n; ++i) stats[i] = ks[i];
    *n_inout = n;
    return MSHGNN_OK;
}

extern "C" const char* mshgnn_plan_specialised(const mshgnn_plan* p) { return p && !p->gen && p->use_spec ? p->spec_name : ""; }

// The regression loss of the plan's `mse` entry points (include/mshgnn.h): checked here, read by value when a call is made (backward_mse, step_call, step_series).
int check_regression_loss(int kind, float delta, const char* who) {
    if (kind != MSHGNN_REG_LOSS_MSE && kind != MSHGNN_REG_LOSS_L1 && kind != MSHGNN_REG_LOSS_HUBER)
        return set_err(MSHGNN_EINVAL, std::string(who) + ": kind must be MSHGNN_REG_LOSS_MSE, _L1 or _HUBER");
    if (kind == MSHGNN_REG_LOSS_HUBER && !(std::isfinite(delta) && delta > 0.f)) return set_err(MSHGNN_EINVAL, std::string(who) + ": Huber's delta must be finite and > 0");
    return MSHGNN_OK;
}
extern "C" int mshgnn_plan_set_regression_loss(mshgnn_plan* p, int kind, float delta) {
    if (!p) return set_err(MSHGNN_EINVAL, "null argument to mshgnn_plan_set_regression_loss");
    if (const int rc = check_regression_loss(kind, delta, "mshgnn_plan_set_regression_loss")) return rc;
    p->reg_kind = kind; p->reg_delta = kind == MSHGNN_REG_LOSS_HUBER ? delta : 1.0f;
    return MSHGNN_OK;
}
extern "C" int mshgnn_plan_get_regression_loss(const mshgnn_plan* p, int32_t* kind_out, float* delta_out) {
    if (!p || !kind_out || !delta_out) return set_err(MSHGNN_EINVAL, "null argument to mshgnn_plan_get_regression_loss");
    *kind_out = p->reg_kind; *delta_out = p->reg_delta;
    return MSHGNN_OK;
}
extern "C" int mshgnn_plan_info(const mshgnn_plan* p, mshgnn_info* info) {
    if (!p || !info) return set_err(MSHGNN_EINVAL, "null argument");
    *info = p->gen ? *gen_info(p) : p->hp.info;
    return MSHGNN_OK;
}

// host-only plan compilation (no GPU needed): used by the CPU test-suite to check the plan compiler
extern "C" int mshgnn_plan_compile_host(const mshgnn_desc* desc, mshgnn_info* info, int32_t* n_tables_out) {
    HostPlan hp;
    const char* eng_env = getenv("MSHGNN_ENGINE");
    if ((eng_env && std::string(eng_env) == "generic") || !compile_plan(desc, hp)) {
        const std::string why = hp.err;
        if (gen_host_compile(desc, info, n_tables_out) == MSHGNN_OK) return MSHGNN_OK;
        return set_err(MSHGNN_EINVAL, why.empty() ? g_err : why + "; generic-width engine: " + g_err);
    }
    if (info) *info = hp.info;
    if (n_tables_out) *n_tables_out = (int32_t)hp.tables.size();
    return MSHGNN_OK;
}

extern "C" int mshgnn_workspace_layout(const mshgnn_plan* p, int64_t batch, int training, mshgnn_ws_layout* out) {
    if (!p || !out || batch < 1) return set_err(MSHGNN_EINVAL, "bad argument to mshgnn_workspace_layout");
    if (p->gen) gen_layout(p, batch, training, out); else layout_workspace(p->hp, batch, training, out);
    return MSHGNN_OK;
}

// the weight-image launch of a plan of element type T: the tiled kernel from PREP_TILED_MIN packs up, else one thread per output vector of the launch's packs
template <typename T> static void launch_prep_t(const PrepArgs& a, bool biases, hipStream_t st) {
    if (prep_use_tiled(a.n_packs)) hipLaunchKernelGGL((k_prep_tiled<T, false>), dim3(prep_tiled_grid(a.n_packs, a.n_biases)), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((k_prep<T, false>), dim3(prep_grid(a, Prec<T>::EPC, biases)), dim3(256), 0, st, a);
}
int launch_prep(const PrepArgs& a, bool split, hipStream_t st) {
    if (split) x3_launch_prep(a, true, st); else launch_prep_t<__bf16>(a, true, st);
    return MSHGNN_OK;
}

int run_finalize(const mshgnn_plan* p, const StepCall& c, const mshgnn_ws_layout& lay, int gw_parts) {
    const HostPlan& hp = p->hp;
    const mshgnn_desc& d = hp.d;
    char* ws = c.ws; float* gparams = c.grad_params; hipStream_t st = c.stream;
    const int B = (int)c.batch, gw_phase = c.gw_phase;
    float* loss = c.loss != LossKind::NONE ? c.loss_out : nullptr;
    FinArgs a{p->d_tables + hp.fin_off, p->d_tables + hp.fin_off, p->d_tables + hp.tgt_off, reinterpret_cast<const float*>(ws + lay.slabs),
              reinterpret_cast<const float*>(ws + lay.dec_slabs), gparams, hp.n_lanes, gw_parts, loss, fin_inv_n(hp, c), fin_n_dec(c), c.accumulates()};
    if (!gparams) {      // activation backward only: no gradient to finalize, one workgroup for the fused loss (if any)
        if (loss) hipLaunchKernelGGL(k_finalize_whole, dim3(1, 1), dim3(256), 0, st, a);
        HIPCHK(hipGetLastError());
        return MSHGNN_OK;
    }
    ProfScope ps(p, hp.ks_fin, st);
    if (fin_split(hp)) {      // bf16 / split plan: the slab sums of this phase; everything else ran in the weight-gradient launch (fill_gradw_side)
        FinSlabArgs s{p->d_tables + hp.fslab_off, p->d_tables + hp.fin_off, a.slabs, gparams, hp.n_lanes, gw_parts, c.accumulates()};
        int n = hp.n_fslab;
        if (gw_phase == 0) n = hp.n_fslab_ph0;
        if (gw_phase == 1) { s.recs += (size_t)hp.n_fslab_ph0 * FSLAB_INTS; n = hp.n_fslab - hp.n_fslab_ph0; }
        if (n > 0) hipLaunchKernelGGL(k_finalize, dim3(n), dim3(256), 0, st, s);
        HIPCHK(hipGetLastError());
        return MSHGNN_OK;
    }
    int f0 = 0, nf = hp.n_fin;
    if (gw_phase == 0) nf = hp.n_fin_ph0;
    if (gw_phase == 1) { f0 = hp.n_fin_ph0; nf = hp.n_fin - hp.n_fin_ph0; a.loss = nullptr; }
    a.fin += (size_t)f0 * FIN_INTS;
    if (nf > 0) hipLaunchKernelGGL(k_finalize_whole, dim3(nf, 64), dim3(256), 0, st, a);
    HIPCHK(hipGetLastError());
    return MSHGNN_OK;
}

// what differs between the fp32 and bf16 plans on the host side of a launch (mshgnn_launch.hpp; the split plan's: mshgnn_x3.hip)
template <typename T> static constexpr LaunchTraits plan_traits{
    (int)sizeof(T), Prec<T>::EPC, Prec<T>::EPC, Prec<T>::BLK, Prec<T>::ENC_MB * Prec<T>::ROWS, Prec<T>::ENC_MB * Prec<T>::BLK, sizeof(T) == 4 ? GW_KW : GWB_KW,
    /*split*/ false, /*embed_prep*/ sizeof(T) == 2, /*src_routes*/ sizeof(T) == 2, /*wide_needs_rows*/ false, /*gradw_series*/ sizeof(T) == 2,
    "the fused window assembly needs 16-byte aligned window rows (pitch a multiple of 8)",
    "wide source rows: the plan-dtype rows need 16-byte alignment and a pitch that is a multiple of 8"};

template <typename T>
static int forward_impl(const mshgnn_plan* p, StepCall& c) {
    // c.loss (one-call steps): the fused stack kernels run decoder, loss and decoder backward in their tail (c.dec_done); where the slab kernels run, the backward
    // sweep of the stack runs in the same launch as well (k_slab_step) and c.stack_done tells backward_impl to skip its own
    const HostPlan& hp = p->hp;
    const mshgnn_desc& d = hp.d;
    const LaunchTraits& tr = plan_traits<T>;
    const int training = c.training;
    mshgnn_ws_layout lay; layout_workspace(hp, c.batch, training, &lay);
    const int B = (int)c.batch;
    char* ws = c.ws; hipStream_t st = c.stream;
    int rc;
    // 1. weight images (bf16 plan with few packs: the layer packs by extra workgroups of the encoder launch, enc_prep_split), 2. encoder
    {
        EncArgs a{}; unsigned enc_grid = 0; int form = 0;
        if ((rc = prep_and_enc_args(p, c, lay, tr, launch_prep_t<T>, a, enc_grid))) return rc;
        ProfScope ps(p, hp.ks_enc, st);
        if ((rc = pick_enc_form(c, a, tr, enc_grid, form))) return rc;
        hipLaunchKernelGGL(ENC_TABLE<T>[form], dim3(enc_grid), dim3(256), tr.enc_lds, st, a, enc_series_src(c, form), enc_wide_src(c, form));
    }
    // 3. layers (+ decoder): one fused launch on the bf16 plan, else one kernel per layer and the decoder kernel
    const int tiles = (B + Prec<T>::ROWS - 1) / Prec<T>::ROWS;
    if constexpr (sizeof(T) == 2) {
        if (p->use_fused) {
            StackArgs a{};
            fill_stack_common(p, c, lay, a);
            fill_stack_tail(p, c, lay, a);
            a.tile_in = ws + lay.x[0]; a.training = training; a.dbg = p->dbg;
            a.stamps = stamp_ptr("MSHGNN_STAMPS");
            const pick::StackPick pk = pick::pick_stack(stack_query(p, c, pick::PLAN_BF16, forward_op(c), tr.blk, a));
            apply_stack_pick(hp, pk, lay, a);
            if (pk.what == pick::STEP) c.stack_done = true;      // the backward sweep runs in the same launch
            ProfScope ps(p, pk.what == pick::STEP ? hp.ks_stack_step : hp.ks_stack_fwd, st);
            return launch_stack(stack_kernel(hp, pk), pk, st, a);
        }
    }
    for (int l = 0; l < hp.L; ++l) {
        LayerArgs a{};
        a.x_in = ws + lay.x[l]; a.x_out = ws + lay.x[l + 1]; a.maskbits = reinterpret_cast<unsigned*>(ws + lay.mask[l]);
        a.hb = ws + lay.hb[l]; a.t1 = ws + lay.t1[l]; a.wpack = ws + lay.wpack; a.bias = reinterpret_cast<const float*>(ws + lay.bias);
        a.prog = p->d_tables + hp.fwd_prog_off[l]; a.B = B; a.NN = hp.NN; a.n_mlp = std::max(1, hp.n_mlp);
        a.dbg = p->dbg;
        ProfScope ps(p, hp.ks_layer_fwd0 + l, st);
        hipLaunchKernelGGL(k_layer_fwd<T>, dim3(tiles), dim3(LAYER_THREADS), hp.n_blk * Prec<T>::BLK, st, a);
    }
    // 4. decoder
    {
        DecArgs a{};
        a.xl = ws + lay.x[hp.L]; a.params = c.params; a.out_mask = p->d_out_mask; a.out = c.out; a.off_w = d.off_dec_w; a.off_b = d.off_dec_b;
        a.B = B; a.NN = hp.NN; a.node0 = hp.type_base[d.out_type]; a.n_out = d.type_nodes[d.out_type]; a.dout = d.out_channels;
        const int64_t rows = (int64_t)B * a.n_out;
        ProfScope ps(p, hp.ks_dec_fwd, st);
        hipLaunchKernelGGL(k_dec_fwd<T>, dim3((unsigned)((rows + 15) / 16)), dim3(256), 0, st, a);
    }
    HIPCHK(hipGetLastError());
    return MSHGNN_OK;
}

template <typename T>
static int backward_impl(const mshgnn_plan* p, const StepCall& c) {
    const HostPlan& hp = p->hp;
    const LaunchTraits& tr = plan_traits<T>;
    mshgnn_ws_layout lay; layout_workspace(hp, c.batch, 1, &lay);
    const int B = (int)c.batch;
    char* ws = c.ws; hipStream_t st = c.stream;
    const int gw_phase = c.gw_phase;
    if (!c.dec_done && gw_phase != 1) {
        DecArgs a{};
        fill_dec_bwd_args(p, c, lay, a);
        ProfScope ps(p, hp.ks_dec_bwd, st);
        hipLaunchKernelGGL((k_dec_bwd<T, false>), dim3(NWG_DEC), dim3(256), 0, st, a);
    }
    const int tiles = (B + Prec<T>::ROWS - 1) / Prec<T>::ROWS;
    bool fused_done = gw_phase == 1 || c.stack_done;      // (stack_done: k_slab_step already ran the backward sweep of the stack, forward_impl)
    if constexpr (sizeof(T) == 2) {
        if (p->use_fused && !fused_done) {
            StackArgs a{};
            fill_stack_common(p, c, lay, a);
            a.tile_in = ws + lay.dx[hp.L]; a.training = 1; a.dbg = p->dbg;
            a.stamps = stamp_ptr("MSHGNN_STAMPS_BWD");
            const pick::StackPick pk = pick::pick_stack(stack_query(p, c, pick::PLAN_BF16, pick::OP_BWD, tr.blk, a));
            apply_stack_pick(hp, pk, lay, a);
            ProfScope ps(p, hp.ks_stack_bwd, st);
            if (int rc = launch_stack(stack_kernel(hp, pk), pk, st, a)) return rc;
            fused_done = true;
        }
    }
    for (int l = hp.L - 1; l >= 0 && !fused_done; --l) {
        LayerArgs a{};
        a.x_in = ws + lay.dx[l + 1]; a.x_out = ws + lay.dx[l]; a.maskbits = reinterpret_cast<unsigned*>(ws + lay.mask[l]);
        a.hb = ws + lay.hb[l]; a.t1 = ws + lay.t1[l]; a.dh = ws + lay.dh[l]; a.du = ws + lay.du[l]; a.x_act = ws + lay.x[0];
        a.wpack = ws + lay.wpack; a.bias = reinterpret_cast<const float*>(ws + lay.bias);
        a.prog = p->d_tables + hp.bwd_prog_off[l]; a.B = B; a.NN = hp.NN; a.n_mlp = std::max(1, hp.n_mlp);
        a.dbg = p->dbg;
        ProfScope ps(p, hp.ks_layer_bwd0 + (hp.L - 1 - l), st);
        hipLaunchKernelGGL(k_layer_bwd<T>, dim3(tiles), dim3(LAYER_THREADS), hp.n_blk * Prec<T>::BLK, st, a);
    }
    const int gw_parts = gw_parts_for(hp.n_parts, hp.n_lanes, hp.gw_ipl, B, tr.gw_windows, p->n_cu);      // window parts of this batch's weight-gradient launch (<= the plan's)
    if (c.grad_params) {      // (NULL: activation backward only -- dX_0 for mshgnn_input_grad, no weight gradients)
        GradwArgs a{};
        fill_gradw_args(p, c, lay, tr, gw_parts, a);
        ProfScope ps(p, hp.ks_gradw, st);
        // (round 6, measured and not kept: phase 1's lanes on a side stream BESIDE phase 0's -- forked behind the stack launch, joined by phase 1's finalize.  On a
        //  1-rank RCCL group the two-phase step took 0.306 ms that way against 0.268 back to back and 0.186 for the plain step: two concurrent sweeps of the batch
        //  evict each other's shared rows.)
        const dim3 grid(a.side.n_grid + std::max(a.n_pad, 0) * gw_parts);      // the slab-free finalize workgroups first (bf16 plan; fp32: none)
        a.n_pad = std::max(a.n_pad, 1);      // (a phase without lanes: only those workgroups)
        if (grid.x == 0) {}
        else if constexpr (sizeof(T) == 4) hipLaunchKernelGGL(k_gradw_f32, grid, dim3(256), 0, st, a);
        else if (c.gradw_from_series && c.series) hipLaunchKernelGGL((k_gradw_bf16_lean<true, true>), grid, dim3(256), 0, st, a);      // raw operands from the series
        else if (a.aligned) hipLaunchKernelGGL(k_gradw_bf16_lean<true>, grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL(k_gradw_bf16_lean<false>, grid, dim3(256), 0, st, a);
    }
    return run_finalize(p, c, lay, gw_parts);
}

// ------------------------------------------------------------------------------------------------------
// The engine dispatch, once per operation.  Every extern "C" entry point below validates its own arguments, fills a StepCall (mshgnn_device.hpp) and
// calls one of these three.
// ------------------------------------------------------------------------------------------------------
static int run_forward(const mshgnn_plan* p, StepCall& c) {
    if (c.wide && c.series) return set_err(MSHGNN_EINVAL, "a call takes its encoder rows from wide sources or from a series, not from both");
    if (p->gen) return gen_forward(p, c);
    if (p->hp.d.dtype == MSHGNN_BF16X3) return x3_forward(p, c);
    if (p->hp.d.dtype == MSHGNN_F32) return forward_impl<float>(p, c);
    return forward_impl<__bf16>(p, c);
}

static int run_backward(const mshgnn_plan* p, const StepCall& c) {
    if (p->gen) return gen_backward(p, c);
    if (p->hp.d.dtype == MSHGNN_BF16X3) return x3_backward(p, c);
    if (p->hp.d.dtype == MSHGNN_F32) return backward_impl<float>(p, c);
    return backward_impl<__bf16>(p, c);
}

// Windows per sub-step of a one-call step, 0: the step runs whole.  Whole: batches under twice MSHGNN_STEP_CHUNK (read when the plan is created; default 32 768; 0 = always whole), the
// generic-width engine (its finalize kernel overwrites), wide-source calls (their source pointers are not offset here) and the series routes (nor are their window starts).  Equal sub-steps of
// whole 16-window tiles.
static int64_t step_chunk_windows(const mshgnn_plan* p, const StepCall& c) {
    const int64_t limit = p->step_chunk;
    if (limit <= 0 || c.batch < 2 * limit || p->gen || c.wide || c.series) return 0;
    const int64_t n = c.batch / limit;      // sub-steps of at least `limit` windows each (a step's cost per window is flat from there up; shorter ones cost ~5 % more)
    return ((c.batch + n - 1) / n + TILE_ROWS - 1) / TILE_ROWS * TILE_ROWS;
}

// One training step with a fused loss: the forward, then the backward from whatever the forward left undone (c.dec_done, c.stack_done) -- on the generic engine, the fp32
// plan and a bf16 plan without the fused stack kernels nothing, which makes it the two-call sequence.  A long batch runs as sub-steps over contiguous window
// ranges into one gradient (StepChunk).
static int run_step(const mshgnn_plan* p, StepCall& c) {
    auto whole = [p](StepCall& s) { const int rc = run_forward(p, s); return rc ? rc : run_backward(p, s); };
    const int64_t cw = step_chunk_windows(p, c);
    if (!cw) return whole(c);
    const mshgnn_desc& d = p->hp.d;
    const int64_t eb = d.dtype == MSHGNN_BF16 ? 2 : 4;      // input rows: bf16 on the bf16 plan, fp32 on the split and fp32 plans
    const int64_t n_out = d.type_nodes[d.out_type], orow = n_out * d.out_channels;
    int idx = 0;
    for (int64_t w0 = 0; w0 < c.batch; w0 += cw, ++idx) {
        const void* xc[MSHGNN_MAX_TYPES] = {};
        for (int t = 0; t < p->n_types; ++t)
            xc[t] = static_cast<const char*>(c.x[t]) + w0 * d.type_nodes[t] * (c.x_pitch ? c.x_pitch[t] : (int64_t)d.type_width[t]) * eb;
        StepCall sub = c;
        sub.x = xc; sub.batch = std::min(cw, c.batch - w0); sub.chunk = StepChunk{c.batch, idx};
        sub.out = c.out + w0 * orow;
        if (c.loss == LossKind::MSE) sub.y = c.y + w0 * orow; else sub.labels = c.labels + w0 * n_out;
        if (const int rc = whole(sub)) return rc;
    }
    return MSHGNN_OK;
}

// ---- the caller's own fp64 / fp32 tensors as inputs (the reference's datasets produce fp64, gnnLightning.py:1183): the encoder converts in registers and
// writes the plan-dtype rows the weight-gradient kernel needs on the side -- no separate cast + re-pitch pass.  The _src entry points check the source
// description into a WideSrc here and hand it to the encoder launch in their call (StepCall.wide).
static int fill_wide_src(const mshgnn_plan* p, int src_bytes, const void* const* src, const int64_t* src_pitch, const char* who, WideSrc& w) {
    if (!p || !src) return set_err(MSHGNN_EINVAL, std::string("null argument to ") + who);
    if (src_bytes != 4 && src_bytes != 8) return set_err(MSHGNN_EINVAL, std::string(who) + ": src_bytes must be 4 (fp32) or 8 (fp64)");
    if (p->gen || p->hp.d.dtype == MSHGNN_F32) return set_err(MSHGNN_EUNSUPPORTED, std::string(who) + ": wide source rows run on the bf16 and split-bf16 plans of the LDS-resident kernels");
    w.bytes = src_bytes;
    for (int t = 0; t < p->n_types; ++t) {
        if (!src[t]) return set_err(MSHGNN_EINVAL, std::string(who) + ": null source tensor");
        w.p[t] = src[t]; w.pitch[t] = src_pitch ? src_pitch[t] : p->hp.d.type_width[t];
        if (w.pitch[t] < p->hp.d.type_width[t]) return set_err(MSHGNN_EINVAL, std::string(who) + ": src_pitch smaller than the feature width");
        if (((uintptr_t)src[t] % (src_bytes == 8 ? 8 : 4)) != 0) return set_err(MSHGNN_EINVAL, std::string(who) + ": source tensor not aligned to its element size");
        // fp32 rows are read in 8-byte units where the width allows it: rows must then start on 8 bytes
        if (src_bytes == 4 && (p->hp.d.type_width[t] & 1) == 0 && ((((uintptr_t)src[t]) | (uintptr_t)(w.pitch[t] * 4)) & 7) != 0)
            return set_err(MSHGNN_EINVAL, std::string(who) + ": fp32 source rows of an even width must start 8-byte aligned (base and pitch)");
    }
    return MSHGNN_OK;
}

// mshgnn_forward and mshgnn_forward_src behind their own checks (wide: null on the plain entry point; both report under the plain name)
static int forward_entry(const mshgnn_plan* p, const WideSrc* wide, const void* const* x, const int64_t* x_pitch, const float* params, float* out,
                         void* workspace, int64_t batch, int training, void* stream) {
    if (!p || !x || !params || !out || !workspace) return set_err(MSHGNN_EINVAL, "null argument to mshgnn_forward");
    if (batch < 1 || batch > (1 << 24)) return set_err(MSHGNN_EINVAL, "batch must be in [1, 2^24]");
    for (int t = 0; t < p->n_types; ++t) if (!x[t]) return set_err(MSHGNN_EINVAL, "null input tensor");
    StepCall c;
    c.x = x; c.x_pitch = x_pitch; c.params = params; c.out = out; c.ws = (char*)workspace; c.batch = batch; c.training = training; c.stream = (hipStream_t)stream;
    c.wide = wide;
    return run_forward(p, c);
}

extern "C" int mshgnn_forward(const mshgnn_plan* p, const void* const* x, const int64_t* x_pitch, const float* params, float* out,
                              void* workspace, int64_t batch, int training, void* stream) {
    return forward_entry(p, nullptr, x, x_pitch, params, out, workspace, batch, training, stream);
}

extern "C" int mshgnn_forward_src(const mshgnn_plan* p, int src_bytes, const void* const* src, const int64_t* src_pitch, void* const* x_rows, const int64_t* x_pitch,
                                  const float* params, float* out, void* workspace, int64_t batch, int training, void* stream) {
    if (!x_rows) return set_err(MSHGNN_EINVAL, "mshgnn_forward_src: x_rows is null (the plan-dtype rows the encoder materialises)");
    WideSrc w{};
    if (const int rc = fill_wide_src(p, src_bytes, src, src_pitch, "mshgnn_forward_src", w)) return rc;
    return forward_entry(p, &w, x_rows, x_pitch, params, out, workspace, batch, training, stream);
}

// the backward entry points: from the output's gradient (grad_out), or from a loss fused into the decoder backward (out + y / labels -> loss_out)
static int backward_entry(const mshgnn_plan* p, const void* const* x, const int64_t* x_pitch, const float* params, float* grad_params, void* workspace,
                          int64_t batch, void* stream, StepCall& c) {
    if (batch < 1 || batch > (1 << 24)) return set_err(MSHGNN_EINVAL, "batch must be in [1, 2^24]");
    c.x = x; c.x_pitch = x_pitch; c.params = params; c.grad_params = grad_params; c.ws = (char*)workspace; c.batch = batch; c.stream = (hipStream_t)stream;
    return MSHGNN_OK;
}

extern "C" int mshgnn_backward(const mshgnn_plan* p, const void* const* x, const int64_t* x_pitch, const float* params, const float* grad_out,
                               float* grad_params, void* workspace, int64_t batch, void* stream) {
    if (!p || !x || !params || !grad_out || !workspace) return set_err(MSHGNN_EINVAL, "null argument to mshgnn_backward");
    StepCall c;
    if (const int rc = backward_entry(p, x, x_pitch, params, grad_params, workspace, batch, stream, c)) return rc;
    c.grad_out = grad_out;
    return run_backward(p, c);
}

extern "C" int mshgnn_backward_mse(const mshgnn_plan* p, const void* const* x, const int64_t* x_pitch, const float* params, const float* out,
                                   const float* y, float* loss_out, float* grad_params, void* workspace, int64_t batch, void* stream) {
    if (!p || !x || !params || !out || !y || !loss_out || !workspace) return set_err(MSHGNN_EINVAL, "null argument to mshgnn_backward_mse");
    StepCall c;
    if (const int rc = backward_entry(p, x, x_pitch, params, grad_params, workspace, batch, stream, c)) return rc;
    c.loss = LossKind::MSE; c.out = const_cast<float*>(out); c.y = y; c.loss_out = loss_out;      // (the backward only reads out)
    c.reg_kind = p->reg_kind; c.reg_delta = p->reg_delta;
    return run_backward(p, c);
}

extern "C" int mshgnn_backward_ce(const mshgnn_plan* p, const void* const* x, const int64_t* x_pitch, const float* params, const float* out,
                                  const int32_t* labels, float* loss_out, float* grad_params, void* workspace, int64_t batch, void* stream) {
    if (!p || !x || !params || !out || !labels || !loss_out || !workspace) return set_err(MSHGNN_EINVAL, "null argument to mshgnn_backward_ce");
    StepCall c;
    if (const int rc = backward_entry(p, x, x_pitch, params, grad_params, workspace, batch, stream, c)) return rc;
    if (p->hp.d.out_channels != 2) return set_err(MSHGNN_EINVAL, "mshgnn_backward_ce needs a 2-logit (contact classification) plan");
    c.loss = LossKind::CE; c.out = const_cast<float*>(out); c.labels = labels; c.loss_out = loss_out;
    return run_backward(p, c);
}

// The one-call steps (mshgnn_step_mse / _ce, their _src twins with `wide`, mshgnn_step_mse_phase): the checks they share, under the name of the plain entry point
// (`who`: the _src twins always reported under it), and the call they fill.  target: y (MSE) or the int32 labels (CE).
static int step_call(const mshgnn_plan* p, const char* who, const void* const* x, const int64_t* x_pitch, const float* params, LossKind kind, const void* target,
                     float* out, float* loss_out, float* grad_params, void* workspace, int64_t batch, void* stream, StepCall& c) {
    if (!p || !x || !params || !target || !out || !loss_out || !grad_params || !workspace) return set_err(MSHGNN_EINVAL, std::string("null argument to ") + who);
    if (batch < 1 || batch > (1 << 24)) return set_err(MSHGNN_EINVAL, "batch must be in [1, 2^24]");
    c.x = x; c.x_pitch = x_pitch; c.params = params; c.out = out; c.ws = (char*)workspace; c.batch = batch; c.training = 1; c.stream = (hipStream_t)stream;
    c.loss = kind; c.loss_out = loss_out; c.grad_params = grad_params;
    if (kind == LossKind::MSE) { c.y = static_cast<const float*>(target); c.reg_kind = p->reg_kind; c.reg_delta = p->reg_delta; }
    else c.labels = static_cast<const int32_t*>(target);
    return MSHGNN_OK;
}
static int step_entry(const mshgnn_plan* p, const WideSrc* wide, const void* const* x, const int64_t* x_pitch, const float* params, LossKind kind, const void* target,
                      float* out, float* loss_out, float* grad_params, void* workspace, int64_t batch, void* stream) {
    StepCall c;
    if (const int rc = step_call(p, kind == LossKind::CE ? "mshgnn_step_ce" : "mshgnn_step_mse", x, x_pitch, params, kind, target, out, loss_out, grad_params, workspace, batch, stream, c)) return rc;
    for (int t = 0; t < p->n_types; ++t) if (!x[t]) return set_err(MSHGNN_EINVAL, "null input tensor");
    if (kind == LossKind::CE && p->hp.d.out_channels != 2) return set_err(MSHGNN_EINVAL, "mshgnn_step_ce: the classification wrappers have two logits per foot");
    c.wide = wide;
    return run_step(p, c);
}

extern "C" int mshgnn_step_mse(const mshgnn_plan* p, const void* const* x, const int64_t* x_pitch, const float* params, const float* y,
                               float* out, float* loss_out, float* grad_params, void* workspace, int64_t batch, void* stream) {
    return step_entry(p, nullptr, x, x_pitch, params, LossKind::MSE, y, out, loss_out, grad_params, workspace, batch, stream);
}

extern "C" int mshgnn_step_ce(const mshgnn_plan* p, const void* const* x, const int64_t* x_pitch, const float* params, const int32_t* labels,
                              float* out, float* loss_out, float* grad_params, void* workspace, int64_t batch, void* stream) {
    return step_entry(p, nullptr, x, x_pitch, params, LossKind::CE, labels, out, loss_out, grad_params, workspace, batch, stream);
}

extern "C" int mshgnn_step_mse_src(const mshgnn_plan* p, int src_bytes, const void* const* src, const int64_t* src_pitch, void* const* x_rows, const int64_t* x_pitch,
                                   const float* params, const float* y, float* out, float* loss_out, float* grad_params, void* workspace, int64_t batch, void* stream) {
    if (!x_rows) return set_err(MSHGNN_EINVAL, "mshgnn_step_mse_src: x_rows is null (the plan-dtype rows the encoder materialises)");
    WideSrc w{};
    if (const int rc = fill_wide_src(p, src_bytes, src, src_pitch, "mshgnn_step_mse_src", w)) return rc;
    return step_entry(p, &w, x_rows, x_pitch, params, LossKind::MSE, y, out, loss_out, grad_params, workspace, batch, stream);
}
extern "C" int mshgnn_step_ce_src(const mshgnn_plan* p, int src_bytes, const void* const* src, const int64_t* src_pitch, void* const* x_rows, const int64_t* x_pitch,
                                  const float* params, const int32_t* labels, float* out, float* loss_out, float* grad_params, void* workspace, int64_t batch, void* stream) {
    if (!x_rows) return set_err(MSHGNN_EINVAL, "mshgnn_step_ce_src: x_rows is null (the plan-dtype rows the encoder materialises)");
    WideSrc w{};
    if (const int rc = fill_wide_src(p, src_bytes, src, src_pitch, "mshgnn_step_ce_src", w)) return rc;
    return step_entry(p, &w, x_rows, x_pitch, params, LossKind::CE, labels, out, loss_out, grad_params, workspace, batch, stream);
}

// The MSE step in two halves (gw_phase): phase 0 = forward, backward sweep and every weight gradient but the encoder's; phase 1 = the encoder's alone, from the dX_0
// phase 0 left in the workspace -- no forward, so what the forward would have told the backward is said here.  Never chunked.
extern "C" int mshgnn_step_mse_phase(const mshgnn_plan* p, const void* const* x, const int64_t* x_pitch, const float* params, const float* y,
                                     float* out, float* loss_out, float* grad_params, void* workspace, int64_t batch, int phase, void* stream) {
    StepCall c;
    if (const int rc = step_call(p, "mshgnn_step_mse_phase", x, x_pitch, params, LossKind::MSE, y, out, loss_out, grad_params, workspace, batch, stream, c)) return rc;
    if (phase != 0 && phase != 1) return set_err(MSHGNN_EINVAL, "phase must be 0 or 1");
    if (p->gen || p->hp.grad_split < 0) return set_err(MSHGNN_EUNSUPPORTED, "this plan has no two-phase gradient split");
    for (int t = 0; t < p->n_types; ++t) if (!x[t]) return set_err(MSHGNN_EINVAL, "null input tensor");
    c.gw_phase = phase;
    if (phase == 0) { if (const int rc = run_forward(p, c)) return rc; }
    else c.dec_done = p->hp.d.dtype == MSHGNN_BF16X3 || (p->hp.d.dtype == MSHGNN_BF16 && p->use_fused);      // (as phase 0's forward found: the plans whose stack kernel has the fused tail)
    return run_backward(p, c);
}

// ------------------------------------------------------------------------------------------------------
// mshgnn_step_mse_series: one training step straight from a sequence's resident raw series -- the window gather of mshgnn_assemble_windows
// fused into the encoder (k_enc_fwd<.., SERIES>), which also writes the materialised windows for the weight-gradient kernel; labels by
// k_window_labels.  bf16 plan with the fused stack kernels; everything after the encoder is mshgnn_step_mse.
// ------------------------------------------------------------------------------------------------------
// the one thing mshgnn_step_*_series needs before its encoder launch: the base pointer of every run's series column (one workgroup).  The windows'
// labels (and the int32 contact flags of the classification step) are computed by extra workgroups of the encoder launch itself (SeriesSrc.lab):
// a launch of their own cost 13.6 us of dependent round trips in front of the encoder, there they run under its tail.
// (K > 1 group elements, orbit descriptors: all K blocks of `runs`, n_total = K * n_runs <= 8 * 128 pointers, in the same one workgroup; K == 1: a single pass)
__global__ void k_series_run_ptrs(const int* runs, int n_total, WindowArgs wa, int elem_bytes, unsigned long long* run_ptr) {
    for (int r = threadIdx.x; r < n_total; r += blockDim.x) {
        bool neg;
        const int sc = run_source(runs[(size_t)r * 5 + 3], wa.sign, neg);
        unsigned long long p = 0ull;
#pragma unroll
        for (int k = 0; k < WIN_MAX_SRC; ++k)
            if (sc >= 0 && (sc >> 8) == k) p = (unsigned long long)(reinterpret_cast<const char*>(wa.src[k]) + (size_t)(sc & 0xff) * wa.src_cstride[k] * elem_bytes);
        run_ptr[r] = p | (neg && p ? RUN_PTR_SIGN : 0ull);      // a negated run: the flag rides in bit 63, masked off by every gather (run_ptr_addr)
    }
}

// ---- what the series routes share: the caller's description of the sequence and the windows, one check of the window descriptor against the plan, one fill of
// SeriesSrc / LabelArgs.  Training = mshgnn_step_mse_series / mshgnn_step_ce_series and their _std forms, evaluation = mshgnn_forward_series.
struct SeriesArgs {      // as the entry points receive them
    const mshgnn_window_desc* d;
    const float* const* src; const void* const* src_bf16; const int64_t* src_cstride; const int64_t* src_rows;
    const int64_t* starts; int64_t batch;
    float* y_out; float* quat_out; int32_t* labels_out;      // labels_out: the classification routes (contact flags = labels != 0)
    void* run_ptrs;
};
struct SeriesChecks {      // where training and evaluation differ
    const char* who;                  // the route's name in messages (who_ce: where a message is the classification step's own)
    const char* who_ce;
    bool labels_required;             // training: the recipe must describe labels; evaluation: only when y_out is given
    bool takes_normalize;             // evaluation and mshgnn_step_*_series_std take standardised recipes (the NORM encoders); the plain training steps refuse them
    bool ce_needs_two_logits;         // training checks the plan's logit pairs here; evaluation leaves them to the caller's loss
    // node rows of several runs need history >= 8 (the encoders take a chunk's 8 elements from at most two runs).  Evaluation and the standardised training steps check it.
    // The plain training steps lack the check: closing that changes what the wrappers must fall back on and belongs in a change of its own -- until then this stays false there.
    bool several_runs_need_history8;
};

// the window descriptor against the plan (x_out: the window buffers training materialises into, or null), then the label description against the model's outputs
static int check_window_desc(const mshgnn_plan* p, const SeriesArgs& s, const SeriesChecks& k, void* const* x_out, const int64_t* x_pitch) {
    const mshgnn_window_desc* d = s.d;
    const mshgnn_desc& md = p->hp.d;
    const bool x3 = md.dtype == MSHGNN_BF16X3, want_y = s.y_out != nullptr, ce = s.labels_out != nullptr;
    const bool dtype_ok = x3 ? (d->dtype == MSHGNN_F32 || d->dtype == MSHGNN_BF16X3) : d->dtype == MSHGNN_BF16;
    const bool labels_ok = d->n_label >= 1 && d->label_cols && d->label_src >= 0 && d->label_src < d->n_src;
    if (d->n_types != md.n_types || !dtype_ok || (d->normalize && !k.takes_normalize) || !d->fast_layout || d->n_src < 1 || d->n_src > WIN_MAX_SRC || d->n_runs < 1 ||
        d->n_runs > WIN_MAX_RUNS || !d->runs || !d->rows || d->history < 1 || (k.labels_required && !labels_ok))
        return set_err(MSHGNN_EINVAL, std::string(k.who) + ": the window descriptor must be a fast_layout" + (k.takes_normalize ? "" : ", unstandardised") + " recipe" +
                                          (k.labels_required ? " with labels" : "") + " at the plan's input dtype (bf16; split plan: fp32)");
    const int epc = x3 ? 4 : 8;      // elements per 16 bytes of the window buffers
    int n_rows = 0;
    for (int t = 0; t < d->n_types; ++t) {
        if (d->type_nodes[t] != md.type_nodes[t] || d->type_width[t] != md.type_width[t]) return set_err(MSHGNN_EINVAL, "window recipe and plan disagree on a node type");
        if (x_out && (!x_out[t] || ((uintptr_t)x_out[t] & 15) || x_pitch[t] % epc || x_pitch[t] < (d->type_width[t] + epc - 1) / epc * epc)) return set_err(MSHGNN_EINVAL, "bad window buffer");
        n_rows += d->type_nodes[t];
    }
    if (n_rows != d->n_rows) return set_err(MSHGNN_EINVAL, "window recipe: one node row per node expected");
    if (k.several_runs_need_history8 && d->history < 8 && d->n_runs > d->n_rows)
        return set_err(MSHGNN_EUNSUPPORTED, std::string(k.who) + ": node rows of several runs need history >= 8; use mshgnn_assemble_windows + mshgnn_forward");
    if (ce && !want_y) return set_err(MSHGNN_EINVAL, std::string(k.who) + ": labels_out comes with y_out");
    if (want_y) {
        if (!labels_ok) return set_err(MSHGNN_EINVAL, "bad label description");
        // the label rows are the model's targets: per out node its out_channels values, or (classification) one contact flag
        if (d->n_label != md.type_nodes[md.out_type] * (ce ? 1 : md.out_channels)) return set_err(MSHGNN_EINVAL, "window recipe: label count differs from the model's outputs");
        if (k.ce_needs_two_logits && ce && md.out_channels != 2) return set_err(MSHGNN_EINVAL, std::string(k.who_ce) + ": the classification wrappers have two logits per foot");
    }
    return MSHGNN_OK;
}
static int check_label_rotation(const SeriesArgs& s, const SeriesChecks& k) {
    if (!s.y_out) return MSHGNN_OK;
    if (s.d->label_rotate && (s.d->n_label % 3 != 0 || s.d->quat_src < 0)) return set_err(MSHGNN_EINVAL, "label rotation needs 3-D labels and a quaternion source");
    if (s.labels_out && s.d->label_rotate) return set_err(MSHGNN_EINVAL, std::string(k.who_ce) + ": contact labels are not rotated");
    return MSHGNN_OK;
}
// the source arrays the gather reads: the fp32 series (split plan, standardised recipes) or their bf16 copies
static int check_series_sources(const SeriesArgs& s, bool fp32_gather, WindowArgs& wa) {
    wa.sign = desc_sign_word(s.d);
    for (int i = 0; i < s.d->n_src; ++i) {
        // (8 elements of slack behind every column: a chunk's 16-byte loads may run past the window's last step)
        if (!s.src[i] || (!fp32_gather && !s.src_bf16[i]) || s.src_rows[i] < s.d->history || s.src_cstride[i] < s.src_rows[i] + 8 || s.src_rows[i] >= (1ll << 31))
            return set_err(MSHGNN_EINVAL, "bad source array (the gather needs cstride >= rows + 8)");
        wa.src[i] = fp32_gather ? s.src[i] : reinterpret_cast<const float*>(s.src_bf16[i]); wa.src_cstride[i] = s.src_cstride[i];
    }
    return MSHGNN_OK;
}
// The run-pointer pre-launch (in front of the encoder, same stream) and the encoder's description of the series.  Labels, quaternions and contact flags come out of extra
// workgroups of the encoder launch (want_y / want_q; a test sequence without labels: none).
static void fill_series_src(const SeriesArgs& s, const WindowArgs& wa, bool fp32_gather, bool want_q, hipStream_t st, SeriesSrc& ser) {
    const mshgnn_window_desc* d = s.d;
    const int K = desc_elements(d);
    if (!d->run_ptrs_ready) {    // (the caller vouches for the scratch's contents otherwise: same descriptor, same source arrays as the call that filled it)
        hipLaunchKernelGGL(k_series_run_ptrs, dim3(1), dim3(256), 0, st, d->runs, K * d->n_runs, wa, fp32_gather ? 4 : 2, reinterpret_cast<unsigned long long*>(s.run_ptrs));
    }
    const bool want_y = s.y_out != nullptr;
    if (want_y || want_q) {
        LabelArgs& l = ser.lab;
        const int ls = want_y ? d->label_src : 0;
        l.lab = s.src[ls]; l.lab_cs = s.src_cstride[ls];
        const bool q = d->quat_src >= 0 && (want_q || d->label_rotate);
        l.quat_src = q ? s.src[d->quat_src] : nullptr; l.quat_cs = q ? s.src_cstride[d->quat_src] : 0;
        l.starts = s.starts; l.B = s.batch; l.T = d->history; l.label_cols = d->label_cols; l.n_label = want_y ? d->n_label : 0; l.label_rotate = want_y ? d->label_rotate : 0;
        l.y = s.y_out; l.quat = s.quat_out; l.labels_int = s.labels_out; l.sign = desc_sign_word(d);
    }
    ser.sign = desc_sign_word(d);
    if (K > 1) ser.n_runs = d->n_runs;      // (the element blocks of run_ptr are n_runs apart)
    ser.run_ptr = reinterpret_cast<const unsigned long long*>(s.run_ptrs); ser.rows = d->rows; ser.starts = s.starts; ser.T = d->history;
    { int r0 = 0; for (int t = 0; t < d->n_types; ++t) { ser.row0[t] = r0; r0 += d->type_nodes[t]; } }
}
// the plans the series routes run on: the bf16 plan with the fused stack kernels and the split plan
static bool series_plan_ok(const mshgnn_plan* p) { return !p->gen && (p->hp.d.dtype == MSHGNN_BF16X3 || (p->hp.d.dtype == MSHGNN_BF16 && p->use_fused)); }

// the statistics pre-pass of the standardised routes: {mean, sd} of every (window, run), one wave each.  ORBIT (K > 1 group elements): the statistics of window b's
// run r are those of ITS element's run -- run pointer (and sign) from block `element` of the table; the layout of `stats` stays [B][n_runs][2] (a window has exactly
// one element) and the lengths are element 0's, which are every element's.
template <bool ORBIT>
__global__ __launch_bounds__(256) void k_series_stats(const int* runs, int n_runs, int K, const unsigned long long* run_ptr, const int64_t* starts, int64_t B, double* stats) {
    const int lane = threadIdx.x & 63;
    const int64_t idx = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);      // (window, run): one wave each
    if (idx >= B * n_runs) return;
    const int64_t b = idx / n_runs; const int r = (int)(idx - b * n_runs);
    const int len = runs[(size_t)r * 5 + 4];
    int64_t sw = 0;
    if constexpr (ORBIT) sw = starts[b];
    const unsigned long long p = run_ptr[ORBIT ? (size_t)start_element(sw, K) * n_runs + r : (size_t)r];
    RunStats rs{0.0, 1.0};      // constant-one runs are left alone (never applied)
    if (p) {
        const float* sp = reinterpret_cast<const float*>(run_ptr_addr(p)) + (ORBIT ? start_row(sw) : starts[b]);
        const bool neg = (p & RUN_PTR_SIGN) != 0;      // the statistics of the NEGATED run, as mshgnn_assemble_windows computes them
        float v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int k = 2 * lane + 128 * (q >> 1) + (q & 1);
            v[q] = 1.0f;
            if (k < len) v[q] = xor_sign(sp[k], neg);
        }
        rs = run_stats(v, len, lane);
    }
    if (lane == 0) *reinterpret_cast<f64x2*>(stats + (size_t)idx * 2) = f64x2{rs.mean, rs.sd};
}
static void launch_series_stats(const mshgnn_window_desc* d, const SeriesSrc& ser, const int64_t* starts, int64_t batch, void* stats, hipStream_t st) {
    const int64_t waves = batch * d->n_runs;
    const dim3 grid((unsigned)((waves + 3) / 4));
    const int K = desc_elements(d);
    hipLaunchKernelGGL(K > 1 ? k_series_stats<true> : k_series_stats<false>, grid, dim3(256), 0, st, d->runs, d->n_runs, K, ser.run_ptr, starts, batch, reinterpret_cast<double*>(stats));
}

// std_route (mshgnn_step_*_series_std): a standardised recipe -- k_series_stats leaves {mean, sd} of every (window, run) in `stats`, the NORM encoders apply them to the
// FP32 series on both plans and write the standardised windows to x_out, which the weight-gradient pass then reads like assembled ones.
static int step_series(const mshgnn_plan* p, const SeriesArgs& s, bool std_route, void* stats, void* const* x_out, const int64_t* x_pitch, const float* params, float* out,
                       float* loss_out, float* grad_params, void* workspace, void* stream) {
    const bool ce = s.labels_out != nullptr;      // classification wrappers: cross entropy over the per-foot logit pairs, labels = the window labels != 0
    const char* who = std_route ? "mshgnn_step_mse_series_std" : "mshgnn_step_mse_series", * who_ce = std_route ? "mshgnn_step_ce_series_std" : "mshgnn_step_ce_series";
    if (!p || !s.d || !s.src || !s.src_cstride || !s.src_rows || !s.starts || !s.y_out || !s.run_ptrs || !params || !out || !loss_out ||
        !grad_params || !workspace || (x_out && !x_pitch)) return set_err(MSHGNN_EINVAL, std::string("null argument to ") + who + " / " + who_ce);
    if (s.batch < 1 || s.batch > (1 << 24)) return set_err(MSHGNN_EINVAL, "batch must be in [1, 2^24]");
    // bf16 plan (fused stack kernels): bf16 copies of the series, optional materialisation.  Split plan (MSHGNN_BF16X3): the fp32 series
    // themselves, windows always materialised (fp32) for its weight-gradient kernel.
    if (!series_plan_ok(p))
        return set_err(MSHGNN_EUNSUPPORTED, std::string(who) + " runs on the bf16 plan with the fused stack kernels or on the split plan; use mshgnn_assemble_windows + mshgnn_step_mse");
    const bool x3 = p->hp.d.dtype == MSHGNN_BF16X3;
    if (std_route) {
        if (!s.d->normalize)
            return set_err(MSHGNN_EINVAL, std::string(who) + ": the window descriptor is unstandardised; use mshgnn_step_mse_series / mshgnn_step_ce_series");
        if (!stats) return set_err(MSHGNN_EINVAL, std::string(who) + ": a standardised recipe needs the stats scratch (mshgnn_forward_series_stats_bytes)");
        if ((uintptr_t)stats & 15) return set_err(MSHGNN_EINVAL, std::string(who) + ": the stats scratch must be 16-byte aligned");
        if (s.d->history < 2) return set_err(MSHGNN_EINVAL, "history must be >= 2 when normalising");
        if (s.d->history > 256) return set_err(MSHGNN_EUNSUPPORTED, "history longer than 256 steps is not supported by this build");
        // (a weight-gradient kernel that standardises its raw operands again is not built: it reads the windows the encoder wrote)
        if (!x_out) return set_err(MSHGNN_EUNSUPPORTED, std::string(who) + ": the weight-gradient pass reads the materialised standardised windows: x_out must be given");
    }
    const bool fp32_gather = x3 || std_route;      // standardisation happens before the bf16 rounding: the bf16 plan's NORM encoder reads the fp32 series too
    if (!fp32_gather && !s.src_bf16) return set_err(MSHGNN_EINVAL, "null argument to mshgnn_step_mse_series / mshgnn_step_ce_series");
    if (x3 && !x_out) return set_err(MSHGNN_EUNSUPPORTED, "the split plan's weight-gradient kernel reads materialised windows: x_out must be given");
    // (the weight-gradient kernel's own series gather takes one table for the whole batch)
    if (!x_out && desc_elements(s.d) > 1) return set_err(MSHGNN_EUNSUPPORTED, std::string(who) + ": a descriptor with several group elements needs materialised windows: x_out must be given");
    // (the plain routes leave several_runs_need_history8 open, see SeriesChecks; the standardised ones are new and check it)
    const SeriesChecks k{who, who_ce, /*labels_required*/ true, /*takes_normalize*/ std_route, /*ce_needs_two_logits*/ true, /*several_runs_need_history8*/ std_route};
    WindowArgs wa{};
    if (const int rc = check_window_desc(p, s, k, x_out, x_pitch)) return rc;
    if (const int rc = check_series_sources(s, fp32_gather, wa)) return rc;
    if (const int rc = check_label_rotation(s, k)) return rc;
    if (const int rc = check_sign_tables(s.d, true, (hipStream_t)stream)) return rc;
    SeriesSrc ser{};
    fill_series_src(s, wa, fp32_gather, /*want_q: the quaternion travels with the labels wherever the recipe has one*/ true, (hipStream_t)stream, ser);
    if (std_route) {
        launch_series_stats(s.d, ser, s.starts, s.batch, stats, (hipStream_t)stream);
        ser.stats = reinterpret_cast<const double*>(stats); ser.n_runs = s.d->n_runs;
    }
    StepCall c;
    c.x = x_out; c.x_pitch = x_pitch; c.params = params; c.out = out; c.ws = (char*)workspace; c.batch = s.batch; c.training = 1; c.stream = (hipStream_t)stream;
    c.loss = ce ? LossKind::CE : LossKind::MSE; c.y = s.y_out; c.labels = s.labels_out; c.loss_out = loss_out; c.grad_params = grad_params;
    if (!ce) { c.reg_kind = p->reg_kind; c.reg_delta = p->reg_delta; }
    c.series = &ser;
    c.gradw_from_series = !x_out;      // no materialised windows at all (plain bf16 route only, see above): the weight-gradient kernel gathers its raw-input operands from the series as well
    return run_step(p, c);
}

extern "C" int mshgnn_step_mse_series(const mshgnn_plan* p, const mshgnn_window_desc* d, const float* const* src, const void* const* src_bf16,
                                      const int64_t* src_cstride, const int64_t* src_rows, const int64_t* starts, int64_t batch,
                                      void* const* x_out, const int64_t* x_pitch, float* y_out, float* quat_out, void* run_ptrs,
                                      const float* params, float* out, float* loss_out, float* grad_params, void* workspace, void* stream) {
    const SeriesArgs s{d, src, src_bf16, src_cstride, src_rows, starts, batch, y_out, quat_out, nullptr, run_ptrs};
    return step_series(p, s, false, nullptr, x_out, x_pitch, params, out, loss_out, grad_params, workspace, stream);
}

extern "C" int mshgnn_step_ce_series(const mshgnn_plan* p, const mshgnn_window_desc* d, const float* const* src, const void* const* src_bf16,
                                     const int64_t* src_cstride, const int64_t* src_rows, const int64_t* starts, int64_t batch,
                                     void* const* x_out, const int64_t* x_pitch, float* y_out, int32_t* labels_out, void* run_ptrs,
                                     const float* params, float* out, float* loss_out, float* grad_params, void* workspace, void* stream) {
    if (!labels_out) return set_err(MSHGNN_EINVAL, "null argument to mshgnn_step_ce_series");
    const SeriesArgs s{d, src, src_bf16, src_cstride, src_rows, starts, batch, y_out, nullptr, labels_out, run_ptrs};
    return step_series(p, s, false, nullptr, x_out, x_pitch, params, out, loss_out, grad_params, workspace, stream);
}
// The same steps on a STANDARDISED recipe (desc->normalize): mshgnn_assemble_windows(normalize) + mshgnn_step_mse / _ce, bit for bit.  stats: the scratch
// mshgnn_forward_series_stats_bytes sizes.  The plain entry points above keep refusing such recipes.
extern "C" int mshgnn_step_mse_series_std(const mshgnn_plan* p, const mshgnn_window_desc* d, const float* const* src, const void* const* src_bf16,
                                          const int64_t* src_cstride, const int64_t* src_rows, const int64_t* starts, int64_t batch,
                                          void* const* x_out, const int64_t* x_pitch, float* y_out, float* quat_out, void* run_ptrs, void* stats,
                                          const float* params, float* out, float* loss_out, float* grad_params, void* workspace, void* stream) {
    const SeriesArgs s{d, src, src_bf16, src_cstride, src_rows, starts, batch, y_out, quat_out, nullptr, run_ptrs};
    return step_series(p, s, true, stats, x_out, x_pitch, params, out, loss_out, grad_params, workspace, stream);
}

extern "C" int mshgnn_step_ce_series_std(const mshgnn_plan* p, const mshgnn_window_desc* d, const float* const* src, const void* const* src_bf16,
                                         const int64_t* src_cstride, const int64_t* src_rows, const int64_t* starts, int64_t batch,
                                         void* const* x_out, const int64_t* x_pitch, float* y_out, int32_t* labels_out, void* run_ptrs, void* stats,
                                         const float* params, float* out, float* loss_out, float* grad_params, void* workspace, void* stream) {
    if (!labels_out) return set_err(MSHGNN_EINVAL, "null argument to mshgnn_step_ce_series_std");
    const SeriesArgs s{d, src, src_bf16, src_cstride, src_rows, starts, batch, y_out, nullptr, labels_out, run_ptrs};
    return step_series(p, s, true, stats, x_out, x_pitch, params, out, loss_out, grad_params, workspace, stream);
}
// ------------------------------------------------------------------------------------------------------
// mshgnn_forward_series: evaluation straight from a sequence's resident raw series -- mshgnn_assemble_windows + mshgnn_forward(training = 0) with the window
// gather fused into the encoder and NO materialised windows (x = NULL: only the nodes whose X_0 can reach the output get encoder workgroups).  Labels,
// quaternions and contact flags come out of the encoder launch's extra workgroups, each optional.  Standardised recipes: a pre-pass leaves {mean, sd} of every
// (window, run) in the caller's scratch (k_series_stats: one wave per run, the per-lane partial sums and the wave_sum order of k_assemble_windows -- the same
// function, run_stats), the NORM encoders apply them to the fp32 series (standardise_one).
// ------------------------------------------------------------------------------------------------------
extern "C" int64_t mshgnn_forward_series_stats_bytes(const mshgnn_window_desc* d, int64_t batch) {
    if (!d || batch < 1 || d->n_runs < 1 || !d->normalize) return 0;
    return batch * (int64_t)d->n_runs * 2 * (int64_t)sizeof(double);
}

extern "C" int mshgnn_forward_series(const mshgnn_plan* p, const mshgnn_window_desc* d, const float* const* src, const void* const* src_bf16,
                                     const int64_t* src_cstride, const int64_t* src_rows, const int64_t* starts, int64_t batch,
                                     float* y_out, float* quat_out, int32_t* labels_out, void* run_ptrs, void* stats, const float* params, float* out,
                                     void* workspace, void* stream) {
    if (!p || !d || !src || !src_cstride || !src_rows || !starts || !run_ptrs || !params || !out || !workspace)
        return set_err(MSHGNN_EINVAL, "null argument to mshgnn_forward_series");
    if (batch < 1 || batch > (1 << 24)) return set_err(MSHGNN_EINVAL, "batch must be in [1, 2^24]");
    if (!series_plan_ok(p))
        return set_err(MSHGNN_EUNSUPPORTED, "mshgnn_forward_series runs on the bf16 plan with the fused stack kernels or on the split plan; use mshgnn_assemble_windows + mshgnn_forward");
    const bool x3 = p->hp.d.dtype == MSHGNN_BF16X3;
    const bool norm = d->normalize != 0;
    if (!x3 && !norm && !src_bf16) return set_err(MSHGNN_EINVAL, "null argument to mshgnn_forward_series (the bf16 plan gathers unstandardised windows from the bf16 copies)");
    if (norm && !stats) return set_err(MSHGNN_EINVAL, "mshgnn_forward_series: a standardised recipe needs the stats scratch (mshgnn_forward_series_stats_bytes)");
    if (norm && d->history < 2) return set_err(MSHGNN_EINVAL, "history must be >= 2 when normalising");
    if (norm && d->history > 256) return set_err(MSHGNN_EUNSUPPORTED, "history longer than 256 steps is not supported by this build");
    if (norm && ((uintptr_t)stats & 15)) return set_err(MSHGNN_EINVAL, "mshgnn_forward_series: the stats scratch must be 16-byte aligned");
    const SeriesArgs s{d, src, src_bf16, src_cstride, src_rows, starts, batch, y_out, quat_out, labels_out, run_ptrs};
    const SeriesChecks k{"mshgnn_forward_series", "mshgnn_forward_series", /*labels_required*/ false, /*takes_normalize*/ true, /*ce_needs_two_logits*/ false,
                         /*several_runs_need_history8*/ true};
    if (const int rc = check_window_desc(p, s, k, nullptr, nullptr)) return rc;
    if (const int rc = check_label_rotation(s, k)) return rc;
    if (d->quat_src >= d->n_src) return set_err(MSHGNN_EINVAL, "quat_src out of range");
    const bool fp32_gather = x3 || norm;      // standardisation happens before the bf16 rounding: the bf16 plan's NORM encoder reads the fp32 series too
    WindowArgs wa{};
    if (const int rc = check_series_sources(s, fp32_gather, wa)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (const int rc = check_sign_tables(d, d->n_label > 0 && d->label_cols != nullptr, st)) return rc;      // (the whole descriptor: the caller vouches for all of it afterwards)
    SeriesSrc ser{};
    fill_series_src(s, wa, fp32_gather, quat_out != nullptr && d->quat_src >= 0, st, ser);
    if (norm) {
        launch_series_stats(d, ser, starts, batch, stats, st);
        ser.stats = reinterpret_cast<const double*>(stats); ser.n_runs = d->n_runs;
    }
    StepCall c;      // evaluation, nothing materialised (x = null): only the nodes whose X_0 can reach the output get encoder workgroups
    c.params = params; c.out = out; c.ws = (char*)workspace; c.batch = batch; c.training = 0; c.stream = st;
    c.series = &ser;
    return run_forward(p, c);
}
