// The stack kernels of the split-bf16 plan (mshgnn_x3.hip): device templates only.  What k_stack_step_x3 / k_stack_fwd_x3_spec / k_stack_bwd_x3_spec and spec_matches_x3
// reach, and nothing else: mshgnn_x3.hip instantiates them over the plan's run-time tables (the interpreters), mshgnn_x3_spec_shard.hip over the compile-time programs of
// mshgnn_spec_tables.inc (X3_*; one program per translation unit) and, after the build, over one plan's own tables (morphsym_hgnn_amd/jit.py).
#pragma once
#include "mshgnn_device.hpp"

// stage the [hi | lo] rows of every node for which keep(n) into LDS: 512 threads = 16 rows x 32 chunks, one node per load, 10 in flight
// (an 18-node tile in two round trips to HBM: with one workgroup per CU nothing else hides them)
template <typename Keep>
__device__ __forceinline__ void stage_tile_x3(char* smem, const T16* src, int NN, int LO, int w0, int B, int tid, Keep keep) {
    const int row = tid >> 5, c = tid & 31;      // chunk c < 16: hi half, else lo half
    const int blk_off = c < 16 ? 0 : LO, cc = c & 15;
    constexpr int BATCH = 10;
    for (int nb = 0; nb < NN; nb += BATCH) {
        u32x4 v[BATCH];
#pragma unroll
        for (int i = 0; i < BATCH; ++i) {
            v[i] = u32x4{0, 0, 0, 0};
            if (nb + i < NN && keep(nb + i) && w0 + row < B) v[i] = *reinterpret_cast<const u32x4*>(src + x3_idx(w0 + row, nb + i, B) + c * 8);
        }
#pragma unroll
        for (int i = 0; i < BATCH; ++i)
            if (nb + i < NN && keep(nb + i)) *reinterpret_cast<u32x4*>(smem + lds_chunk<T16>(blk_off + nb + i, row, cc)) = v[i];
    }
}

// three-product block GEMM of the base_transform chain on this wave's <= 2 accumulators: acc[u] += LDS[blk] (hi + lo) . W (hi + lo)
template <int N> __device__ __forceinline__ void mlp_mac3(P16::Acc (&acc)[N], const char* smem, int blk0, int lo_blk, int nmlp, int wh, const P16::BFrag& wh_, const P16::BFrag& wl_, int lane) {
    P16::AFrag af;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int n = 2 * u + wh;
        if (n < nmlp) {
            load_afrag<T16>(af, smem, blk0 + n, lane);
            mac(acc[u], af, wh_);
            mac(acc[u], af, wl_);
            load_afrag<T16>(af, smem, lo_blk + blk0 + n, lane);
            mac(acc[u], af, wh_);
        }
    }
}

// ------------------------------------------------------------------------------------------------------
// The forward stack (k_stack_fwd_x3 of mshgnn_x3.hip, k_stack_fwd_x3_spec, the first half of k_stack_step_x3): the whole message-passing stack (+ decoder, + wrapper
// MSE and decoder backward under mshgnn_step_mse) of one 16-window tile in one 8-wave workgroup -- k_stack_fwd of the bf16 plan on hi/lo planes
// ------------------------------------------------------------------------------------------------------
// ALIAS: the base_transform scratch blocks are the blocks of the last nodes (topologies whose doubled tile leaves no room: MiniCheetah-K4)
// STEP: part of k_stack_step_x3 -- the decoder tail leaves dX_L (both planes) in the out-type nodes' LDS blocks for the backward sweep of the same launch
// one forward layer of the split plan's 8-wave workgroup.  FH / FP: the layer's header and this wave half's program, interpreted (FHdr / FProg) or compile-time
// (SHdr / SProg: specialised kernels); WHS: the wave half as a template constant (compile-time programs: the per-node header reads fold) or -1; mid(): what has
// to settle between the MACs and the stores
template <bool ALIAS, bool STEP, int WHS, class FH, class FP, class Mid>
__device__ __forceinline__ void x3_fwd_layer(const StackArgs& a, char* smem, const T16* wpack, int wn, int wh, int lane, int l, int L, const FH& fh, const FP& wp, Mid&& mid) {
    using T = T16; using P = P16;
    const int tid = threadIdx.x, w0 = blockIdx.x * P::ROWS, B = a.B, NN = a.NN, LO = a.lo_blk, SCR = a.scr0;
    const int whv = WHS >= 0 ? WHS : wh;
    const bool train = a.training != 0;
    P::Acc acc[FS_HS];
        const int nmlp = fh[FH_NMLP], flags = fh[FH_FLAGS];
#pragma unroll
        for (int u = 0; u < FS_HS; ++u) {
            const int n = 2 * u + whv;
            if (n < NN && fh[FH_KIND + n] != NK_DEAD) acc_init_bias<T>(acc[u], a.bias + (size_t)fh[FH_BIAS + n] * H, wn, lane);
            else acc_fill(acc[u], 0.f);
        }
        FS_STAMP(2 + 4 * l);
        fs_run<T>(wp, acc, smem, wpack, wn, lane);
        // lane constants of the epilogue rebuilt per layer from an opaque copy of the lane id (per-node addresses derived from them were hoisted out
        // of the layer loop and spilled; a scratch reload next to pending stores is a full vmcnt(0) drain)
        const int lq = opaque(lane);
        const int win = c_win(lq), w = w0 + win, col = wn * 32 + c_oct(lq);
        const bool w_ok = w < B;
        FS_STAMP(3 + 4 * l);
        __syncthreads();   // every wave is done reading X_l: the node blocks may be overwritten
        FS_STAMP(4 + 4 * l);

        u32x4 hph[2] = {}, hpl[2] = {}, tph[2] = {}, tpl[2] = {};
        u32x4 vrh[2] = {}, vrl[2] = {};      // ALIAS: residual octets of the victim nodes SCR + wh + 2 j this wave owns, read before the chain overwrites their blocks
        if constexpr (ALIAS) {
            if (nmlp > 0 && (flags & FF_RESIDUAL)) {
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int v = SCR + whv + 2 * j;
                    if (v < SCR + nmlp && fh[FH_KIND + v] != NK_DEAD) {
                        vrh[j] = *reinterpret_cast<const u32x4*>(smem + lds_chunk<T>(v, win, col / P::EPC));
                        vrl[j] = *reinterpret_cast<const u32x4*>(smem + lds_chunk<T>(LO + v, win, col / P::EPC));
                    }
                }
            }
        }
        if (nmlp > 0) {
            // base_transform: Y = W2 relu(W1 H + b1) + b2 on the first nmlp nodes (hgnn_c2.py:117-121,156); scratch blocks NN + i (hi),
            // LO + NN + i (lo).  The H and T1 stashes are kept packed in registers and stored after the chain.
            P::BFrag bfh, bfl;
            load_bfrag<T>(bfh, wpack, fh[FH_W1], wn, lane);
            load_bfrag<T>(bfl, wpack, a.n_img + fh[FH_W1], wn, lane);
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int n = 2 * u + whv;
                if (n < nmlp) {
                    split_oct(acc[u].c[0], acc[u].c[1], hph[u], hpl[u]);
                    *reinterpret_cast<u32x4*>(smem + lds_chunk<T>(SCR + n, win, col / P::EPC)) = hph[u];
                    *reinterpret_cast<u32x4*>(smem + lds_chunk<T>(LO + SCR + n, win, col / P::EPC)) = hpl[u];
                    acc_init_bias<T>(acc[u], a.bias + (size_t)fh[FH_B1] * H, wn, lane);
                }
            }
            __syncthreads();
            mlp_mac3(acc, smem, SCR, LO, nmlp, whv, bfh, bfl, lane);      // accumulators 0..1 = nodes 0..3
            load_bfrag<T>(bfh, wpack, fh[FH_W2], wn, lane);
            load_bfrag<T>(bfl, wpack, a.n_img + fh[FH_W2], wn, lane);
            __syncthreads();   // all reads of H done before T1 overwrites the scratch blocks
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int n = 2 * u + whv;
                if (n < nmlp) {
                    split_oct(relu4(acc[u].c[0]), relu4(acc[u].c[1]), tph[u], tpl[u]);
                    *reinterpret_cast<u32x4*>(smem + lds_chunk<T>(SCR + n, win, col / P::EPC)) = tph[u];
                    *reinterpret_cast<u32x4*>(smem + lds_chunk<T>(LO + SCR + n, win, col / P::EPC)) = tpl[u];
                    acc_init_bias<T>(acc[u], a.bias + (size_t)fh[FH_B2] * H, wn, lane);
                }
            }
            __syncthreads();
            mlp_mac3(acc, smem, SCR, LO, nmlp, whv, bfh, bfl, lane);      // accumulators 0..1 = nodes 0..3
        }
        FS_STAMP(16 + l);
        // every load issued so far has landed before the first store of the epilogue goes out
        __builtin_amdgcn_s_waitcnt((7 << 4) | (15 << 8));
        mid();      // (FProg::settle of the next header / program: no vmcnt(0) for them at the top of the next layer)
        if (nmlp > 0 && train && w_ok) {
            T* hb = reinterpret_cast<T*>(a.ws + a.hb_off[l]);
            T* t1 = reinterpret_cast<T*>(a.ws + a.t1_off[l]);
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int n = 2 * u + whv;
                if (n < nmlp) {
                    *reinterpret_cast<u32x4*>(hb + x3_idx(w, n, B) + col) = hph[u];
                    *reinterpret_cast<u32x4*>(hb + x3_idx(w, n, B) + H + col) = hpl[u];
                    *reinterpret_cast<u32x4*>(t1 + x3_idx(w, n, B) + col) = tph[u];
                    *reinterpret_cast<u32x4*>(t1 + x3_idx(w, n, B) + H + col) = tpl[u];
                }
            }
        }

        // X_{l+1}[n] = f(H[n]) (+ X_l[n]) for every live node, in place; stash + relu bits on the side
        T* xo = reinterpret_cast<T*>(a.ws + a.x_off[l + 1]);
        uint8_t* maskbytes = reinterpret_cast<uint8_t*>(a.ws + a.mask_off[l]);
        u32x4 resh[FS_HS], resl[FS_HS]; int kindv[FS_HS];     // the residual octets of every node, all LDS reads in flight together
#pragma unroll
        for (int u = 0; u < FS_HS; ++u) {
            const int n = 2 * u + whv;
            kindv[u] = n < NN ? fh[FH_KIND + n] : NK_DEAD;
            resh[u] = u32x4{0, 0, 0, 0}; resl[u] = u32x4{0, 0, 0, 0};
            if (kindv[u] != NK_DEAD && (flags & FF_RESIDUAL)) {
                if (ALIAS && nmlp > 0 && n >= SCR && n < SCR + nmlp) {      // a victim: its block holds T1 by now
                    resh[u] = ((n - SCR) >> 1) == 0 ? vrh[0] : vrh[1]; resl[u] = ((n - SCR) >> 1) == 0 ? vrl[0] : vrl[1];
                } else {
                    resh[u] = *reinterpret_cast<const u32x4*>(smem + lds_chunk<T>(n, win, col / P::EPC));
                    resl[u] = *reinterpret_cast<const u32x4*>(smem + lds_chunk<T>(LO + n, win, col / P::EPC));
                }
            }
        }
#pragma unroll
        for (int u = 0; u < FS_HS; ++u) {
            const int n = 2 * u + whv;
            if (n < NN) {
                const int kind = kindv[u];
                if (kind != NK_DEAD) {
                    if (kind == NK_RELU) {
                        const unsigned bits = relu_with_bits<T>(acc[u]);
                        if (train) maskbytes[relu_byte(n, B, w, col)] = (uint8_t)bits;
                    }
                    f32x4 y0 = acc[u].c[0], y1 = acc[u].c[1];
                    if (flags & FF_RESIDUAL) {
                        f32x4 r0, r1;
                        join_oct(resh[u], resl[u], r0, r1);
                        y0 += r0; y1 += r1;
                    }
                    u32x4 hi, lo;
                    split_oct(y0, y1, hi, lo);
                    *reinterpret_cast<u32x4*>(smem + lds_chunk<T>(n, win, col / P::EPC)) = hi;
                    *reinterpret_cast<u32x4*>(smem + lds_chunk<T>(LO + n, win, col / P::EPC)) = lo;
                    if (train && w_ok && !(STEP && l + 1 == L)) {      // (X_L of a one-launch step is read by nobody)
                        T* q = xo + x3_idx(w, n, B) + col;
                        stash_store(q, hi, a.stash_nt != 0);
                        stash_store(q + H, lo, a.stash_nt != 0);
                    }
                }
            }
        }
        __syncthreads();
        FS_STAMP(5 + 4 * l);
}
// the layers of a compile-time program SP for wave half WH, unrolled
template <bool ALIAS, bool STEP, class SP, int WH, int l = 0>
__device__ __forceinline__ void x3_fwd_layers_static(const StackArgs& a, char* smem, const T16* wpack, int wn, int lane) {
    if constexpr (l < SP::L) {
        x3_fwd_layer<ALIAS, STEP, WH>(a, smem, wpack, wn, WH, lane, l, SP::L, SHdr<SP, 0, l>{}, SProg<SP, 0, l, WH>{}, [] {});
        x3_fwd_layers_static<ALIAS, STEP, SP, WH, l + 1>(a, smem, wpack, wn, lane);
    }
}

template <bool ALIAS, bool STEP, class SP = void> __device__ __forceinline__ void stack_fwd_x3_body(const StackArgs& a, char* smem) {
    using T = T16; using P = P16;
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wn = wv & 3, wh = wv >> 2;
    const int w0 = blockIdx.x * P::ROWS, B = a.B, NN = a.NN, LO = a.lo_blk;
    const T* wpack = reinterpret_cast<const T*>(a.wpack);

    FS_STAMP(0);
    stage_tile_x3(smem, reinterpret_cast<const T*>(a.tile_in), NN, LO, w0, B, tid, [](int) { return true; });
    __syncthreads();
    FS_STAMP(1);

    if constexpr (std::is_void<SP>::value) {
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
            x3_fwd_layer<ALIAS, STEP, -1>(a, smem, wpack, wn, wh, lane, l, a.L, fh, wp, [&] { fhn.settle(); wpn.settle(); });
        }
    } else if (wh == 0) x3_fwd_layers_static<ALIAS, STEP, SP, 0>(a, smem, wpack, wn, lane);      // (uniform per wave: each half runs its own straight-line program; the
    else x3_fwd_layers_static<ALIAS, STEP, SP, 1>(a, smem, wpack, wn, lane);                      //  barriers pair up by count)
    decoder_tail<T, LAYER_THREADS, true, STEP>(a, smem, tid, lane, wv, w0, B);
    FS_STAMP(30);
}

// ------------------------------------------------------------------------------------------------------
// The backward stack (k_stack_bwd_x3 of mshgnn_x3.hip, k_stack_bwd_x3_spec, the second half of k_stack_step_x3): the L backward layers of a tile -- k_stack_bwd of the bf16 plan on hi/lo planes
// ------------------------------------------------------------------------------------------------------
// STEP: part of k_stack_step_x3 -- the forward's decoder tail of the same launch left the dX_L tile in LDS; the layers' programs are a.prog_off_b
// one backward layer (see x3_fwd_layer); acc carries nothing between layers: the residual term is re-read from the tile
template <int WHS, class FH, class FP, class Mid>
__device__ __forceinline__ void x3_bwd_layer(const StackArgs& a, char* smem, const T16* wpack, int wn, int wh, int lane, int l, const FH& bh, const FP& wp, Mid&& mid) {
    using T = T16; using P = P16;
    const int w0 = blockIdx.x * P::ROWS, B = a.B, NN = a.NN, LO = a.lo_blk;
    const int whv = WHS >= 0 ? WHS : wh;
    P::Acc acc[FS_HS];
        const int nmlp = bh[FH_NMLP], flags = bh[FH_FLAGS];
        const uint8_t* maskbytes = reinterpret_cast<const uint8_t*>(a.ws + a.mask_off[l]);
        // lane constants rebuilt per layer from an opaque copy of the lane id: the per-node 64-bit addresses derived from them were hoisted out of
        // the layer loop and spilled, and a scratch reload next to the epilogue's pending stores is a full vmcnt(0) drain
        const int lq = opaque(lane);
        const int win = c_win(lq), w = w0 + win, col = wn * 32 + c_oct(lq), g8 = (lq >> 4) << 3;
        const bool w_ok = w < B;

        // phase 1 (each lane on the octets it owns): the accumulator of node n starts at its residual term G_{l+1}[n]; relu nodes are
        // then masked in place (both planes) -> dH_l[n]
        {
            unsigned mword[FS_HS]; u32x4 rawh[FS_HS], rawl[FS_HS]; int kindv[FS_HS];
#pragma unroll
            for (int u = 0; u < FS_HS; ++u) {
                const int n = 2 * u + whv;
                kindv[u] = n < NN ? bh[FH_KIND + n] : NK_DEAD;
                mword[u] = 0u; rawh[u] = u32x4{0, 0, 0, 0}; rawl[u] = u32x4{0, 0, 0, 0};
                if (kindv[u] == NK_RELU && w_ok) mword[u] = maskbytes[relu_byte(n, B, w, wn * 32 + g8)];
                if (kindv[u] != NK_DEAD) {
                    rawh[u] = *reinterpret_cast<const u32x4*>(smem + lds_chunk<T>(n, win, col / P::EPC));
                    rawl[u] = *reinterpret_cast<const u32x4*>(smem + lds_chunk<T>(LO + n, win, col / P::EPC));
                }
            }
#pragma unroll
            for (int u = 0; u < FS_HS; ++u) {
                const int n = 2 * u + whv;
                acc_fill(acc[u], 0.f);
                if (kindv[u] != NK_DEAD) {
                    if (bh[FH_RES + n]) join_oct(rawh[u], rawl[u], acc[u].c[0], acc[u].c[1]);
                    if (kindv[u] == NK_RELU) {
                        *reinterpret_cast<u32x4*>(smem + lds_chunk<T>(n, win, col / P::EPC)) = chunk_mask_bits<T>(rawh[u], mword[u]);
                        *reinterpret_cast<u32x4*>(smem + lds_chunk<T>(LO + n, win, col / P::EPC)) = chunk_mask_bits<T>(rawl[u], mword[u]);
                    }
                }
            }
        }
        __syncthreads();

        if (nmlp > 0) {
            // dT1 = dY W2 ; dU = dT1 . (T1 > 0) ; dH = dU W1     (backward of base_transform, in place on nodes 0..nmlp-1)
            const T* t1 = reinterpret_cast<const T*>(a.ws + a.t1_off[l]);
            T* du = reinterpret_cast<T*>(a.ws + a.du_off[l]);
            T* dh = reinterpret_cast<T*>(a.ws + a.dh_off[l]);
            P::BFrag bfh, bfl;
            P::Acc tm[2];
            u32x4 traw[2];
            load_bfrag<T>(bfh, wpack, bh[FH_W2], wn, lane);
            load_bfrag<T>(bfl, wpack, a.n_img + bh[FH_W2], wn, lane);
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int n = 2 * u + whv;
                traw[u] = u32x4{0, 0, 0, 0};
                acc_fill(tm[u], 0.f);
                if (n < nmlp && w_ok) traw[u] = *reinterpret_cast<const u32x4*>(t1 + x3_idx(w, n, B) + col);     // the hi half carries the sign of T1
            }
            mlp_mac3(tm, smem, 0, LO, nmlp, whv, bfh, bfl, lane);
            load_bfrag<T>(bfh, wpack, bh[FH_W1], wn, lane);
            load_bfrag<T>(bfl, wpack, a.n_img + bh[FH_W1], wn, lane);
            __syncthreads();   // all reads of the dY blocks done
            u32x4 duh[2] = {}, dul[2] = {};
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int n = 2 * u + whv;
                if (n < nmlp) {
                    f32x4 t0, t1v, r0, r1; unpack_oct(traw[u], t0, t1v);
#pragma unroll
                    for (int j = 0; j < 4; ++j) { r0[j] = t0[j] > 0.f ? tm[u].c[0][j] : 0.f; r1[j] = t1v[j] > 0.f ? tm[u].c[1][j] : 0.f; }
                    split_oct(r0, r1, duh[u], dul[u]);
                    *reinterpret_cast<u32x4*>(smem + lds_chunk<T>(n, win, col / P::EPC)) = duh[u];
                    *reinterpret_cast<u32x4*>(smem + lds_chunk<T>(LO + n, win, col / P::EPC)) = dul[u];
                    acc_fill(tm[u], 0.f);
                }
            }
            __syncthreads();
            mlp_mac3(tm, smem, 0, LO, nmlp, whv, bfh, bfl, lane);
            __syncthreads();   // all reads of the dU blocks done
            __builtin_amdgcn_s_waitcnt((7 << 4) | (15 << 8));
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int n = 2 * u + whv;
                if (n < nmlp) {
                    u32x4 hh, hl;
                    split_oct(tm[u].c[0], tm[u].c[1], hh, hl);
                    *reinterpret_cast<u32x4*>(smem + lds_chunk<T>(n, win, col / P::EPC)) = hh;
                    *reinterpret_cast<u32x4*>(smem + lds_chunk<T>(LO + n, win, col / P::EPC)) = hl;
                    if (w_ok) {
                        *reinterpret_cast<u32x4*>(du + x3_idx(w, n, B) + col) = duh[u];
                        *reinterpret_cast<u32x4*>(du + x3_idx(w, n, B) + H + col) = dul[u];
                        *reinterpret_cast<u32x4*>(dh + x3_idx(w, n, B) + col) = hh;
                        *reinterpret_cast<u32x4*>(dh + x3_idx(w, n, B) + H + col) = hl;
                    }
                }
            }
            __syncthreads();
        }

        // phase 2: dX_l[j] = (residual) + dH_j W_rootsum + sum_r sum_{j->i} dH_i W_rel^r
        fs_run<T>(wp, acc, smem, wpack, wn, lane);
        __syncthreads();   // every wave is done reading dH_l

        T* dxo = reinterpret_cast<T*>(a.ws + a.dx_off[l]);
        const uint8_t* m0 = reinterpret_cast<const uint8_t*>(a.ws + a.mask0_off);
        mid();      // next header / program landed before the stores go out (FProg::settle)
        // layer 0: the encoder's relu bytes of every node are requested before the first store of the epilogue (one round trip; a load waited for
        // while stores are in flight drains them all)
        unsigned xbv[FS_HS];
#pragma unroll
        for (int u = 0; u < FS_HS; ++u) {
            const int n = 2 * u + whv;
            xbv[u] = 0xffu;
            if ((flags & FF_ENC_MASK) && w_ok && n < NN && bh[FH_OUT + n]) xbv[u] = m0[relu_byte(n, B, w, wn * 32 + g8)];
        }
#pragma unroll
        for (int u = 0; u < FS_HS; ++u) {
            const int n = 2 * u + whv;
            if (n < NN && bh[FH_OUT + n]) {
                f32x4 y0 = acc[u].c[0], y1 = acc[u].c[1];
                if ((flags & FF_ENC_MASK) && w_ok) {   // layer 0: x relu'(X_0): the encoder's relu byte of this lane
                    const unsigned xb = xbv[u];
#pragma unroll
                    for (int j = 0; j < 4; ++j) { y0[j] = ((xb >> j) & 1u) ? y0[j] : 0.f; y1[j] = ((xb >> (4 + j)) & 1u) ? y1[j] : 0.f; }
                }
                u32x4 hi, lo;
                split_oct(y0, y1, hi, lo);
                if (l > 0) {
                    *reinterpret_cast<u32x4*>(smem + lds_chunk<T>(n, win, col / P::EPC)) = hi;
                    *reinterpret_cast<u32x4*>(smem + lds_chunk<T>(LO + n, win, col / P::EPC)) = lo;
                }
                if (w_ok) {
                    T* q = dxo + x3_idx(w, n, B) + col;
                    stash_store(q, hi, a.stash_nt != 0);
                    stash_store(q + H, lo, a.stash_nt != 0);
                }
            }
        }
        __syncthreads();
}
template <class SP, int WH, int l>
__device__ __forceinline__ void x3_bwd_layers_static(const StackArgs& a, char* smem, const T16* wpack, int wn, int lane) {
    if constexpr (l >= 0) {
        x3_bwd_layer<WH>(a, smem, wpack, wn, WH, lane, l, SHdr<SP, 1, l>{}, SProg<SP, 1, l, WH>{}, [] {});
        x3_bwd_layers_static<SP, WH, l - 1>(a, smem, wpack, wn, lane);
    }
}

template <bool STEP, class SP = void> __device__ __forceinline__ void stack_bwd_x3_body(const StackArgs& a, char* smem) {
    using T = T16; using P = P16;
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wn = wv & 3, wh = wv >> 2;
    const int w0 = blockIdx.x * P::ROWS, B = a.B, NN = a.NN, LO = a.lo_blk;
    const T* wpack = reinterpret_cast<const T*>(a.wpack);
    auto prog_of = [&](int l) { return STEP ? a.prog_off_b[l] : a.prog_off[l]; };

    // dX_L tile: only the nodes that are live in the last layer carry a gradient
    if constexpr (!STEP) {
        const FHdr bh(a.tables + prog_of(a.L - 1), lane);
        stage_tile_x3(smem, reinterpret_cast<const T*>(a.tile_in), NN, LO, w0, B, tid, [&](int n) { return bh[FH_KIND + n] != NK_DEAD; });
    }
    __syncthreads();

    if constexpr (std::is_void<SP>::value) {
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
            x3_bwd_layer<-1>(a, smem, wpack, wn, wh, lane, l, bh, wp, [&] { bhn.settle(); wpn.settle(); });
        }
    } else if (wh == 0) x3_bwd_layers_static<SP, 0, SP::L - 1>(a, smem, wpack, wn, lane);
    else x3_bwd_layers_static<SP, 1, SP::L - 1>(a, smem, wpack, wn, lane);
}
// mshgnn_step_mse on the split plan: both sweeps of a tile in one launch (k_slab_step of mshgnn.hip: dX_L stays in LDS, no second launch, no tile reload)
// SP: void = the plan's tables are interpreted; else the compile-time program of one (topology, depth) on the split plan (mshgnn_spec_tables.inc, X3_*)
template <bool ALIAS, class SP = void> __global__ __launch_bounds__(LAYER_THREADS, 2) void k_stack_step_x3(StackArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    stack_fwd_x3_body<ALIAS, true, SP>(a, smem);
    __syncthreads();
    stack_bwd_x3_body<true, SP>(a, smem);
}
// the forward launch alone (evaluation / first call of the two-call training route: what the nn.Module surface -- default precision "x3" -- runs) and the backward launch alone over
// the same programs; predicated stores like the interpreters', so ragged batches take them too.  Same MACs, same order: the interpreters' bits.
template <bool ALIAS, class SP> __global__ __launch_bounds__(LAYER_THREADS, 2) void k_stack_fwd_x3_spec(StackArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    stack_fwd_x3_body<ALIAS, false, SP>(a, smem);
}
template <class SP> __global__ __launch_bounds__(LAYER_THREADS, 2) void k_stack_bwd_x3_spec(StackArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    stack_bwd_x3_body<false, SP>(a, smem);
}

// Specialised stack kernels of the split plan: the three kernels above over the compile-time program of one (topology, depth) -- mshgnn_spec_tables.inc (X3_*), generated from
// this library's own plan compiler.  A plan takes one only when its fused tables are exactly the ints the kernel was compiled from.  The kernels are instantiated in translation
// units of their own (mshgnn_x3_spec_shard.hip with -DMSHGNN_SPEC_SHARD=1..7: csrc/Makefile), side by side with the rest; a shard exports one selector.
#include "mshgnn_spec_tables.inc"
using StackKernelX3 = void (*)(StackArgs);
template <class SP> static bool spec_matches_x3(const HostPlan& hp) {
    if (!hp.split || !hp.fused || hp.L != SP::L || hp.NN != SP::NN || (hp.x3_alias ? 1 : 0) != SP::ALIAS) return false;
    for (int l = 0; l < SP::L; ++l) {
        if (hp.fs_fwd_off[l] + SP::ROW > (int)hp.tables.size() || hp.fs_bwd_off[l] + SP::ROW > (int)hp.tables.size()) return false;
        if (memcmp(hp.tables.data() + hp.fs_fwd_off[l], SP::fwd[l], sizeof(int32_t) * SP::ROW) != 0) return false;
        if (memcmp(hp.tables.data() + hp.fs_bwd_off[l], SP::bwd[l], sizeof(int32_t) * SP::ROW) != 0) return false;
    }
    return true;
}
#define X3_SHARD_DECL(k) StackKernelX3 x3_spec_shard##k(const HostPlan& hp, int form, const char** name);      // form: pick::SpecFormX3 (mshgnn_pick.hpp)
SPEC_SHARD_LIST(X3_SHARD_DECL)
