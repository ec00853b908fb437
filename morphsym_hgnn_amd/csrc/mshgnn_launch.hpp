// The host side of a launch, once for the three precisions of the LDS-resident engine: what turns a StepCall into kernel arguments.  The fp32 / bf16 plans
// (forward_impl / backward_impl, mshgnn.hip) and the split-bf16 plan (x3_forward / x3_backward, mshgnn_x3.hip) keep their own launch tables; every argument struct they
// pass is filled here, and which row of a table a launch takes is mshgnn_pick.hpp's decision (pick_stack / pick_enc), queried and applied here.  What differs between the
// plans is a LaunchTraits constant, never a second copy of a fill.
#pragma once
#include "mshgnn_device.hpp"
#include "mshgnn_pick.hpp"

struct LaunchTraits {
    int in_bytes;           // element size of the encoder's input rows (the split plan reads fp32)
    int in_epc;             // ... and their elements per 16-byte chunk
    int pack_epc;           // elements per 16-byte chunk of a weight image
    int blk;                // bytes of one LDS node block
    int enc_windows;        // windows per encoder workgroup
    int enc_lds;            // dynamic LDS of the encoder launch
    int gw_windows;         // windows per step of the weight-gradient kernel
    bool split;             // hi / lo weight images: the plan's pack list holds both planes, a launch names the images of one (hp.n_img)
    bool embed_prep;        // the encoder launch can pack the layer images under its tail (EncArgs.prep)
    // kept differences between the plans
    bool src_routes;        // the encoder gathers from a series or converts wide sources; fp32 plan: no series route, wide sources refused
    bool wide_needs_rows;   // wide sources: aligned plan-dtype rows must be given (split plan); else they are checked only where x is given
    bool gradw_series;      // the weight-gradient kernel can gather raw operands from the series (StepCall.gradw_from_series); split plan: always materialised rows
    const char* series_rows_err;      // the series route's refusal of unaligned window rows
    const char* wide_rows_err;        // the wide route's
};

inline int plan_packs(const HostPlan& hp, const LaunchTraits& tr) { return tr.split ? hp.n_img : (int)hp.packs.size(); }

// ---- weight images: which packs the launch in front of the encoder takes, which ones the encoder's extra workgroups
using PrepLaunch = void (*)(const PrepArgs&, bool biases, hipStream_t);      // the plan's k_prep* launch (per-thread or tiled kernel: prep_use_tiled)
inline unsigned prep_grid(const PrepArgs& a, int pack_epc, bool biases) {      // per-thread kernel: one thread per output vector of the launch's packs (+ one per bias element)
    const int64_t total = (int64_t)(a.pack_n < 0 ? a.n_packs : a.pack_n) * (H * H / pack_epc) + (biases ? (int64_t)a.n_biases * H : 0);
    return (unsigned)((total + 255) / 256);
}
struct PrepSplit {
    bool embed;             // few packs: only the encoder's packs (the last ones of the list) + the biases in front; the layer packs [0, enc_pack0) under the encoder's tail --
    int enc_pack0;          // the whole-list launch in front of the encoder cost 10.9 us
    PrepArgs front, layers; // the launch in front of the encoder; the embedded part (embed only)
};
inline PrepSplit enc_prep_split(const mshgnn_plan* p, const StepCall& c, const mshgnn_ws_layout& lay, const LaunchTraits& tr) {
    const HostPlan& hp = p->hp;
    PrepSplit s{};
    const PrepArgs all{c.params, c.ws + lay.wpack, reinterpret_cast<float*>(c.ws + lay.bias), p->d_packs, p->d_biases, plan_packs(hp, tr), (int)hp.biases.size()};
    s.enc_pack0 = all.n_packs;
    for (int t = 0; t < hp.NT; ++t) if (hp.pack_enc_base[t] >= 0) s.enc_pack0 = std::min(s.enc_pack0, hp.pack_enc_base[t]);
    static const bool embed_off = TUNE_ENV("MSHGNN_PREP_EMBED") && atoi(TUNE_ENV("MSHGNN_PREP_EMBED")) == 0;      // (A/B runs)
    s.embed = tr.embed_prep && !c.series && !prep_use_tiled(all.n_packs) && s.enc_pack0 > 0 && !embed_off;
    s.front = s.layers = all;
    if (s.embed) { s.front.pack0 = s.enc_pack0; s.front.pack_n = all.n_packs - s.enc_pack0; s.layers.pack0 = 0; s.layers.pack_n = s.enc_pack0; }
    return s;
}

// ---- encoder.  Returns the pitch error as the entry points report it; grid = the encoder's own workgroups + those of an embedded prep.  An embedded prep needs the
// aligned encoder: where the rows are not aligned a.prep_vecs stays 0 and the layer images are packed in front of the encoder after all (prep_and_enc_args).
inline int fill_enc_args(const mshgnn_plan* p, const StepCall& c, const mshgnn_ws_layout& lay, const LaunchTraits& tr, const PrepSplit& ps, EncArgs& a, unsigned& grid) {
    const HostPlan& hp = p->hp;
    const mshgnn_desc& d = hp.d;
    char* ws = c.ws;
    a.n_types = hp.NT; a.B = (int)c.batch; a.NN = hp.NN; a.tiles = (a.B + tr.enc_windows - 1) / tr.enc_windows;
    a.wg_prefix[0] = 0;
    const bool all_rows = c.series != nullptr && c.x != nullptr;
    for (int t = 0; t < hp.NT; ++t) {
        a.x[t] = c.x ? c.x[t] : nullptr; a.pitch[t] = c.x_pitch ? c.x_pitch[t] : d.type_width[t];      // (x == NULL: a series / wide route that materialises nothing)
        if (a.pitch[t] < d.type_width[t]) return set_err(MSHGNN_EINVAL, "x_pitch smaller than the feature width");
        a.vb[t] = vec_bytes(a.x[t], a.pitch[t], tr.in_bytes);
        if (t == 0) a.aligned = 1;
        if (a.vb[t] != 16 || a.pitch[t] % tr.in_epc) a.aligned = 0;
        a.width[t] = d.type_width[t]; a.tbase[t] = hp.type_base[t]; a.nkc[t] = hp.enc_nkc[t];
        a.pack0[t] = hp.pack_enc_base[t]; a.bias_idx[t] = hp.bias_enc[t]; a.sign_off[t] = hp.sign_off[t];
        // the launch's nodes of this type: those whose X_0 can reach the output; with window rows to materialise (series route, x given) every node,
        // the others marked in skip_mask
        a.node_off[t] = t == 0 ? 0 : a.node_off[t - 1] + a.nodes[t - 1];
        a.nodes[t] = 0;
        for (int i = 0; i < d.type_nodes[t]; ++i) {
            const bool need = hp.need_n[0][hp.type_base[t] + i];
            if (need || all_rows) a.node_list[a.node_off[t] + a.nodes[t]++] = (unsigned char)i;
            if (!need) a.skip_mask |= 1ull << (hp.type_base[t] + i);
        }
        a.wg_prefix[t + 1] = a.wg_prefix[t] + a.nodes[t] * a.tiles;
    }
    a.tbase[hp.NT] = hp.NN;
    a.wpack = ws + lay.wpack; a.bias = reinterpret_cast<const float*>(ws + lay.bias); a.signs = p->d_signs; a.x0 = ws + lay.x[0];
    a.mask0 = (c.training && lay.dd[0]) ? reinterpret_cast<uint8_t*>(ws + lay.dd[0]) : nullptr;
    grid = (unsigned)a.wg_prefix[hp.NT];
    if (ps.embed && a.aligned) { a.prep = ps.layers; a.prep_vecs = ps.enc_pack0 * (H * H / tr.pack_epc); grid += (unsigned)((a.prep_vecs + 255) / 256); }
    return MSHGNN_OK;
}

// steps 1 and 2 of a forward up to the encoder launch: the prep launch(es) on the stream, the encoder's arguments and grid
inline int prep_and_enc_args(const mshgnn_plan* p, const StepCall& c, const mshgnn_ws_layout& lay, const LaunchTraits& tr, PrepLaunch launch, EncArgs& a, unsigned& grid) {
    const PrepSplit ps = enc_prep_split(p, c, lay, tr);
    auto prep = [&](const PrepArgs& pa, bool biases) { ProfScope scope(p, p->hp.ks_prep, c.stream); launch(pa, biases, c.stream); };
    prep(ps.front, true);
    if (int rc = fill_enc_args(p, c, lay, tr, ps, a, grid)) return rc;
    if (ps.embed && !a.prep_vecs) prep(ps.layers, false);      // the element-wise encoder has no embedded prep: pack the layer images in front of it after all
    return MSHGNN_OK;
}

// where the encoder's rows come from: the facts of the call for pick_enc (mshgnn_pick.hpp), its refusals in this plan's words.  Adds the label workgroups of a series
// route to the grid; form: the row of the plan's encoder table (pick::EncForm).
inline int pick_enc_form(const StepCall& c, const EncArgs& a, const LaunchTraits& tr, unsigned& grid, int& form) {
    pick::EncFacts f;
    f.series = c.series != nullptr; f.wide_bytes = c.wide ? (c.wide->bytes == 8 ? 8 : 4) : 0; f.x_given = c.x != nullptr; f.aligned = a.aligned != 0;
    if (c.series) { f.stats = c.series->stats != nullptr; f.sign = c.series->sign; f.label_rows = (int)c.series->lab.B; }
    f.src_routes = tr.src_routes; f.wide_needs_rows = tr.wide_needs_rows;
    const pick::EncPick pk = pick::pick_enc(f);
    if (pk.err == MSHGNN_EUNSUPPORTED) return set_err(pk.err, "wide source rows: not on the fp32 plan (cast the inputs)");
    if (pk.err) return set_err(pk.err, c.series ? tr.series_rows_err : tr.wide_rows_err);
    grid += pk.label_wgs; form = pk.form;
    return MSHGNN_OK;
}
// the sources an encoder form reads (the others stay empty)
inline SeriesSrc enc_series_src(const StepCall& c, int form) { return pick::enc_form_series(form) ? *c.series : SeriesSrc{}; }
inline WideSrc enc_wide_src(const StepCall& c, int form) { return pick::enc_form_wide(form) ? *c.wide : WideSrc{}; }

// ---- decoder backward (the launch of its own: two-call training, plans without a fused tail)
inline void fill_dec_bwd_args(const mshgnn_plan* p, const StepCall& c, const mshgnn_ws_layout& lay, DecArgs& a) {
    const HostPlan& hp = p->hp;
    const mshgnn_desc& d = hp.d;
    char* ws = c.ws;
    a.xl = ws + lay.x[hp.L]; a.dxl = ws + lay.dx[hp.L]; a.params = c.params; a.out_mask = p->d_out_mask; a.gout = c.grad_out;
    a.slabs = reinterpret_cast<float*>(ws + lay.dec_slabs); a.off_w = d.off_dec_w; a.off_b = d.off_dec_b;
    a.B = (int)c.batch; a.NN = hp.NN; a.node0 = hp.type_base[d.out_type]; a.n_out = d.type_nodes[d.out_type]; a.dout = d.out_channels; a.slab0 = 0;
    if (c.loss == LossKind::MSE) { a.y = c.y; a.out = c.out; a.loss = c.loss_out; a.inv_n = 1.0f / (float)(c.total_windows() * a.n_out * a.dout); a.reg_kind = c.reg_kind; a.reg_delta = c.reg_delta; }
    if (c.loss == LossKind::CE) { a.labels = c.labels; a.out = c.out; a.loss = c.loss_out; a.inv_n = 1.0f / (float)(c.total_windows() * a.n_out); }
}

// ---- stack kernels: what forward, backward and one-launch step share (offsets a launch does not read cost nothing).  tile_in, training, the programs (prog_off*),
// mask0_off and the plan's own fields (bf16: dbg, stagger; split: lo_blk, n_img, scr0) stay with the caller.
inline void fill_stack_common(const mshgnn_plan* p, const StepCall& c, const mshgnn_ws_layout& lay, StackArgs& a) {
    const HostPlan& hp = p->hp;
    a.ws = c.ws;
    for (int l = 0; l <= hp.L; ++l) { a.x_off[l] = lay.x[l]; a.dx_off[l] = lay.dx[l]; }
    for (int l = 0; l < hp.L; ++l) { a.mask_off[l] = lay.mask[l]; a.hb_off[l] = lay.hb[l]; a.t1_off[l] = lay.t1[l]; a.dh_off[l] = lay.dh[l]; a.du_off[l] = lay.du[l]; }
    a.wpack = c.ws + lay.wpack; a.bias = reinterpret_cast<const float*>(c.ws + lay.bias); a.tables = p->d_tables;
    a.B = (int)c.batch; a.NN = hp.NN; a.L = hp.L;
    a.node0 = hp.type_base[hp.d.out_type]; a.n_out = hp.d.type_nodes[hp.d.out_type];      // the nodes that carry X_L / dX_L (the only live type of the last layer)
    a.stash_nt = stash_nt_for(p->stash_nt_force, c.batch, stash_rows_of(hp), H * 2);      // (counted per row of 256 bytes on both plans: stash_nt_for)
}
// the forward's tail: decoder, and with a fused loss (one-call steps) loss and decoder backward -- c.dec_done tells the backward
inline void fill_stack_tail(const mshgnn_plan* p, StepCall& c, const mshgnn_ws_layout& lay, StackArgs& a) {
    const mshgnn_desc& d = p->hp.d;
    a.params = c.params; a.out_mask = p->d_out_mask; a.out = c.out; a.off_dec_w = d.off_dec_w; a.off_dec_b = d.off_dec_b; a.dout = d.out_channels;
    if (c.y_fused()) {
        a.y = c.y_fused(); a.dec_slabs = reinterpret_cast<float*>(c.ws + lay.dec_slabs);
        a.inv_n = 1.0f / (float)(c.total_windows() * a.n_out * a.dout);
        a.reg_kind = c.reg_kind; a.reg_delta = c.reg_delta;
    } else if (c.labels_fused()) {      // mshgnn_step_ce: cross entropy over the per-foot logit pairs, mean over B * n_out rows
        a.labels = c.labels_fused(); a.dec_slabs = reinterpret_cast<float*>(c.ws + lay.dec_slabs);
        a.inv_n = 1.0f / (float)(c.total_windows() * a.n_out);
    }
    c.dec_done = c.y_fused() || c.labels_fused();
}
// ---- the stack launch: the pick's query from the plan and the call (every use_* / slab / program switch of the plan is read here and nowhere else on the launch path),
// the pick's fields into the kernel arguments, the launch of the picked row
using StackKernelFn = void (*)(StackArgs);
inline pick::StackQuery stack_query(const mshgnn_plan* p, const StepCall& c, int plan, int op, int blk, const StackArgs& a) {
    const HostPlan& hp = p->hp;
    pick::StackQuery q;
    q.plan = plan; q.op = op; q.B = (int)c.batch; q.n_cu = p->n_cu;
    q.use_fused = p->use_fused; q.use_slab = p->use_slab; q.slab_force = p->slab_force; q.use_spec = p->use_spec; q.use_step = p->use_step;
    // L1 / Huber on the bf16 plan: the interpreting kernels.  The compile-time programs' tails are compiled for MSE and cross entropy alone (decoder_tail_impl, KS), so that the
    // MSE path of the tuned kernels carries nothing of the other kinds; same tables, same stashes, same bits (tests/test_spec_gpu.py), so a forward over the program and a
    // backward_mse over the interpreter go together.
    if (plan == pick::PLAN_BF16 && c.loss == LossKind::MSE && c.reg_kind != MSHGNN_REG_LOSS_MSE) q.use_spec = false;
    q.stash_nt = a.stash_nt; q.gw_phase = c.gw_phase;
    q.n_mlp = hp.n_mlp; q.sl_hb = hp.sl_hb; q.sl_blk = hp.sl_blk; q.fs_blk = hp.fs_blk; q.x3_alias = hp.x3_alias;
    q.node0 = a.node0; q.n_out = a.n_out; q.blk = blk; q.stagger = p->stagger; q.extra_blk = FS_EXTRA_BLK;
    return q;
}
inline int forward_op(const StepCall& c) { return c.dec_done ? pick::OP_FWD_LOSS : c.training ? pick::OP_FWD_TRAIN : pick::OP_FWD_EVAL; }
// program tables, scratch offset, store policy and stagger of the picked launch
inline void apply_stack_pick(const HostPlan& hp, const pick::StackPick& pk, const mshgnn_ws_layout& lay, StackArgs& a) {
    const int* fwd = pk.slab_prog ? hp.sl_fwd_off : hp.fs_fwd_off;
    const int* bwd = pk.slab_prog ? hp.sl_bwd_off : hp.fs_bwd_off;
    for (int l = 0; l < hp.L; ++l) { a.prog_off[l] = pk.what == pick::BWD ? bwd[l] : fwd[l]; if (pk.what == pick::STEP) a.prog_off_b[l] = bwd[l]; }
    if (pk.what != pick::FWD) a.mask0_off = lay.dd[0];
    a.red_off = pk.red_off; a.stash_nt = pk.stash_nt; a.stagger = pk.stagger;
}
inline int launch_stack(StackKernelFn kernel, const pick::StackPick& pk, hipStream_t st, const StackArgs& a) {
    if (!kernel) return set_err(MSHGNN_EHIP, std::string("no kernel in the launch table for ") + pick::kernel_name(pk.family, pk.k));
    hipLaunchKernelGGL(kernel, dim3(pk.tiles), dim3(pk.threads), pk.lds, st, a);
    HIPCHK(hipGetLastError());
    return MSHGNN_OK;
}

// ---- weight gradients: every lane of the step, or the lanes of one phase of a two-phase step (c.gw_phase)
// ---- finalize work of a step: the mean the fused loss is scaled by, and how many decoder partial slabs there are (one per tile from a fused forward, else k_dec_bwd's)
inline float fin_inv_n(const HostPlan& hp, const StepCall& c) {
    const mshgnn_desc& d = hp.d;
    return 1.0f / (float)(c.total_windows() * d.type_nodes[d.out_type] * (c.loss == LossKind::CE ? 1 : d.out_channels));
}
inline int fin_n_dec(const StepCall& c) { return c.dec_done ? (int)((c.batch + TILE_ROWS - 1) / TILE_ROWS) : NWG_DEC; }
inline bool fin_split(const HostPlan& hp) { return hp.d.dtype != MSHGNN_F32; }      // bf16 / split plan: slab-free ops in the weight-gradient launch, k_finalize sums slabs only

// The slab-free finalize ops of this call's finalize range as extra workgroups of its weight-gradient launch: the decoder sums and the loss where the whole step or
// phase 0 runs, the zero fills of the range unless a sub-step of a chunked step accumulates (the first sub-step has written them).
// They come FIRST in the grid, padded to a multiple of 8 workgroups: the launch's own workgroups keep their index modulo 8, which is the XCD the plan placed each lane on
// (lane_order; unpadded, 122 of them in front of A1-C2's 448 cost the launch 66.8 -> 70.6 us: HISTORY.md).  n_main: the launch's own workgroups.
inline void fill_gradw_side(const mshgnn_plan* p, const StepCall& c, const mshgnn_ws_layout& lay, int n_main, GwSide& s) {
    const HostPlan& hp = p->hp;
    s = GwSide{};
    if (!fin_split(hp) || !c.grad_params) return;
    int first = 0, n = hp.n_side_dec;      // records: [decoder sums | zero fills of phase 0 | zero fills of phase 1]
    if (!c.accumulates()) n += hp.n_side_zero[0] + (c.gw_phase == 0 ? 0 : hp.n_side_zero[1]);
    if (c.gw_phase == 1) { first = hp.n_side_dec + hp.n_side_zero[0]; n = c.accumulates() ? 0 : hp.n_side_zero[1]; }
    static const int where = [] { const char* e = TUNE_ENV("MSHGNN_GW_SIDE"); return e ? atoi(e) : 0; }();      // (A/B runs: 1 = last in the grid, 2 = first without the padding)
    s.recs = p->d_tables + hp.side_off + (size_t)first * SIDE_INTS; s.n = n;
    s.n_grid = where == 0 ? (n + 7) / 8 * 8 : n; s.wg0 = where == 1 ? n_main : 0; s.main0 = where == 1 ? 0 : s.n_grid;
    s.dec_slabs = reinterpret_cast<const float*>(c.ws + lay.dec_slabs); s.grad = c.grad_params;
    s.loss = c.loss != LossKind::NONE && c.gw_phase != 1 ? c.loss_out : nullptr;
    s.inv_n = fin_inv_n(hp, c); s.n_dec = fin_n_dec(c); s.accumulate = c.accumulates();
}

inline void fill_gradw_args(const mshgnn_plan* p, const StepCall& c, const mshgnn_ws_layout& lay, const LaunchTraits& tr, int gw_parts, GradwArgs& a) {
    const HostPlan& hp = p->hp;
    const mshgnn_desc& d = hp.d;
    a.ws = c.ws;
    for (int l = 0; l <= hp.L; ++l) { a.buf_off[BUF_X + l] = lay.x[l]; a.buf_off[BUF_DX + l] = lay.dx[l]; }
    for (int l = 0; l < hp.L; ++l) a.buf_off[BUF_MASK + l] = lay.mask[l];
    for (int l = 0; l < hp.L; ++l) { a.buf_off[BUF_DH + l] = lay.dh[l]; a.buf_off[BUF_HB + l] = lay.hb[l]; a.buf_off[BUF_T1 + l] = lay.t1[l]; a.buf_off[BUF_DU + l] = lay.du[l]; }
    for (int t = 0; t < hp.NT; ++t) {
        a.x[t] = c.x ? c.x[t] : nullptr; a.pitch[t] = c.x_pitch ? c.x_pitch[t] : d.type_width[t]; a.nodes[t] = d.type_nodes[t];
        a.vb[t] = vec_bytes(a.x[t], a.pitch[t], tr.in_bytes);
        if (t == 0) a.aligned = 1;
        if (a.vb[t] != 16 || a.pitch[t] % tr.in_epc) a.aligned = 0;
    }
    if (tr.gradw_series && c.gradw_from_series && c.series) a.ser = *c.series;      // (bf16 plan only: raw operands gathered from the series, nothing was materialised)
    a.items = p->d_tables + hp.item_off; a.lanes = p->d_tables + hp.lane_off; a.lane_order = p->d_tables + hp.lane_order_off; a.n_pad = hp.n_lanes_pad;
    if (c.gw_phase >= 0) { a.lane_order = p->d_tables + hp.order_ph_off[c.gw_phase]; a.n_pad = hp.npad_ph[c.gw_phase]; }
    a.signs = p->d_signs; a.slabs = reinterpret_cast<float*>(c.ws + lay.slabs); a.B = (int)c.batch; a.n_lanes = hp.n_lanes; a.n_parts = gw_parts;
    fill_gradw_side(p, c, lay, std::max(a.n_pad, 0) * gw_parts, a.side);
    // (dbg / stamps stay zero: no weight-gradient kernel of this engine reads them)
}
