// Which kernel a launch of the LDS-resident engine gets: the stack launch of the three plans (pick_stack) and the encoder launch (pick_enc), as pure functions over
// plain ints.  Host only, no HIP types (g++ compiles it into libmshgnn_hostplan.so; tests/test_resident_pick.py pins it on the CPU).  mshgnn.hip / mshgnn_x3.hip fill a
// query, launch row `k` of the picked family's table with the pick's grid, block and LDS, copy the pick's fields into the kernel arguments and decide nothing else.
#pragma once
#include "mshgnn_plan.hpp"

namespace mshgnn { namespace pick {

enum Plan : int { PLAN_F32, PLAN_BF16, PLAN_X3 };
enum Op : int { OP_FWD_EVAL, OP_FWD_TRAIN, OP_BWD, OP_FWD_LOSS };      // FWD_LOSS: a training forward with a fused loss (StepCall.dec_done after fill_stack_tail)
enum Family : int { PER_LAYER, STACK8, SLAB, SLAB_SPEC, X3, X3_SPEC, FAMILY_COUNT };
enum What : int { FWD, BWD, STEP };
constexpr int STACK8_THREADS = 512;      // (= LAYER_THREADS of mshgnn_device.hpp: the per-layer, 8-wave and split-plan kernels)

// ---- the specialised forms that exist over a compile-time program.  kind 0: one-call step, 1: forward alone (tr: training), 2: backward alone; nt: the stash store policy;
// full: the batch is whole 16-window tiles (unpredicated stores).  bf16 plan: both store policies on whole tiles; on a ragged batch the predicated forms that exist -- the
// one-call step with plain stash stores (a ragged batch whose stash wants non-temporal stores keeps the interpreter: the weight-gradient launch behind plain stores loses more
// than the program wins at 8 layers) and the evaluation forward (predication is free at 3 layers and costs 22-27 % on the 8-layer programs, hence both forms); the two-call
// training route of a ragged batch keeps the interpreters (-1).  Split plan: one form per kind, predicated stores like its interpreters' (ragged batches run them too).
enum SpecForm : int { SF_STEP, SF_STEP_NT, SF_STEP_RAGGED, SF_EVAL, SF_EVAL_RAGGED, SF_TRAIN, SF_TRAIN_NT, SF_BWD, SF_BWD_NT, SPEC_FORMS };
enum SpecFormX3 : int { SFX_STEP, SFX_FWD, SFX_BWD, SPEC_FORMS_X3 };
constexpr int spec_form(int plan, int kind, int tr, int nt, int full) {
    if (plan == PLAN_X3) return kind >= 0 && kind <= 2 ? kind : -1;
    if (plan != PLAN_BF16 || kind < 0 || kind > 2) return -1;
    if (kind == 0) return full ? (nt ? SF_STEP_NT : SF_STEP) : (nt ? -1 : SF_STEP_RAGGED);
    if (kind == 1 && !tr) return full ? SF_EVAL : SF_EVAL_RAGGED;      // (an evaluation stashes nothing: no store policy)
    if (!full) return -1;
    return (kind == 1 ? SF_TRAIN : SF_BWD) + (nt ? 1 : 0);
}

// ---- table rows and their names
constexpr int slab_nm(int n_mlp) { return n_mlp <= 2 ? 2 : 4; }                   // bound on the base_transform nodes
constexpr int slab_hb(int sl_hb) { return sl_hb <= SL_HB ? SL_HB : SL_HB_MAX; }      // group-B slots
constexpr int slab_row(int what, int nm, int hb) { return what * 4 + (nm == 4 ? 2 : 0) + (hb == SL_HB_MAX ? 1 : 0); }      // [what][NM in {2, 4}][HB in {SL_HB, SL_HB_MAX}]
enum X3Row : int { X3_FWD, X3_FWD_ALIAS, X3_BWD, X3_STEP, X3_STEP_ALIAS, X3_ROWS };
constexpr int STACK8_ROWS = 3, SLAB_ROWS = 12, PER_LAYER_ROWS = 2;
constexpr const char* PER_LAYER_NAMES[PER_LAYER_ROWS] = {"k_layer_fwd<T>", "k_layer_bwd<T>"};
constexpr const char* STACK8_NAMES[STACK8_ROWS] = {"k_stack_fwd<bf16>", "k_stack_bwd<bf16>", "k_stack_step<bf16>"};
constexpr const char* SLAB_NAMES[SLAB_ROWS] = {
    "k_slab_fwd<bf16,2,SL_HB>", "k_slab_fwd<bf16,2,SL_HB_MAX>", "k_slab_fwd<bf16,4,SL_HB>", "k_slab_fwd<bf16,4,SL_HB_MAX>",
    "k_slab_bwd<bf16,2,SL_HB>", "k_slab_bwd<bf16,2,SL_HB_MAX>", "k_slab_bwd<bf16,4,SL_HB>", "k_slab_bwd<bf16,4,SL_HB_MAX>",
    "k_slab_step<bf16,2,SL_HB>", "k_slab_step<bf16,2,SL_HB_MAX>", "k_slab_step<bf16,4,SL_HB>", "k_slab_step<bf16,4,SL_HB_MAX>"};
constexpr const char* SLAB_SPEC_NAMES[SPEC_FORMS] = {
    "k_slab_step<SP,NT=0,FULL>", "k_slab_step<SP,NT=1,FULL>", "k_slab_step<SP,NT=0,RAGGED>", "k_slab_fwd_spec<SP,TR=0,NT=0,FULL>", "k_slab_fwd_spec<SP,TR=0,NT=0,RAGGED>",
    "k_slab_fwd_spec<SP,TR=1,NT=0,FULL>", "k_slab_fwd_spec<SP,TR=1,NT=1,FULL>", "k_slab_bwd_spec<SP,NT=0>", "k_slab_bwd_spec<SP,NT=1>"};
constexpr const char* X3_NAMES[X3_ROWS] = {"k_stack_fwd_x3<false>", "k_stack_fwd_x3<true>", "k_stack_bwd_x3", "k_stack_step_x3<false>", "k_stack_step_x3<true>"};
constexpr const char* X3_SPEC_NAMES[SPEC_FORMS_X3] = {"k_stack_step_x3<ALIAS,SP>", "k_stack_fwd_x3_spec<ALIAS,SP>", "k_stack_bwd_x3_spec<SP>"};
constexpr int family_rows(int family) {
    return family == PER_LAYER ? PER_LAYER_ROWS : family == STACK8 ? STACK8_ROWS : family == SLAB ? SLAB_ROWS : family == SLAB_SPEC ? (int)SPEC_FORMS : family == X3 ? (int)X3_ROWS :
           family == X3_SPEC ? (int)SPEC_FORMS_X3 : 0;
}
inline const char* kernel_name(int family, int k) {
    if (k < 0 || k >= family_rows(family)) return "";
    return family == PER_LAYER ? PER_LAYER_NAMES[k] : family == STACK8 ? STACK8_NAMES[k] : family == SLAB ? SLAB_NAMES[k] : family == SLAB_SPEC ? SLAB_SPEC_NAMES[k] :
           family == X3 ? X3_NAMES[k] : X3_SPEC_NAMES[k];
}

// One-launch step: the tail's reduction scratch (red_need bytes: one decoder slab per wave) must not touch the out-type nodes' blocks, which receive dX_L for the backward
// sweep.  It sits in the blocks in front of them, or (models whose out type comes first: the centroidal-momentum ones) in the blocks behind them, inside lds_extent
// (bf16: the launch's LDS; split plan: the hi plane).  Returns its byte offset, or -1: neither fits, no one-launch step.
constexpr int place_red_scratch(int node0, int n_out, int blk_bytes, int64_t red_need, int64_t lds_extent) {
    const int64_t red_back = (int64_t)(node0 + n_out) * blk_bytes;
    if ((int64_t)node0 * blk_bytes >= red_need) return 0;
    return red_back + red_need <= lds_extent ? (int)red_back : -1;
}
constexpr int64_t red_need(int threads) { return (int64_t)(threads / 64) * DEC_SLAB_FLOATS * (int64_t)sizeof(float); }

struct StackQuery {
    int plan = PLAN_BF16, op = OP_FWD_EVAL;
    int B = 0, n_cu = 256;
    bool use_fused = false, use_slab = false, slab_force = false;      // MSHGNN_FUSED / MSHGNN_SLAB at plan creation (slab_force: MSHGNN_SLAB=2)
    bool use_spec = false;      // the plan has a compile-time program (built in, or attached) and MSHGNN_SPEC is not 0
    bool use_step = false;      // MSHGNN_STEP_KERNEL is not 0
    int stash_nt = 0;           // stash_nt_for, as fill_stack_common computed it
    int gw_phase = -1;
    int n_mlp = 0, sl_hb = 0, sl_blk = 0, fs_blk = 0;
    bool x3_alias = false;
    int node0 = 0, n_out = 0, blk = 0;      // the out type's first node block and block count; bytes of one LDS node block
    int stagger = 0;            // the plan's MSHGNN_STAGGER
    int extra_blk = 0;          // FS_EXTRA_BLK of the build (instrumented builds: LDS room for the per-segment clocks)
};
struct StackPick {
    int family = PER_LAYER, what = FWD;
    int NM = 0, HB = 0, NT = 0, TR = 0, FULL = 0, ALIAS = 0;      // the row's template coordinates (0 where the family has none)
    int k = 0;                  // row of the family's launch table
    int threads = STACK8_THREADS, lds = 0, tiles = 0;      // (PER_LAYER: lds 0 -- the layer loops launch with the plan's n_blk blocks)
    bool slab_prog = false;     // the launch reads the slab program tables (sl_fwd_off / sl_bwd_off), else the fused ones (fs_*)
    int red_off = 0;            // STEP: byte offset of the tail's reduction scratch
    int stash_nt = 0;           // the launch's stash store policy
    int stagger = 0;
};

// A slab workgroup has 4 waves for a whole tile (a lone one is ~12 % slower than the 8-wave kernels' workgroup: 69 against 62 us at 3 layers), two fit a CU: the interpreting
// slab kernels pay off from the first tile the 8-wave kernels would need a second round for (257 .. 383 tiles, 8-wave against slab launch: 113 / 77 us at 3 layers, 425 / 295
// at 8, MiniCheetah-K4 440 / 330 -- tools/slab_threshold_sweep.py; rounds 3-4 switched at 1.5 tiles per CU).  MSHGNN_SLAB=2: at every batch.
constexpr bool slab_for(const StackQuery& q, int tiles) { return q.use_slab && (q.slab_force || tiles > q.n_cu); }

inline StackPick pick_stack(const StackQuery& q) {
    StackPick r;
    const int tiles = (q.B + TILE_ROWS - 1) / TILE_ROWS;
    const bool bwd = q.op == OP_BWD, training = q.op != OP_FWD_EVAL, full = q.B > 0 && q.B % TILE_ROWS == 0;
    r.tiles = tiles; r.what = bwd ? BWD : FWD; r.stash_nt = q.stash_nt;
    if (q.plan == PLAN_F32 || !q.use_fused) { r.k = r.what; return r; }      // one kernel per layer (the fp32 plan; MSHGNN_FUSED=0)
    if (q.plan == PLAN_X3) {
        // the split plan has only 8-wave kernels; its program's kernels have predicated stores, so every batch takes them.  A two-phase step (gw_phase >= 0) keeps the
        // backward sweep a launch of its own on this plan (the bf16 plan has no such condition); an evaluation leaves the store policy set.
        r.lds = 2 * q.fs_blk * q.blk;
        const int red = !bwd && q.gw_phase < 0 && q.op == OP_FWD_LOSS && q.use_step ? place_red_scratch(q.node0, q.n_out, q.blk, red_need(STACK8_THREADS), (int64_t)q.fs_blk * q.blk) : -1;
        if (red >= 0) { r.what = STEP; r.red_off = red; }
        r.family = q.use_spec ? X3_SPEC : X3;
        r.ALIAS = r.what != BWD && q.x3_alias ? 1 : 0;      // (the backward kernels have no such form)
        r.k = q.use_spec ? (r.what == STEP ? SFX_STEP : r.what == FWD ? SFX_FWD : SFX_BWD) : r.what == BWD ? X3_BWD : (r.what == STEP ? X3_STEP : X3_FWD) + r.ALIAS;
        return r;
    }
    const bool big = slab_for(q, tiles), spec = q.use_slab && q.use_spec;
    r.stagger = big && tiles > q.n_cu ? q.stagger : 0;      // (MSHGNN_SLAB=2 below one tile per CU: one workgroup per CU, nothing to stagger)
    if (!training) r.stash_nt = 0;      // an evaluation stashes nothing
    const int nt = r.stash_nt;
    bool slab = big;
    int form = -1;
    if (bwd) {      // the backward alone on its program at every whole-tile batch size, like the forward
        if (spec) form = spec_form(PLAN_BF16, 2, 1, nt, full);
    } else {
        // Slab or 8-wave kernels: the 8-wave ones take batches of at most one tile per CU -- unless the one-call step has a compile-time program for this launch: a single
        // tile's chain on the specialised slab kernel is 37-42 us where the interpreting 8-wave kernel takes 57-62 (A1-C2, 32 .. 4 096 windows; 8 layers: 140-166 against
        // 202-209; 32 windows 0.0828 -> 0.0626 ms/step, 4 096: 0.131 -> 0.114, 30: 0.083 -> 0.063, 8 190: 0.209 -> 0.183), so the specialised step runs at every batch
        // size.  MSHGNN_SLAB=0 / MSHGNN_SPEC=0 keep the 8-wave kernels there.  A step needs the tail's reduction scratch beside the out-type blocks of its family's LDS.
        const bool want_step = q.use_step && q.op == OP_FWD_LOSS;
        const int step_form = spec ? spec_form(PLAN_BF16, 0, 1, nt, full) : -1;
        auto red = [&](bool on_slab) {
            return place_red_scratch(q.node0, q.n_out, q.blk, red_need(on_slab ? SL_THREADS : STACK8_THREADS), (int64_t)((on_slab ? q.sl_blk : q.fs_blk) + q.extra_blk) * q.blk); };
        if (!slab && want_step && step_form >= 0 && red(true) >= 0) slab = true;
        const int red_off = want_step ? red(slab) : -1;
        if (red_off >= 0) {
            r.what = STEP; r.red_off = red_off;
            if (q.use_spec && q.B > 0 && slab) form = spec_form(PLAN_BF16, 0, 1, nt, full);
        } else if (spec) {      // the forward alone (evaluation / two-call training) on its program
            form = spec_form(PLAN_BF16, 1, training, nt, full);
            if (form >= 0) slab = true;
        }
    }
    if (form >= 0) slab = true;
    r.slab_prog = slab;
    if (!slab) { r.family = STACK8; r.k = r.what; r.lds = (q.fs_blk + q.extra_blk) * q.blk; return r; }
    r.threads = SL_THREADS; r.lds = (q.sl_blk + q.extra_blk) * q.blk;
    r.NM = slab_nm(q.n_mlp); r.HB = slab_hb(q.sl_hb);
    if (form < 0) { r.family = SLAB; r.k = slab_row(r.what, r.NM, r.HB); return r; }
    r.family = SLAB_SPEC; r.k = form;
    r.FULL = full; r.NT = nt; r.TR = training || bwd;
    return r;
}

// ---- the encoder launch: where its rows come from.  ALIGNED / ELEMENTWISE: the caller's plan-dtype rows; WIDE4 / WIDE8: the caller's fp32 / fp64 rows, converted by the
// encoder (plan-dtype rows written to x on the side where x is given); SERIES*: gathered from a sequence's resident series -- raw or standardised (_STD: the series carries
// statistics), plain, with the signs of one group element (SIGNED: a nonzero sign word) or with a group element per window (ORBIT: K > 1 in the sign word).
enum EncForm : int { ELEMENTWISE, ALIGNED, WIDE4, WIDE8, SERIES, SERIES_STD, SERIES_SIGNED, SERIES_SIGNED_STD, SERIES_ORBIT, SERIES_ORBIT_STD, ENC_FORMS };
constexpr const char* ENC_FORM_NAMES[ENC_FORMS] = {"ELEMENTWISE", "ALIGNED", "WIDE4", "WIDE8", "SERIES", "SERIES_STD", "SERIES_SIGNED", "SERIES_SIGNED_STD", "SERIES_ORBIT", "SERIES_ORBIT_STD"};
constexpr bool enc_form_series(int form) { return form >= SERIES; }
constexpr bool enc_form_wide(int form) { return form == WIDE4 || form == WIDE8; }
struct EncFacts {
    bool series = false, stats = false;      // a series source; ... with statistics (standardised windows)
    int sign = 0;                            // its sign word
    int label_rows = 0;                      // ... and the rows of its label gather
    int wide_bytes = 0;                      // a wide source's element size (0: none)
    bool x_given = false, aligned = false;   // window rows to write / read; 16-byte aligned rows and pitches
    bool src_routes = false, wide_needs_rows = false;      // LaunchTraits: the plan's encoder has series / wide routes; wide sources need aligned plan-dtype rows
};
struct EncPick { int form; unsigned label_wgs; int err; };      // err: MSHGNN_OK, MSHGNN_EUNSUPPORTED (wide rows on a plan without source routes), MSHGNN_EINVAL (unaligned rows)
constexpr EncPick pick_enc(const EncFacts& f) {
    const int plain = f.aligned ? ALIGNED : ELEMENTWISE;
    if (!f.src_routes) return {plain, 0u, f.wide_bytes ? MSHGNN_EUNSUPPORTED : MSHGNN_OK};
    if (f.series) {      // x = the window buffers the rows are materialised into (may be null)
        if (f.x_given && !f.aligned) return {plain, 0u, MSHGNN_EINVAL};
        const int base = (f.sign >> MSHGNN_WINDOW_ELEMENTS_SHIFT) != 0 ? SERIES_ORBIT : f.sign ? SERIES_SIGNED : SERIES;
        return {base + (f.stats ? 1 : 0), (unsigned)((f.label_rows + 255) / 256), MSHGNN_OK};
    }
    if (f.wide_bytes) {
        if ((f.x_given || f.wide_needs_rows) && !f.aligned) return {plain, 0u, MSHGNN_EINVAL};
        return {f.wide_bytes == 8 ? WIDE8 : WIDE4, 0u, MSHGNN_OK};
    }
    return {plain, 0u, MSHGNN_OK};
}

}}  // namespace mshgnn::pick
