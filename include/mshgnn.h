/*
 * mshgnn.h -- C-ABI of the MI355X-native MS-HGNN message-passing engine (libmshgnn.so).
 *
 * The reference (lunarlab-gatech/MorphSym-HGNN) has no FFI layer: its hot path sits behind two Python
 * surfaces.  This header is the boundary a maintainer would bind instead of
 *   GRF_HGNN_C2.forward   src/ms_hgnn/lightning_py/hgnn_c2.py:133-182   (+ autograd backward of it)
 *   GRF_HGNN_K4.forward   src/ms_hgnn/lightning_py/hgnn_k4.py:146-196
 *   GRF_HGNN.forward      src/ms_hgnn/lightning_py/hgnn.py:57-62
 *   MSE loss of the Lightning wrapper  gnnLightning.py:633-639, 680-695
 * i.e. everything `torch_geometric.nn.{HeteroDictLinear, HeteroConv, GraphConv, Linear}` + ATen execute for
 * one minibatch of time-window graphs (hgnn_c2.py:3, :88, :100-113, :131).
 *
 * Conventions: plain pointers and sizes, no torch types; every function returns 0 on success or a negative
 * MSHGNN_E* code (never throws across the ABI); mshgnn_last_error() gives the text for the calling thread.
 * All device buffers are caller-allocated (e.g. by the torch caching allocator); no ownership transfer.
 * forward/backward are asynchronous on the caller's HIP stream (passed as void* = hipStream_t).  A plan is
 * immutable after creation, so forward/backward are re-entrant from autograd worker threads as long as each
 * call uses its own workspace.  A workspace carries the activation stash from a forward to its backward: use one
 * workspace per stream, with the device that owns it current (hipSetDevice) when the entry point is called -- two
 * forwards on one workspace overwrite each other's stash, whatever streams they run on.
 *
 * Engines: plan creation picks the LDS-resident kernels (hidden == 128, <= 20 nodes per window, in-degree 1 on 'mean' relations) where
 * they apply, else the generic-width engine (any hidden multiple of 128 up to 2048, any node count / in-degree; bf16 or split-bf16
 * arithmetic -- an MSHGNN_F32 request is served by the latter at the same tolerance).  mshgnn_info.kernel_sets bit 2 tells which.
 *
 * Data layout ("dense window-major"): every window graph of a minibatch has the same tiny topology, so the
 * PyG-batched [B*n_type, F] tensors the reference passes are already [B, n_type, F] contiguous; they are
 * consumed as-is.  dtype selects storage/operand precision of inputs and activations:
 *   MSHGNN_F32  : fp32 storage, exact-fp32 MFMA (v_mfma_f32_16x16x4_f32)           -- parity mode (1e-4 rel).  ONLY on the LDS-resident
 *                 kernels: a plan that falls to the generic-width engine (mshgnn_info.kernel_sets & 4: hidden != 128, > 20 nodes, mean
 *                 aggregation with in-degree > 1) has no fp32-MFMA variant and serves an MSHGNN_F32 request with the split-bf16 arithmetic of
 *                 MSHGNN_BF16X3 (inputs stay fp32; products x_hi w_hi + x_lo w_hi + x_hi w_lo with fp32 accumulation: measured <= 1.4e-5 of the
 *                 fp64 reference, tolerance 1e-4) -- NOT a bit-exact fp32 fma chain.
 *   MSHGNN_BF16 : bf16 storage + bf16 MFMA operands, fp32 accumulate, fp32 weights  -- throughput mode
 *   MSHGNN_BF16X3: fp32 inputs, hi/lo bf16 planes, three bf16 MFMA products per term -- parity mode at bf16-MFMA speed
 * Parameters and parameter gradients are always one flat fp32 buffer (offsets given in the descriptor).
 */
#ifndef MSHGNN_H
#define MSHGNN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSHGNN_MAX_TYPES 4
#define MSHGNN_F32 0
#define MSHGNN_BF16 1
#define MSHGNN_BF16X3 2   /* split-bf16 parity plan: fp32 inputs; every activation stored as two bf16 planes (hi + lo, 16 mantissa
                             bits); products on the bf16 MFMA as hi*hi + hi*lo + lo*hi, fp32 accumulate -- 1e-4 relative like
                             MSHGNN_F32 at a multiple of its speed.  LDS-resident for topologies with <= 20 nodes whose two planes fit a
                             CU's LDS: 2 x nodes <= 40 blocks (every A1 / Solo graph; MiniCheetah-K4's 20 nodes exactly, its four
                             base_transform scratch blocks aliasing node blocks) -- anything larger runs on the generic-width engine */

#define MSHGNN_OK 0
#define MSHGNN_EINVAL (-1)      /* bad descriptor / argument */
#define MSHGNN_EUNSUPPORTED (-2) /* valid request the engine cannot run (e.g. hidden not a multiple of 128) */
#define MSHGNN_EHIP (-3)        /* HIP runtime error */
#define MSHGNN_ENOMEM (-4)

#define MSHGNN_FLAG_RESIDUAL 1u      /* X <- f(H) + X            (hgnn_c2.py:161-166)                 */
#define MSHGNN_FLAG_BASE_MLP 2u      /* base_transform on mlp_type (hgnn_c2.py:117-121,156)           */

typedef struct mshgnn_plan mshgnn_plan;

/* One model instance over one robot topology.  Relation r is the reference's edge type
 * (src_type, rel, dst_type); its GraphConv has lin_rel (weight+bias) and lin_root (weight only).
 * All offsets are element offsets into the flat fp32 parameter buffer.                              */
typedef struct mshgnn_desc {
    int32_t n_types;                              /* node types, in data_metadata[0] order            */
    int32_t hidden;                               /* hidden_channels: a multiple of 128 (128: LDS-resident kernels; else generic-width engine) */
    int32_t num_layers;                           /* message-passing layers                           */
    int32_t n_rel;                                /* relations, in data_metadata[1] order             */
    int32_t out_type;                             /* node type the decoder reads ('foot')             */
    int32_t out_channels;                         /* out_channels_per_foot                            */
    int32_t mlp_type;                             /* type with the base_transform epilogue, or -1     */
    uint32_t flags;                               /* MSHGNN_FLAG_*                                    */
    int32_t dtype;                                /* MSHGNN_F32 | MSHGNN_BF16 | MSHGNN_BF16X3          */
    int32_t type_nodes[MSHGNN_MAX_TYPES];         /* nodes of each type per window                    */
    int32_t type_width[MSHGNN_MAX_TYPES];         /* input feature width F_type                       */
    const int32_t* rel_src;                       /* [n_rel] source type                              */
    const int32_t* rel_dst;                       /* [n_rel] destination type                         */
    const int32_t* rel_mean;                      /* [n_rel] 1 = 'mean' aggregation, 0 = 'add'        */
    const int32_t* rel_edge_off;                  /* [n_rel+1] prefix offsets into edges              */
    const int32_t* edges;                         /* [2*E] (src_node, dst_node) per-window pairs      */
    const float* in_mask[MSHGNN_MAX_TYPES];       /* [n_t*F_t] +-1 symmetry mask (apply_symmetry), host */
    const float* out_mask;                        /* [n_out*out_channels] +-1 (ms_foot_decoder), host */
    /* flat-parameter offsets */
    const int64_t* off_enc_w;                     /* [n_types]  encoder.lins.<t>.weight [h, F_t]      */
    const int64_t* off_enc_b;                     /* [n_types]                                        */
    const int64_t* off_rel_w;                     /* [L*n_rel]  convs.l.convs.<r>.lin_rel.weight      */
    const int64_t* off_rel_b;                     /* [L*n_rel]                 ...lin_rel.bias        */
    const int64_t* off_root_w;                    /* [L*n_rel]                 ...lin_root.weight     */
    int64_t off_mlp[4];                           /* base_transform.0.{w,b}, base_transform.2.{w,b}   */
    int64_t off_dec_w, off_dec_b;                 /* decoder.{weight,bias}                            */
    int64_t n_flat;                               /* length of the flat parameter buffer              */
} mshgnn_desc;

/* Work / traffic the plan executes per window (dead nodes of the last layers are skipped).           */
typedef struct mshgnn_info {
    int32_t rows_per_tile;        /* windows per workgroup tile of the layer kernels                   */
    int32_t total_nodes;          /* nodes per window                                                  */
    int64_t lds_bytes;            /* dynamic LDS of the layer kernels                                  */
    double flops_fwd;             /* algorithmic FLOPs / window, forward (2 FLOP per MAC)              */
    double flops_bwd;             /* algorithmic FLOPs / window, backward (dX chain + all dW)          */
    double flops_exec_fwd;        /* FLOPs / window the kernels actually issue (per-edge MACs, padding) */
    double flops_exec_bwd;
    double bytes_in;              /* input bytes / window at the plan dtype                            */
    int32_t n_gradw_workgroups;   /* split-K workgroups of the weight-gradient kernel                  */
    int32_t n_launches_fwd, n_launches_bwd;
    int32_t kernel_sets;          /* bit 0: fused stack kernels (bf16 plan), bit 1: slab stack kernels (two 4-wave workgroups per
                                     CU; used for batches of >= 1.5 tiles per CU), bit 2: generic-width engine -- what the plan allows  */
    int64_t grad_split;           /* two-phase step (mshgnn_step_mse_phase): gradients [grad_split, n_flat) are final after
                                     phase 0, [0, grad_split) (the encoder's) after phase 1; -1: the plan has no split       */
    double bytes_in_live;         /* input bytes / window of the nodes whose inputs can reach the output at this depth (<= bytes_in): what
                                     the plan reads.  A1-C2 at L = 3: the base nodes are four hops from the feet, their 3 600 B never matter */
} mshgnn_info;

/* Offsets (bytes) of the per-layer buffers inside the workspace, for tests / debugging.              */
typedef struct mshgnn_ws_layout {
    size_t total;
    size_t x[17];       /* X_l      [B][NN][h]  l = 0..L   (dtype)      hidden state after the encoder / layer l-1 */
    size_t dx[17];      /* dX_l     [B][NN][h]  l = 0..L   (dtype)                                                  */
    size_t dh[16];      /* dH_l     [B][NN][h]  l = 0..L-1 (dtype)      gradient w.r.t. the HeteroConv output       */
    size_t dd[16];      /* dd[0]: relu bytes of the encoder activation X_0 (layout as mask[l], training only); generic engine: dd[1] / dd[2] =
                           forward / backward sums of more than 32 rows into one node, L buffers of [aggregates][B][h] each (0: none); rest 0 */
    size_t mask[16];    /* relu bits, one byte per (node, window, 8 features): [NN][4][ceil(B/16)][4][16] uint8          */
    size_t hb[16], t1[16], du[16];  /* base_transform stash [B][n_mlp][h] (dtype)                                   */
    size_t wpack;       /* packed weights                                                                          */
    size_t bias;        /* packed biases (fp32)                                                                    */
    size_t dec_slabs;   /* decoder partial gradients (fp32)                                                                         */
    size_t slabs;       /* split-K partial weight gradients (fp32)                                                 */
    size_t loss;        /* 16 floats                                                                               */
} mshgnn_ws_layout;

/* Per-kernel timing (HIP events on the caller's stream) + the algorithmic work of each kernel of a step.   */
#define MSHGNN_BOUND_HBM 0
#define MSHGNN_BOUND_MFMA 1
typedef struct mshgnn_kernel_stat {
    char name[32];
    int32_t launches;             /* launches accumulated since the last read                          */
    int32_t bound;                /* MSHGNN_BOUND_* : the roofline that bounds this kernel             */
    float total_ms;               /* sum of event-measured durations                                   */
    float _pad;
    double flops_per_window;      /* algorithmic FLOPs / window / launch                                */
    double flops_exec_per_window; /* FLOPs the kernel issues / window / launch                          */
    double bytes_per_window;      /* algorithmic HBM bytes / window / launch                            */
} mshgnn_kernel_stat;

const char* mshgnn_last_error(void);
const char* mshgnn_version(void);
/* ABI guard for callers that keep their own copy of this header: MSHGNN_ABI_VERSION changes whenever a struct below changes size or meaning (5: mshgnn_info
 * gained bytes_in_live, kernel_sets bits 3 / 4 retired; 6: mshgnn_window_desc gained run_ptrs_ready), and the sizes the LIBRARY was built with can be compared with the caller's sizeof() before any
 * struct crosses the boundary -- mshgnn_plan_info / mshgnn_workspace_layout write sizeof(struct) bytes through the pointer they are given.                */
#define MSHGNN_ABI_VERSION 6
int mshgnn_abi_version(void);
size_t mshgnn_struct_size(int which);      /* 0: mshgnn_desc, 1: mshgnn_info, 2: mshgnn_ws_layout, 3: mshgnn_window_desc, 4: mshgnn_kernel_stat; else 0 */

int mshgnn_plan_create(const mshgnn_desc* desc, mshgnn_plan** plan_out);
void mshgnn_plan_destroy(mshgnn_plan* plan);
int mshgnn_plan_info(const mshgnn_plan* plan, mshgnn_info* info);
/* Name of the compile-time program ("A1C2_L3", ...) this plan's stack launches run on -- the one-call training steps, the forward alone (evaluation) and the two-call training
 * route; at every batch size (batches that are not whole 16-window tiles: predicated forms of the step and of the evaluation forward) -- or "" when the plan's tables are
 * interpreted at run time.  The kernels are specialised at build time for the topologies BASELINE.json names and the model types the reference's scripts default to
 * (csrc/mshgnn_spec_tables.inc, generated from this library's own plan compiler); a plan takes one only when its tables equal the kernel's, and MSHGNN_SPEC=0 at plan creation
 * keeps the interpreting kernels (same bits either way: tests/test_spec_gpu.py).  Nothing in the reference corresponds: its forward is interpreted by PyTorch
 * (hgnn_c2.py:150-166). */
const char* mshgnn_plan_specialised(const mshgnn_plan* plan);
/* Attach a program compiled for THIS plan after the library was built: `selector` is the `mshgnn_jit_program` symbol of a small shared library made from the library's own
 * kernel source over the plan's own tables (csrc/mshgnn.hip as -DMSHGNN_SPEC_SHARD=99; morphsym_hgnn_amd/jit.py renders the tables, compiles with hipcc and caches the result).
 * For topologies the build has no program for (any URDF through the topology compiler): their stack launches then run straight-line code like the BASELINE topologies' instead of
 * the interpreting kernels -- same MACs, same order, same bits.  LDS-resident bf16 and split-bf16 plans (the latter: `mshgnn_jit_program_x3` of csrc/mshgnn_x3.hip); the tables are compared with the plan's, a mismatch is MSHGNN_EINVAL and changes
 * nothing.  The caller keeps that shared library loaded for the plan's lifetime.  Nothing in the reference corresponds (its forward is interpreted by PyTorch). */
int mshgnn_plan_attach_program(mshgnn_plan* plan, void* selector);
/* The plan compiler alone, on the host: no HIP device is touched, nothing is allocated.  Fills `info` (work counts, LDS bytes, kernel sets: what
 * mshgnn_plan_info would report for a plan of this descriptor) and the number of 32-bit table entries the plan would upload; returns the same error
 * codes / mshgnn_last_error() text as mshgnn_plan_create for a descriptor no engine takes.  Used by the CPU test-suite and by callers that size a
 * deployment before a GPU is attached (replaces nothing in the reference: its models have no compile step, hgnn_c2.py:10-131).  */
int mshgnn_plan_compile_host(const mshgnn_desc* desc, mshgnn_info* info, int32_t* n_tables_out);

/* Profiling: while enabled, forward/backward bracket every kernel with HIP events on the stream (not
 * graph-capturable, not thread-safe).  mshgnn_profile_read synchronises the recorded events, fills up to
 * *n_inout stats (one per kernel of a step, in launch order), sets *n_inout and resets the accumulators.   */
int mshgnn_profile_enable(mshgnn_plan* plan, int on);
int mshgnn_profile_read(mshgnn_plan* plan, mshgnn_kernel_stat* stats, int32_t* n_inout);

/* Workspace for `batch` windows.  training=0: forward-only (no stash beyond what forward needs).    */
int mshgnn_workspace_layout(const mshgnn_plan* plan, int64_t batch, int training, mshgnn_ws_layout* out);

/* Forward.  x[t]: device pointer [batch][n_t][x_pitch[t]] at the plan dtype (x_pitch[t] >= F_t elements;
 * NULL pitch array = dense).  params: device fp32 flat buffer.  out: device fp32 [batch][n_out][out_channels]
 * (== the reference's [B*4, out] and, for C2 3-D GRF, its [B, 12] view; output mask applied).           */
int mshgnn_forward(const mshgnn_plan* plan, const void* const* x, const int64_t* x_pitch, const float* params,
                   float* out, void* workspace, int64_t batch, int training, void* stream);

/* Backward of the forward that last ran on `workspace` with the same x/params.  grad_out: device fp32
 * [batch][n_out][out_channels] (dL/d out).  grad_params: device fp32 flat buffer, fully OVERWRITTEN with
 * dL/d params (parameters that cannot influence the output get exact zeros).
 * grad_params == NULL (here and on mshgnn_backward_mse / _ce): activation backward only -- the backward sweep runs and leaves the encoder's
 * dY in the workspace for mshgnn_input_grad, the weight-gradient and finalize launches are skipped (frozen parameters; _mse / _ce still write
 * loss_out).                                                                                            */
int mshgnn_backward(const mshgnn_plan* plan, const void* const* x, const int64_t* x_pitch, const float* params,
                    const float* grad_out, float* grad_params, void* workspace, int64_t batch, void* stream);

/* Backward with the wrapper's MSE fused in (one launch less, no grad_out round trip): `out` is the forward's output,
 * y the labels in the same [batch][n_out][out_channels] order; loss_out (device float[1]) receives mean((out-y)^2). */
int mshgnn_backward_mse(const mshgnn_plan* plan, const void* const* x, const int64_t* x_pitch, const float* params,
                        const float* out, const float* y, float* loss_out, float* grad_params, void* workspace,
                        int64_t batch, void* stream);

/* One whole training step of the regression wrappers: forward + MSE + backward, == mshgnn_forward(training=1) followed by
 * mshgnn_backward_mse, same results up to fp32 summation order.  On the bf16 plan the decoder, the loss and the decoder
 * backward all run inside the fused forward kernel (one launch less, no X_L / dX_L round trip); other plans run the
 * two-call sequence.  out receives the forward output, loss_out mean((out - y)^2), grad_params every gradient.
 * Batches of at least twice MSHGNN_STEP_CHUNK windows (read at plan creation, default 32768, 0 = never; mshgnn_step_ce alike; not the generic-width engine, not the
 * _src / _series forms) run as equal sub-steps of at least that many windows over contiguous window ranges on the front of the same workspace: same out, loss and gradient up to fp32
 * summation order (sub-step sums are added in order: still deterministic); afterwards the workspace holds the stashes of the LAST sub-step only.             */
int mshgnn_step_mse(const mshgnn_plan* plan, const void* const* x, const int64_t* x_pitch, const float* params, const float* y,
                    float* out, float* loss_out, float* grad_params, void* workspace, int64_t batch, void* stream);

/* One whole training_step of the classification wrappers (forward + CrossEntropyLoss over the per-foot logit pairs + loss.backward(),
 * gnnLightning.py:640-648, 680-722) in one call: on the bf16 plan the decoder, the cross entropy and the decoder backward run in the tail of the
 * fused forward kernel (== mshgnn_forward followed by mshgnn_backward_ce, which the other plans run).  labels: device int32 [batch][n_out] in {0, 1}. */
int mshgnn_step_ce(const mshgnn_plan* plan, const void* const* x, const int64_t* x_pitch, const float* params, const int32_t* labels,
                   float* out, float* loss_out, float* grad_params, void* workspace, int64_t batch, void* stream);

/* The same step in two calls, for overlapping the gradient all-reduce with compute on several GPUs: phase 0 runs the forward,
 * the loss, the backward sweep and every weight gradient except the encoder's -- grad_params[grad_split, n_flat) and
 * loss_out are final when it completes; phase 1 finishes the encoder's gradients, grad_params[0, grad_split).  A caller
 * launches the all-reduce of the first region between the two calls (bench.py, N > 1).  Results are bit-identical to
 * mshgnn_step_mse.  Plans without a split (mshgnn_info.grad_split < 0) return an error.                                   */
int mshgnn_step_mse_phase(const mshgnn_plan* plan, const void* const* x, const int64_t* x_pitch, const float* params,
                          const float* y, float* out, float* loss_out, float* grad_params, void* workspace, int64_t batch,
                          int phase, void* stream);

/* The regression loss of a plan: MSE (the default of a fresh plan), L1 or Huber -- torch.nn.MSELoss / L1Loss / HuberLoss(delta), mean reduction (the reference trains
 * on MSE alone and has its L1 metric commented out, gnnLightning_com.py:66,77,103).  Per output element, d = out - y in fp32, inv_n the fp32 reciprocal of the element
 * count of the WHOLE batch (chunked steps included), mask the plan's output mask:
 *   MSE   (0): term = d d,                                                      g = 2 d inv_n mask
 *   L1    (1): term = |d|,                                                      g = (d > 0 ? inv_n : d < 0 ? -inv_n : d inv_n) mask   (0 at d == 0; NaN for a NaN d)
 *   Huber (2): term = |d| <= delta ? 0.5 d d : delta (|d| - 0.5 delta),         g = (d < -delta ? -delta : d > delta ? delta : d) inv_n mask
 * loss = (sum of terms) inv_n, summed in the fixed order of the MSE path.
 * EVERY ENTRY POINT WITH `mse` IN ITS NAME -- mshgnn_step_mse, _step_mse_src, _step_mse_phase (both phases), _backward_mse, _step_mse_series, _step_mse_series_std -- AND
 * mshgnn_mlp_step(loss_kind 0) COMPUTES THE PLAN'S REGRESSION LOSS: with the default these are the MSE instructions on the MSE operands, unchanged.  THE SETTING IS READ
 * WHEN THE CALL IS MADE AND PASSED BY VALUE in the kernel arguments: a captured graph keeps the kind and delta it was captured with, whatever the plan is set to later.
 * delta is read for Huber only (finite and > 0) and ignored otherwise.  MSHGNN_EINVAL, with the function's name in mshgnn_last_error(): a null plan / pointer, an
 * unknown kind, a Huber delta that is not finite and > 0.  A plan carries no task: the cross-entropy entry points never read the setting (the Python models refuse
 * it on a classification model).  The setters are not thread-safe against calls in flight on the same plan.                                                          */
#define MSHGNN_REG_LOSS_MSE 0
#define MSHGNN_REG_LOSS_L1 1
#define MSHGNN_REG_LOSS_HUBER 2
int mshgnn_plan_set_regression_loss(mshgnn_plan* plan, int kind, float delta);
int mshgnn_plan_get_regression_loss(const mshgnn_plan* plan, int32_t* kind_out, float* delta_out);
/* (mshgnn_mlp_set_regression_loss / _get_regression_loss, the same pair for an MLP plan: with the MLP entry points below) */
/* The same losses stand-alone, for the two-call routes: loss_out (device float[1]) = (sum of terms) / n and grad_out (nullable) [n] = g as above without a mask, in ONE
 * launch for all three kinds.  No floating-point atomic and nothing to clear: every workgroup leaves its partial sum in `scratch`, the one that finishes last adds them
 * in index order -- two runs give the same bits.  scratch: mshgnn_regression_loss_scratch_bytes(n) bytes (<= 1040) of device memory, 16-byte aligned, zeroed ONCE by
 * the caller (every call leaves it ready for the next one on the same stream).  Kind 0 evaluates the expressions of mshgnn_mse_loss, which stays as it is.            */
size_t mshgnn_regression_loss_scratch_bytes(int64_t n);
int mshgnn_regression_loss(const float* out, const float* y, int64_t n, int kind, float delta, float* loss_out, float* grad_out, void* scratch, void* stream);

/* Backward with the classification wrapper's cross entropy fused in (gnnLightning.py:640-648: CrossEntropyLoss over the
 * batch*4 per-foot logit pairs, mean).  `out` = the forward's logits [batch][n_out][2], labels int32 [batch][n_out] in
 * {0,1}; loss_out (device float[1]) receives the mean cross entropy.  Only for plans with out_channels == 2.            */
int mshgnn_backward_ce(const mshgnn_plan* plan, const void* const* x, const int64_t* x_pitch, const float* params,
                       const float* out, const int32_t* labels, float* loss_out, float* grad_params, void* workspace,
                       int64_t batch, void* stream);

/* Gradients with respect to the INPUTS (torch.autograd on the reference's x_dict leaves, hgnn_c2.py:150-151 + apply_symmetry): after a training
 * forward and mshgnn_backward / _mse / _ce (grad_params may be NULL) on the same workspace and batch,
 *   dx[t][w n_t + i][f] = in_mask[t][i][f] . sum_j dY_enc[w, node i of type t][j] W_enc[t][j][f]
 * for every type with dx[t] != NULL (NULL: skipped), written at dx_pitch[t] elements per row (NULL pitch array = dense F_t) as fp32 (dx_bytes 4) or fp64
 * (dx_bytes 8; any other value: MSHGNN_EUNSUPPORTED).  Rows of nodes the plan does not compute (they cannot reach the output at this depth) and pad
 * columns [F_t, pitch) are exact zeros.  One launch; arithmetic per plan (fp32 MFMA / bf16 operands / split-bf16 hi-lo products, fp32 accumulation),
 * every element one K sum in one workgroup: deterministic.  params: the flat fp32 buffer of that forward.                               */
int mshgnn_input_grad(const mshgnn_plan* plan, const float* params, void* const* dx, const int64_t* dx_pitch, int dx_bytes, const void* workspace,
                      int64_t batch, void* stream);

/* Adam on the flat fp32 buffers (configure_optimizers, gnnLightning.py:258-265; torch.optim.Adam defaults, no weight
 * decay / amsgrad).  step is 1-based; grads are multiplied by grad_scale first (1/world_size after a sum all-reduce).
 * All four buffers: device fp32, n elements, 16-byte aligned; params and both moments are updated in place, grads is
 * only read.  The bias corrections 1 - beta^step are formed in double from the fp32 betas and rounded to fp32 once. */
int mshgnn_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, int64_t step,
                     float lr, float beta1, float beta2, float eps, float grad_scale, void* stream);
/* The same update with the step count kept on the DEVICE: *step_count = steps taken so far (int64, device memory); the launch uses t = *step_count + 1 for
 * the bias corrections (formed in fp64 on the device) and stores t behind the update.  Nothing that changes from step to step is a launch argument, so a training step (forward, loss,
 * backward, this) can be captured once in a HIP graph and replayed -- what torch.optim.Adam(capturable=True) does for the reference's optimizer
 * (gnnLightning.py:258-265).  morphsym_hgnn_amd.optim.FlatAdam(graph_safe=True), wrappers.GraphedTrainingStep.                                          */
int mshgnn_adam_step_counted(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, int64_t* step_count,
                             float lr, float beta1, float beta2, float eps, float grad_scale, void* stream);

/* SGD on the flat fp32 buffers (configure_optimizers with optimizer = "sgd", gnnLightning.py:258-265): torch.optim.SGD, maximize = False.
 *   d = g grad_scale (+ weight_decay p when weight_decay != 0);
 *   momentum != 0:  buf = d on the first step, momentum buf + (1 - dampening) d on later ones;  d = nesterov ? d + momentum buf : buf;
 *   p -= lr d.
 * The first step is step == 1, or *step_count == 0 when step_count (device int64[1], 8-byte aligned) is given: then `step` is not read, the sweep reads the
 * count and a one-thread launch behind it adds 1.  lr_dev (device float[1]) given: it is read INSTEAD of lr, once at the head of the sweep -- with both on
 * the device nothing that changes from step to step is a launch argument, and a captured step follows a learning-rate schedule.  momentum_buf: NULL exactly
 * when momentum == 0; on the first step it is only written.  params, grads, momentum_buf: device fp32, n elements, 16-byte aligned; grads is only read.
 * MSHGNN_EINVAL (nothing launched): a null / misaligned buffer, n < 1, step < 1 without step_count, negative or NaN lr / momentum / weight_decay, nesterov
 * with momentum <= 0 or dampening != 0 (torch's constructor refuses the same).  morphsym_hgnn_amd.optim.FlatSGD.                                           */
int mshgnn_sgd_step(float* params, const float* grads, float* momentum_buf, int64_t n, int64_t step, int64_t* step_count, float lr, const float* lr_dev,
                    float momentum, float dampening, float weight_decay, int nesterov, float grad_scale, void* stream);
/* Adam with weight decay on the flat buffers, step count and learning rate on the host or on the device as for mshgnn_sgd_step.
 *   decoupled == 0: torch.optim.Adam(weight_decay): g' = g grad_scale + weight_decay p enters both moments;
 *   decoupled != 0: torch.optim.AdamW: p *= 1 - lr weight_decay first, then the Adam update from g grad_scale.
 * Bias corrections as the two entry points above form them (fp64, rounded to fp32 once; on the host from `step`, on the device from *step_count).  With
 * weight_decay == 0 the result is bit for bit mshgnn_adam_step's (host step) / mshgnn_adam_step_counted's (device step), with lr_dev or without.
 * morphsym_hgnn_amd.optim.FlatAdam(weight_decay) / FlatAdamW.                                                                                                */
int mshgnn_adamw_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, int64_t step, int64_t* step_count, float lr,
                      const float* lr_dev, float beta1, float beta2, float eps, float weight_decay, int decoupled, float grad_scale, void* stream);

/* Gradient clipping on the flat gradient buffer (torch.nn.utils.clip_grad_norm_, norm_type = 2), two launches, both capturable.
 * mshgnn_grad_norm: *norm_out (device double[1]) = sqrt(sum g_i^2), accumulated in fp64 (an fp32 square is exact there).  Bit-reproducible, no floating-point
 * atomic: the grid is min(ceil(ceil(n / 4) / 256), 256) workgroups of 256 threads -- a function of n alone -- every lane adds its grid-stride quads in
 * ascending order, waves reduce in a fixed butterfly, the workgroup that finishes last adds the workgroups' partial sums in index order.  scratch:
 * mshgnn_grad_norm_scratch_bytes(n) bytes (<= 2064) of device memory, 16-byte aligned, zeroed ONCE by the caller (every call leaves it ready for the next
 * one on the same stream).  grads: 16-byte aligned, only read; n >= 1.
 * mshgnn_grad_clip: g *= c for every element, c = min(1, max_norm / (*norm + 1e-6)) formed in fp64 and rounded to fp32 once; c == 1 leaves every bit as it
 * was (the sign of a zero included).  max_norm >= 0.                                                                                                             */
size_t mshgnn_grad_norm_scratch_bytes(int64_t n);
int mshgnn_grad_norm(const float* grads, int64_t n, double* norm_out, void* scratch, void* stream);
int mshgnn_grad_clip(float* grads, int64_t n, const double* norm, float max_norm, void* stream);

/* Loss of the Lightning wrapper (gnnLightning.py:633-639): loss = mean((out - y)^2) over n elements and
 * grad_out = 2 (out - y) / n (NULL: loss only).  loss_out: device float[1], cleared by the call.        */
int mshgnn_mse_loss(const float* out, const float* y, int64_t n, float* loss_out, float* grad_out, void* stream);

/* Loss of the classification wrappers (gnnLightning.py:640-648, customMetrics.py:6-25): mean cross entropy over `rows` per-foot logit
 * pairs (logits [rows][2], labels int32 [rows], nonzero = stable contact) and grad_out [rows][2] = (softmax - onehot) / rows
 * (NULL: loss only).  loss_out: device float[1].                                                                                  */
int mshgnn_ce_loss(const float* logits, const int32_t* labels, int64_t rows, float* loss_out, float* grad_out, void* stream);

/* ---- step metrics of the Lightning wrappers ------------------------------------------
 * The reference's torchmetrics states are plain sums across steps (gnnLightning.py:52-63, customMetrics.py:11-54); each
 * call ADDS one step's sums into caller-owned device state (zero it to start an epoch / to get step values).  Math in
 * fp64, a fixed reduction order (bit-reproducible).
 *
 * regression (calculate_losses_step, gnnLightning.py:124-130 / :633-639): state double[3]:
 *   [0] += sum (y_pred - y)^2   [1] += sum |y_pred - y|   [2] += n        => MSE = [0]/[2], RMSE = sqrt(MSE), L1 = [1]/[2]
 * MSHGNN_EINVAL before any launch (this call and every call below, down to mshgnn_metrics_com_step): a null pointer where none is allowed,
 * n / batch / n_bases < 1, a double / int64 state or a scratch that is not 8-byte aligned (the kernels run 64-bit atomics on them).         */
int mshgnn_metrics_regression(const float* y_pred, const float* y, int64_t n, double* state, void* stream);

/* classification (gnnLightning.py:132-151, 285-348): logits fp32 [batch*4][2] (per foot: no-contact, contact), labels int32
 * [batch][4] in {0,1} (read as `!= 0`: any nonzero label is a stable contact, as mshgnn_ce_loss reads it).  ce_state double[2]: [0] += sum of per-foot cross entropies, [1] += 4*batch.  counts int64[18]:
 *   [0] += batch, [1] += windows whose 16-class argmax (classification_conversion_16_class, :306-348) equals the label
 *   state 8 y0 + 4 y1 + 2 y2 + y3, [2 + 4k .. 5 + 4k] += tp, fp, fn, tn of leg k (BinaryF1Score, customMetrics.py:26-54). */
int mshgnn_metrics_classification(const float* logits, const int32_t* y, int64_t batch, double* ce_state, int64_t* counts,
                                  void* stream);

/* The same sums for one training / validation step in ONE multi-workgroup launch (what a wrapper's calculate_losses_step needs every step):
 * batch_* (nullable as a pair) receive this step's sums (overwritten -- no zeroing) followed by the step's published values, so that a
 * wrapper logs them without further launches: batch_state double[8] = sq, abs, n, MSE, RMSE, L1, 0, 0; batch_ce double[8] = ce sum, rows,
 * CE, 16-class accuracy, F1 of leg 0..3 (customMetrics.py:51-54, 0/0 -> 0); epoch_* (nullable as a pair; double[3] / double[2]) have the sums added, and grad_out (nullable) receives the gradient of the step's loss with respect to the predictions -- what
 * `training_step` returns for backward (gnnLightning.py:709-722): regression d MSE / d y_pred = 2 (y_pred - y) / n, fp32 [n];
 * classification d CE / d logits = (softmax - onehot) / (4 batch), fp32 [batch*4][2].  scratch: MSHGNN_METRICS_SCRATCH_BYTES of device
 * memory, 8-byte aligned, zeroed ONCE by the caller and then owned by these calls (per-workgroup partials + a ticket the kernel resets;
 * the partials are added in workgroup order: bit-reproducible); one scratch per stream.                                                  */
#define MSHGNN_METRICS_SCRATCH_BYTES 16384
int mshgnn_metrics_regression_step(const float* y_pred, const float* y, int64_t n, double* batch_state, double* epoch_state,
                                   float* grad_out, void* scratch, void* stream);
int mshgnn_metrics_classification_step(const float* logits, const int32_t* y, int64_t batch, double* batch_ce, int64_t* batch_counts,
                                       double* epoch_ce, int64_t* epoch_counts, float* grad_out, void* scratch, void* stream);

/* The extra sums of the centroidal-momentum wrappers (COM_Base_Lightning.calculate_losses_step, gnnLightning_com.py:96-121;
 * CosineSimilarityMetric, customMetrics.py:56-95): y_pred / y fp32 [batch][n_bases][6], each base node (lin(3) | ang(3)), standardised;
 * y_mean / y_std: HOST double[6] of the dataset's Standarizer (soloDataset.py:12-46).  state double[8] (batch_state overwritten,
 * epoch_state added into, either nullable):  [0] sum sq err of the lin halves  [1] of the ang halves  [2] = [3] 3 n_bases batch
 * [4] sum over windows of cos(lin_pred, lin) of base node 0 after un-standardising  [5] the same for ang  [6] batch  [7] 0.
 * MSE_lin = [0]/[2], MSE_ang = [1]/[3], cos_sim_lin = [4]/[6], cos_sim_ang = [5]/[6].  scratch: as for the two calls above.          */
int mshgnn_metrics_com_step(const float* y_pred, const float* y, int64_t batch, int n_bases, const double* y_mean, const double* y_std,
                            double* batch_state, double* epoch_state, void* scratch, void* stream);

/* The step sums per SEGMENT, for an evaluator's table of one row per symmetry operator and one column group per test sequence
 * (research/evaluator_regression-grf_c2.py:170-221, evaluator_classification_k4.py:57-89) out of ONE sweep: window b carries an id
 * segment[b] (DEVICE int32[batch]; an evaluation uses element * n_sequences + sequence) and its sums are added to row segment[b] of the state.
 * An id outside [0, n_segments), negative ids included, adds its window to the extra row n_segments (the overflow row): nothing is indexed
 * past the state, and there is no flag word and no host read.
 *   regression: y_pred / y fp32 [batch][per_window]; state double[n_segments + 1][3], row s: [0] += sum (y_pred - y)^2, [1] += sum |y_pred - y|,
 *     [2] += per_window * windows, over the windows of segment s (the sums of mshgnn_metrics_regression).
 *   classification: the layouts of mshgnn_metrics_classification; ce_state double[n_segments + 1][2], counts int64[n_segments + 1][18], row s
 *     what that call keeps, over the windows of segment s (16-class product rule, first maximum wins).
 * One launch, asynchronous on `stream`, nothing allocated.  All sums fp64 and bit-reproducible: the result is a function of the arguments alone,
 * for any arrangement of ids (sorted runs, shuffled, all equal, all distinct) and any arrival order of waves and workgroups.  No
 * floating-point atomic: a lane adds its window's terms in index order, a wave adds the lanes of one id in a fixed butterfly and leaves one
 * entry per distinct id in its slot of the scratch, and the workgroup that draws the last ticket adds every id's entries in (slot, entry)
 * order (csrc/mshgnn_train_ops.hip); the int64 counters are added with integer atomics, exact in any order.
 * scratch: mshgnn_metrics_segmented_scratch_bytes(batch) = 16 + 1544 * ceil(batch / 64) bytes of device memory (a ticket, then per 64
 * windows one slot of an entry count and 64 entries of id, windows and two sums), 8-byte aligned, zeroed ONCE by the caller and then owned by
 * these calls (the ticket is reset by the kernel); a scratch serves every batch up to the one it was sized for; one scratch per stream.
 * MSHGNN_EINVAL before any launch: a null pointer, batch < 1, per_window < 1, n_segments < 1, a scratch that is not 8-byte aligned.          */
size_t mshgnn_metrics_segmented_scratch_bytes(int64_t batch);
int mshgnn_metrics_regression_segmented(const float* y_pred, const float* y, int64_t batch, int32_t per_window, const int32_t* segment,
                                        int32_t n_segments, double* state, void* scratch, void* stream);
int mshgnn_metrics_classification_segmented(const float* logits, const int32_t* y, int64_t batch, const int32_t* segment, int32_t n_segments,
                                            double* ce_state, int64_t* counts, void* scratch, void* stream);

/* The centroidal-momentum sums per SEGMENT (the rows of research/evaluator_regression-com.py:50-76: Test Loss, Cos Sim Lin, Cos Sim Ang per
 * symmetry operator): y_pred / y / y_mean / y_std as mshgnn_metrics_com_step takes them, segment / n_segments / the overflow row n_segments as the
 * two segmented calls above define them.  state double[n_segments + 1][8], row s in the layout of mshgnn_metrics_com_step over the windows of
 * segment s: [0] += sq err of the lin halves, [1] += of the ang halves, [2] and [3] += 3 n_bases windows, [4] / [5] += the cosines of base node
 * 0's lin / ang vectors after un-standardising, [6] += windows, [7] untouched.  A window's terms are formed with the operations of
 * mshgnn_metrics_com_step in its order: the squared differences over (base, k) in index order, then each cosine as
 * sum (a / max(|a|, 1e-8)) (b / max(|b|, 1e-8)).  The discipline of the segmented calls: one launch, asynchronous, nothing allocated, fp64, no
 * floating-point atomic, bit-reproducible for any arrangement of ids and any arrival order (lane, wave butterfly per id, last workgroup merges
 * in (slot, entry) order).
 * scratch: mshgnn_metrics_com_segmented_scratch_bytes(batch) = 16 + 2568 * ceil(batch / 64) bytes (a ticket, then per 64 windows one slot of an
 * entry count and 64 entries of id, windows and FOUR sums), 8-byte aligned, zeroed once by the caller and then owned by this call; it serves
 * every batch up to the one it was sized for; one scratch per stream; not interchangeable with the scratch of the two calls above.
 * MSHGNN_EINVAL before any launch: a null pointer, batch < 1, n_bases < 1, n_segments < 1, a state or scratch that is not 8-byte aligned.     */
size_t mshgnn_metrics_com_segmented_scratch_bytes(int64_t batch);
int mshgnn_metrics_com_segmented(const float* y_pred, const float* y, int64_t batch, int n_bases, const double* y_mean, const double* y_std,
                                 const int32_t* segment, int32_t n_segments, double* state, void* scratch, void* stream);

/* body_frame_to_world_frame (gnnLightning.py:663-676) without the per-step CPU/scipy round trip: quat fp32 [batch][4] is
 * the world->body rotation, scalar-last (x, y, z, w) as scipy.Rotation.from_quat takes it; grf fp32 [batch][4][3].       */
int mshgnn_grf_body_to_world(const float* quat, const float* grf_body, float* grf_world, int64_t batch, void* stream);

/* ---- on-device window assembly ---------------------------------------------------------------
 * Replaces the per-window feature building of the dataset classes (quadSDKDataset_Morph.py:304-369, 444-488;
 * flexibleDataset.py:340-400, 563-596) + PyG collate: the sequence's raw series stay in HBM, fp32 COLUMN-major (element
 * (row, col) at src[col * src_cstride + row], so a window of one column is one contiguous stretch), and a batch of
 * windows [start, start + history) is gathered into the engine's inputs [batch][n_t][x_pitch[t]] (dtype).
 * runs (DEVICE int32[n_runs][5], sorted by (type, node)): {type, node, first feature, source << 8 | column (or -1: constant
 * 1), length <= 256}: features first .. first + length - 1 of that node row = src(start + k, column), k = 0 .. length - 1
 * (standardised over the window when normalize, as flexibleDataset.py:390-396).  rows (DEVICE int32[n_rows][2]): the run
 * range [begin, end) of every node row (one wave assembles one node row of one window).  Labels: y[b][k] = src[label_src][start + history - 1][label_cols[k]]
 * (label_cols: DEVICE int32[n_label]); label_rotate: 3-D world-frame GRFs -> body frame with the quaternion
 * src[quat_src] of that row (quadSDKDataset.py, load_data_at_dataset_seq_3d); quat_out (optional) receives it.         */
typedef struct mshgnn_window_desc {
    int32_t n_types, dtype, history, normalize;
    int32_t type_nodes[MSHGNN_MAX_TYPES], type_width[MSHGNN_MAX_TYPES];
    int32_t n_src, n_runs, n_rows;
    int32_t fast_layout;      /* != 0: the caller states that the runs of every node row all have one length and follow each other from FEATURE 0 on
                               * (first feature of the row's first run == 0; what a recipe of T-long variables gives): with 16-byte aligned output
                               * rows and no standardisation the gather then runs as one 16-byte store per output chunk (k_assemble_windows_fast),
                               * which also zeroes the pad columns up to the end of a row's last chunk.  The tables live on the device: the
                               * statement is not checked                                                                                      */
    const int32_t* runs;
    const int32_t* rows;
    int32_t n_label, label_src, label_rotate, quat_src;      /* quat_src = -1: none */
    const int32_t* label_cols;
    int32_t run_ptrs_ready;   /* mshgnn_step_*_series: != 0 = the caller states that the run_ptrs scratch still holds what an earlier call with THIS descriptor and
                               * THESE source arrays wrote there (the runs' column pointers depend on nothing else): the one-workgroup launch that resolves them
                               * in front of the encoder (4.8 us) is skipped.  0: resolve them (always safe).                                       */
    int32_t sign_flags;       /* group-transformed windows (the field was reserved: ABI 6 as before, a zero means what it meant).  bit 0: the caller states that
                               * `runs` source words and `label_cols` entries may carry MSHGNN_WINDOW_SIGN_FLAG (see below); with bit 0 clear the tables are read
                               * as they always were.  bit 1: the caller vouches that an earlier call with THIS descriptor (same tables) returned MSHGNN_OK, so
                               * the tables are not read back and checked again (the check is one small synchronous device-to-host copy: not capturable).
                               * bits 8..15: K, the number of group elements whose tables are stacked behind each other (ORBIT BATCHES below); 0 or 1: one table, as
                               * always.  K in [2, 8]; K > 1 implies bit 0. */
} mshgnn_window_desc;

/* SIGNED RUNS AND LABELS (sign_flags bit 0): g . window for an element g of a morphological symmetry group is a choice of columns and a +-1 per column, so it
 * is described by the same tables over the same resident series:
 *   runs[r][3]     = MSHGNN_WINDOW_SIGN_FLAG | source << 8 | column   (sources are < 12, columns < 256: bit 30 is free) -- the run's elements are negated
 *   label_cols[k]  = MSHGNN_WINDOW_SIGN_FLAG | column                 -- label k is negated (after the body-frame rotation; labels_out stays y != 0)
 * The negation is an XOR of the element's sign bit (0x80000000 on fp32, 0x8000 on bf16), never a multiply: exact, it commutes bit for bit with the bf16
 * rounding and -- up to the sign of a zero -- with the per-window standardisation, which is computed on the negated run.  Every gather applies it
 * (mshgnn_assemble_windows, mshgnn_forward_series, mshgnn_step_*_series[_std], x_out == NULL included), and the windows a training step writes to x_out are the
 * transformed ones.  quat_out is not transformed.  Refused with MSHGNN_EINVAL before any launch (unless bit 1 vouches): a negative source word other than -1
 * (the constant-1 run is the word -1 and cannot carry a sign), a source >= n_src, a label column whose column part is outside [0, 256) -- and a stream that
 * is being captured while the check is still due.                                                                                                        */
#define MSHGNN_WINDOW_SIGN_FLAG (1 << 30)

/* ORBIT BATCHES (sign_flags bits 8..15 = K > 1): every window of a batch carries its own group element.  The tables are stacked element-major over the same series,
 *   runs        int32[K][n_runs][5]      label_cols  int32[K][n_label]      run_ptrs scratch  K * n_runs * 8 bytes
 * and n_runs, rows, n_rows and mshgnn_forward_series_stats_bytes stay those of ONE element (a window has exactly one).  Window b's element rides in starts[b]:
 * bits 56..63 hold the element index, the low 56 bits the start row.  These bits are read only when the descriptor announces K > 1; with K <= 1 the high bits stay
 * unread, as always.  Every gather of window b takes its run word, run pointer and label column from block `element` of the tables; the statistics of a standardised
 * recipe are those of the window's own element's run.  quat_out is not transformed.
 * The checking call (bit 1 clear) refuses with MSHGNN_EINVAL before any launch, besides what it refuses in every element's sign tables: K > 8; an element table whose
 * {type, node, first feature, length} differs from element 0's in any run; a constant-1 run (source word -1) that is not constant-1 in every element.
 * An element index >= K in a device `starts` entry is clamped to K - 1 inside the kernels (one min): it never indexes past the tables.  Device-given starts stay
 * unchecked otherwise, rows as always.
 * Routes: mshgnn_assemble_windows, mshgnn_forward_series (standardised recipes included), mshgnn_step_mse_series / _ce_series with x_out given and the two _std steps.
 * x_out == NULL on the plain steps is refused with MSHGNN_EUNSUPPORTED for K > 1 (the weight-gradient kernel's own series gather has no per-window tables): materialise. */
#define MSHGNN_WINDOW_MAX_ELEMENTS 8
#define MSHGNN_WINDOW_ELEMENTS_SHIFT 8                                   /* sign_flags: K = (sign_flags >> 8) & 0xff */
#define MSHGNN_WINDOW_ELEMENTS_MASK 0xff
#define MSHGNN_START_ELEMENT_SHIFT 56                                    /* starts[b]: element = (uint64) starts[b] >> 56 */
#define MSHGNN_START_ROW_MASK ((((int64_t)1) << MSHGNN_START_ELEMENT_SHIFT) - 1)   /* starts[b]: row = starts[b] & MSHGNN_START_ROW_MASK */

int mshgnn_assemble_windows(const mshgnn_window_desc* desc, const float* const* src, const int64_t* src_cstride,
                            const int64_t* src_rows, const int64_t* starts /* device int64[batch] */, int64_t batch,
                            void* const* x_out, const int64_t* x_pitch, float* y_out, float* quat_out, void* stream);

/* Dataset indices -> window start rows, for a dataset of SEVERAL sequences whose series are concatenated row-wise into one set of source arrays (the
 * reference's ConcatDataset of per-sequence Subsets, research/train_regression-grf_msgn.py:57-73).  A view of the dataset takes the windows [lo_s, hi_s) of
 * sequence s, in sequence order: cum (DEVICE int64[n_seq + 1], cum[0] = 0, non-decreasing) holds the cumulative window counts, first_row (DEVICE
 * int64[n_seq]) the row of the concatenated series at which window lo_s of sequence s starts.  One thread per index i = index[b]: it finds s with
 * cum[s] <= i < cum[s + 1] (binary search over cum, staged in LDS for n_seq <= 1024, in global memory beyond) and writes
 * starts_out[b] = first_row[s] + (i - cum[s]); empty ranges are never selected.  An index outside [0, cum[n_seq]) writes start row 0 and stores 1 to
 * bad_out[0] (a plain store of the constant: every writer writes the same value).  bad_out is NOT cleared here -- the caller zeroes it and reads it
 * when it likes, so that the flag accumulates over an epoch.  With start row 0 a whole window of the first sequence, every row written is safe to hand
 * to the gathers above and below, which do not check `starts`.  MSHGNN_EINVAL before any launch: a null pointer, n_seq < 1, batch < 1 (cum and first_row
 * live on the device and are not looked at by the host).  One launch on `stream`, no allocation, no host read: capturable in a HIP graph.          */
int mshgnn_dataset_starts(const int64_t* cum, const int64_t* first_row, int32_t n_seq, const int64_t* index /* device int64[batch] */, int64_t batch,
                          int64_t* starts_out /* device int64[batch] */, int32_t* bad_out /* device int32[1] */, void* stream);

/* One training step straight from a sequence's resident raw series: mshgnn_assemble_windows + mshgnn_step_mse with the window gather FUSED INTO THE
 * ENCODER (no separate pass that writes and re-reads the batch's windows): the encoder kernel gathers its K chunks from bf16 copies of the series
 * (src_bf16: same shapes / column strides as src, every column followed by >= 8 elements of slack: src_cstride >= src_rows + 8), and writes the
 * materialised windows x_out (bf16, 16-byte aligned rows, pitch a multiple of 8) for the weight-gradient pass and for the caller; labels / quaternions come
 * from the fp32 series as in mshgnn_assemble_windows.  The descriptor must be a bf16, fast_layout, unstandardised recipe whose node types match the
 * plan's; bf16 plan with the fused stack kernels (else MSHGNN_EUNSUPPORTED: assemble, then mshgnn_step_mse).  run_ptrs: device scratch, 8 bytes per run.
 * x_out == NULL (x_pitch ignored): NO materialised windows -- the weight-gradient kernel gathers its raw-input operands from the series as well.
 * Results are bit-identical to mshgnn_assemble_windows followed by mshgnn_step_mse either way.
 * Split plan (MSHGNN_BF16X3): the encoder gathers from the fp32 series themselves (src; src_bf16 may be NULL; the same 8 elements of slack behind
 * every column), the descriptor's dtype is MSHGNN_F32 / MSHGNN_BF16X3, x_out (fp32, 16-byte aligned rows, pitch a multiple of 4) is required.     */
int mshgnn_step_mse_series(const mshgnn_plan* plan, const mshgnn_window_desc* desc, const float* const* src, const void* const* src_bf16,
                           const int64_t* src_cstride, const int64_t* src_rows, const int64_t* starts /* device int64[batch] */, int64_t batch,
                           void* const* x_out, const int64_t* x_pitch, float* y_out, float* quat_out, void* run_ptrs,
                           const float* params, float* out, float* loss_out, float* grad_params, void* workspace, void* stream);

/* The same for the classification wrappers (mshgnn_step_ce): labels_out (device int32 [batch][n_out]) receives the window labels != 0 (the
 * contact flags of the window's last step), y_out the float label rows.                                                                         */
int mshgnn_step_ce_series(const mshgnn_plan* plan, const mshgnn_window_desc* desc, const float* const* src, const void* const* src_bf16,
                          const int64_t* src_cstride, const int64_t* src_rows, const int64_t* starts, int64_t batch,
                          void* const* x_out, const int64_t* x_pitch, float* y_out, int32_t* labels_out, void* run_ptrs,
                          const float* params, float* out, float* loss_out, float* grad_params, void* workspace, void* stream);

/* The two steps above on a STANDARDISED recipe (desc->normalize != 0, history in [2, 256]): mshgnn_assemble_windows + mshgnn_step_mse / mshgnn_step_ce on the
 * standardised windows, bit for bit, in one call.  A pre-pass writes {mean, sd} of every (window, run) into `stats` (device scratch, 16-byte aligned,
 * mshgnn_forward_series_stats_bytes(desc, batch) bytes), the encoder standardises the FP32 series with the arithmetic of mshgnn_assemble_windows (one shared
 * device function) on BOTH plans -- src_bf16 may be NULL, run_ptrs are resolved for 4-byte elements -- and writes the standardised windows to x_out in the
 * plan's input dtype (bf16 plan: bf16 rows, pitch a multiple of 8; split plan: fp32 rows, pitch a multiple of 4; pad columns beyond the last 16-byte chunk
 * untouched).  The weight-gradient pass reads those windows and nothing else: x_out == NULL is MSHGNN_EUNSUPPORTED on either plan.  Refused before anything is
 * launched: an unstandardised descriptor (MSHGNN_EINVAL: use the plain entry points), stats NULL or misaligned, history < 2 (MSHGNN_EINVAL), history > 256,
 * history < 8 with node rows of several runs, the fp32 plan, the generic-width engine, the per-layer kernels (MSHGNN_EUNSUPPORTED), and whatever the plain
 * entry points refuse in the label description.  Every launch goes on `stream`.  run_ptrs / desc->run_ptrs_ready as in mshgnn_step_mse_series; a scratch
 * filled by mshgnn_forward_series on the same standardised descriptor and sources may be vouched for here and the other way round.                        */
int mshgnn_step_mse_series_std(const mshgnn_plan* plan, const mshgnn_window_desc* desc, const float* const* src, const void* const* src_bf16,
                               const int64_t* src_cstride, const int64_t* src_rows, const int64_t* starts /* device int64[batch] */, int64_t batch,
                               void* const* x_out, const int64_t* x_pitch, float* y_out, float* quat_out, void* run_ptrs, void* stats,
                               const float* params, float* out, float* loss_out, float* grad_params, void* workspace, void* stream);
int mshgnn_step_ce_series_std(const mshgnn_plan* plan, const mshgnn_window_desc* desc, const float* const* src, const void* const* src_bf16,
                              const int64_t* src_cstride, const int64_t* src_rows, const int64_t* starts, int64_t batch,
                              void* const* x_out, const int64_t* x_pitch, float* y_out, int32_t* labels_out, void* run_ptrs, void* stats,
                              const float* params, float* out, float* loss_out, float* grad_params, void* workspace, void* stream);

/* Evaluation straight from a sequence's resident raw series: mshgnn_assemble_windows + mshgnn_forward(training = 0) in one call, with the window gather fused
 * into the encoder and NO materialised windows at all -- results are bit-identical to that pair.  `workspace` is one laid out for training = 0; nothing is
 * stashed.  Same plans as mshgnn_step_*_series: the bf16 plan with the fused stack kernels (src_bf16 as there) and the split plan MSHGNN_BF16X3 (fp32 series,
 * src_bf16 may be NULL); the fp32 plan, the generic-width engine (MSHGNN_EUNSUPPORTED) and descriptors whose node types differ from the plan's (MSHGNN_EINVAL)
 * are refused.  The stack launch is the one mshgnn_forward(training = 0) runs, compile-time programs included.
 * By-products, each optional (NULL: not computed): y_out fp32 [batch][n_label], quat_out fp32 [batch][4], labels_out int32 [batch][n_label] (y != 0, the
 * classification wrappers' contact flags; needs y_out).  A sequence without labels passes NULL for all three; the descriptor's label fields are then not read.
 * STANDARDISED recipes (desc->normalize != 0, history in [2, 256]) are accepted here: every run with a source column is standardised over its window,
 * (x - mean) / sd with Bessel's correction in fp64, NaN -> 0, then rounded to fp32 (and to bf16 on the bf16 plan) exactly as mshgnn_assemble_windows does --
 * one shared device function computes both.  A pre-pass writes {mean, sd} of every (window, run) into `stats` (device scratch, 16-byte aligned,
 * mshgnn_forward_series_stats_bytes(desc, batch) = batch * n_runs * 16 bytes; 0 and `stats` ignored for unstandardised recipes); the encoder then reads the
 * FP32 series on both plans (src_bf16 may be NULL on the bf16 plan too).  The plain training entry points keep refusing standardised recipes (their _std forms take them).
 * run_ptrs / desc->run_ptrs_ready as in mshgnn_step_mse_series; the pointers are those of the series the encoder reads, so a scratch filled by a
 * mshgnn_step_*_series call with the same (unstandardised) descriptor and sources may be vouched for here and the other way round.                        */
int mshgnn_forward_series(const mshgnn_plan* plan, const mshgnn_window_desc* desc, const float* const* src, const void* const* src_bf16,
                          const int64_t* src_cstride, const int64_t* src_rows, const int64_t* starts /* device int64[batch] */, int64_t batch,
                          float* y_out /* nullable */, float* quat_out /* nullable */, int32_t* labels_out /* nullable */,
                          void* run_ptrs, void* stats /* standardised recipes only */, const float* params, float* out, void* workspace, void* stream);
int64_t mshgnn_forward_series_stats_bytes(const mshgnn_window_desc* desc, int64_t batch);

/* ---- stand-alone operators behind the four torch_geometric.nn names ----------------------------------
 * For a maintainer who swaps only the PyG import (hgnn_c2.py:3): Linear / HeteroDictLinear (hgnn_c2.py:88,131), GraphConv
 * (hgnn_c2.py:100-112) and their autograd backward on arbitrary graphs and widths, fp32 operands, fp32 MFMA, no float atomics.
 *
 * mshgnn_op_gemm: C[m ldc + n] (+)= sum_k A[m sAm + k sAk] B[n sBn + k sBk] (+ bias[n]) -- element strides, so the three products
 * of a Linear are one entry point: y = x W^T + b (A = x, B = W), dx = dy W (B = W with sBn = 1, sBk = in), dW = dy^T x (A = dy with
 * sAm = 1, sAk = out; B = x with sBn = 1, sBk = in: reduction over the rows, split-K with a fixed-order sum).
 * mshgnn_op_gemm_workspace: bytes of device workspace that shape needs (0: none).  accumulate != 0 adds into C.
 * K == 0 is an empty sum (C (+)= bias; A and B are not read and may be null); M == 0 or N == 0 writes nothing.                   */
int64_t mshgnn_op_gemm_workspace(int64_t M, int64_t N, int64_t K, int32_t* splits_out);
int mshgnn_op_gemm(const float* A, int64_t sAm, int64_t sAk, const float* B, int64_t sBn, int64_t sBk, const float* bias,
                   float* C, int64_t ldc, int64_t M, int64_t N, int64_t K, int accumulate, void* workspace, void* stream);

/* GraphConv's aggregation (PyG: propagate with aggr 'add' / 'mean', before lin_rel): out[r][:] = sum over the CSR row r of
 * edge_scale[e] x[col[e]][:] (edge_scale null: 1; 'mean': 1 / max(in-degree, 1) of the edge's destination).  The backward is the
 * same call on the CSR of the transposed graph.  rowptr: int32[n_rows + 1], col / edge_scale: [n_edges], all on the device.   */
int mshgnn_op_aggregate(const float* x, int64_t ldx, const int32_t* rowptr, const int32_t* col, const float* edge_scale,
                        float* out, int64_t ldo, int64_t n_rows, int64_t width, void* stream);

/* bias gradient: out[n] = sum_m X[m ldx + n], two fixed-order stages; workspace bytes from mshgnn_op_colsum_workspace.      */
int64_t mshgnn_op_colsum_workspace(int64_t M, int64_t N);
int mshgnn_op_colsum(const float* X, int64_t ldx, float* out, int64_t M, int64_t N, void* workspace, void* stream);

/* The same operators over `double` buffers (csrc/mshgnn_ops.hip), for a caller who keeps the reference's precision (torch.set_default_dtype(torch.float64),
 * gnnLightning.py:1183) on the device: ops.compute_dtype("f64"), model.set_precision("f64").  Contracts, argument meaning (element strides, accumulate, bias,
 * ldc, K == 0, M == 0 / N == 0) and every MSHGNN_EINVAL refusal are those of the fp32 entry points above; no value is narrowed to fp32 on the way.
 * mshgnn_op_gemm_f64: the inner product is v_mfma_f64_16x16x4_f64; the split-K rule is mshgnn_op_gemm_workspace's (the same split count for the same shape),
 * partials are doubles in ws[z][M][N] (mshgnn_op_gemm_f64_workspace bytes) and are added in ascending z, then bias, then C when accumulating.
 * mshgnn_op_aggregate_f64: edges in CSR order; edge_scale[e] * x and the add round separately.  mshgnn_op_colsum_f64: 512-row blocks, then the blocks in order. */
int64_t mshgnn_op_gemm_f64_workspace(int64_t M, int64_t N, int64_t K, int32_t* splits_out);
int mshgnn_op_gemm_f64(const double* A, int64_t sAm, int64_t sAk, const double* B, int64_t sBn, int64_t sBk, const double* bias,
                       double* C, int64_t ldc, int64_t M, int64_t N, int64_t K, int accumulate, void* workspace, void* stream);
int mshgnn_op_aggregate_f64(const double* x, int64_t ldx, const int32_t* rowptr, const int32_t* col, const double* edge_scale,
                            double* out, int64_t ldo, int64_t n_rows, int64_t width, void* stream);
int64_t mshgnn_op_colsum_f64_workspace(int64_t M, int64_t N);
int mshgnn_op_colsum_f64(const double* X, int64_t ldx, double* out, int64_t M, int64_t N, void* workspace, void* stream);

/* ---- the reference's own input tensors, uncast ---------------------------------------------------------------------------------------------------
 * The reference's datasets hand the model fp64 tensors at the dense pitch (torch.set_default_dtype(float64), gnnLightning.py:1183; x_dict[type] is
 * [B n_t, F_t]).  These three entry points are mshgnn_forward / mshgnn_step_mse / mshgnn_step_ce for such tensors: src[t] = device pointer to the caller's
 * rows, src_bytes = 8 (fp64) or 4 (fp32), src_pitch[t] in elements (NULL = dense).  The encoder converts in registers (fp64 -> fp32 -> bf16, round to nearest
 * even at each step: exactly the values torch's .to() produces, two roundings included) and WRITES the plan-dtype rows into x_rows[t] ([batch][n_t][x_pitch[t]], 16-byte aligned, pitch a
 * whole number of 16-byte chunks: what mshgnn_backward* and the weight-gradient pass of the step read) for the nodes the plan reads -- instead of a separate
 * cast + re-pitch pass over the batch (A1-C2, 8192 windows: 472 MB read + 118 MB written + 118 MB re-read).  bf16 and split-bf16 plans of the LDS-resident
 * kernels; MSHGNN_EUNSUPPORTED on the fp32 plan and the generic-width engine (cast there).  fp32 rows of an even width must start 8-byte aligned.      */
int mshgnn_forward_src(const mshgnn_plan* plan, int src_bytes, const void* const* src, const int64_t* src_pitch, void* const* x_rows,
                       const int64_t* x_pitch, const float* params, float* out, void* workspace, int64_t batch, int training, void* stream);
int mshgnn_step_mse_src(const mshgnn_plan* plan, int src_bytes, const void* const* src, const int64_t* src_pitch, void* const* x_rows,
                        const int64_t* x_pitch, const float* params, const float* y, float* out, float* loss_out, float* grad_params,
                        void* workspace, int64_t batch, void* stream);
int mshgnn_step_ce_src(const mshgnn_plan* plan, int src_bytes, const void* const* src, const int64_t* src_pitch, void* const* x_rows,
                       const int64_t* x_pitch, const float* params, const int32_t* labels, float* out, float* loss_out, float* grad_params,
                       void* workspace, int64_t batch, void* stream);

/* ---- data-parallel gradient exchange on the caller's stream (replaces the bucketed all-reduce of Lightning-DDP, ---------------------
 * gnnLightning.py:1396-1400) -- one process per GPU, replicated weights, windows sharded: the ONLY collective of a step is the mean of the flat fp32
 * gradient over the ranks.  RCCL is bound at run time (dlopen of `rccl_path`, else librccl.so as the process already has it / as the loader finds it):
 * no link-time dependency, single-GPU callers never load it.  mshgnn_comm_unique_id on rank 0 -> the 128 bytes travel to every rank by any means
 * (torch.distributed's store, MPI, a file) -> mshgnn_comm_create on every rank with its device current (collective: ncclCommInitRank).
 * mshgnn_comm_allreduce_mean enqueues ncclAllReduce(buf, buf, n, float32, avg) on `stream` and returns: stream-ordered behind the step that produced
 * buf, no host synchronisation, capturable in a HIP graph together with the step.  _sum: the same with ncclSum (callers that weight by window counts). */
typedef struct mshgnn_comm mshgnn_comm;
int mshgnn_comm_unique_id(const char* rccl_path, void* id_out_128_bytes);
int mshgnn_comm_create(const char* rccl_path, const void* id_128_bytes, int nranks, int rank, mshgnn_comm** comm_out);
void mshgnn_comm_destroy(mshgnn_comm* comm);
int mshgnn_comm_allreduce_mean(mshgnn_comm* comm, float* buf, int64_t n, void* stream);
int mshgnn_comm_allreduce_sum(mshgnn_comm* comm, float* buf, int64_t n, void* stream);

/* ---- MLP baselines (csrc/mshgnn_mlp.hip) -------------------------------------------------------------------------------------------------------------
 * The reference's MLP (gnnLightning.py:391-405: nn.Sequential of num_layers Linear layers with ReLU between them, in -> hidden -> ... -> hidden -> out) on the
 * bf16 arithmetic class of the HGNN engine's bf16 plan: inputs and weights are bf16 MFMA operands (weights rounded from the flat fp32 buffer), fp32 accumulation
 * and bias add, activations and activation gradients pass between layers as bf16, output / loss / parameter gradients fp32.  No floating-point atomic: every
 * sum has a fixed order, two runs give identical bits.
 * dtype MSHGNN_BF16X3 runs the same launches on the split-bf16 arithmetic class of the HGNN engine's parity plan (1e-4 of fp64): every operand of a product
 * travels as hi = bf16(v), lo = bf16(v - hi) (both roundings to nearest even) and a product is hi hi + lo hi + hi lo with fp32 accumulation.  The dense rows are
 * fp32 and are split while they are staged; every packed weight region of the workspace is a hi image followed by a lo image; every stash and activation
 * gradient is rows of [hi hidden | lo hidden] bf16 (dZ of the output layer: [hi 16 | lo 16]); the ReLU mask of the backward sweep is [hi > 0].  There is no
 * series form on this dtype.  The flat parameter buffer is torch's state_dict order of that nn.Sequential: 0.weight, 0.bias,
 * 2.weight, 2.bias, ..., each weight [out_f, in_f] row-major (mshgnn_mlp_info.off_w / off_b, Linear layer i = 0 .. num_layers - 1).
 * Supported: hidden 128 / 256 / 384 / 512, in_channels 1 .. 16384 (no alignment condition), out_channels 1 .. 16, num_layers 2 .. 16, dtype MSHGNN_BF16 or
 * MSHGNN_BF16X3 (not MSHGNN_F32);
 * anything else is MSHGNN_EUNSUPPORTED with the limit named in mshgnn_last_error().
 * A step is five launches at any depth: weight pack, input layer, stack (layers 2 .. L, the loss tail and the backward sweep down to dZ_1 in one workgroup
 * per 32-row tile, activations LDS-resident), weight gradients (partial sums over row slabs), fixed-order slab sum (+ the loss).  The series form adds the
 * one-workgroup run-pointer launch unless the caller vouches (run_ptrs_ready).  Every launch goes on `stream`; nothing is allocated, nothing read back.        */
#define MSHGNN_MLP_MAX_LAYERS 16
typedef struct mshgnn_mlp_plan mshgnn_mlp_plan;
typedef struct mshgnn_mlp_desc {
    int32_t in_channels, hidden, out_channels, num_layers, dtype;
} mshgnn_mlp_desc;
typedef struct mshgnn_mlp_info {
    int64_t n_flat;                               /* length of the flat parameter buffer                                           */
    int64_t off_w[MSHGNN_MLP_MAX_LAYERS];         /* Linear layer i: weight [out_f, in_f] at off_w[i], bias [out_f] at off_b[i]    */
    int64_t off_b[MSHGNN_MLP_MAX_LAYERS];
    int32_t rows_per_tile;                        /* windows per workgroup tile of the input-layer and stack launches             */
    int32_t n_launches_step;                      /* launches of one mshgnn_mlp_step on dense rows                                 */
    int64_t lds_bytes;                            /* dynamic LDS of the stack launch                                               */
    double flops_fwd, flops_bwd;                  /* algorithmic FLOPs / window (2 per MAC): forward; backward (dA chain + all dW)  */
} mshgnn_mlp_info;
/* Where a batch's rows come from.  Dense form: x != NULL, bf16 rows (MSHGNN_BF16X3: fp32 rows) [batch][pitch], 16-byte aligned, pitch a multiple of 8 and >= in_channels rounded up to 8;
 * columns at or beyond in_channels are ignored.  Series form (MSHGNN_BF16 only; MSHGNN_BF16X3: MSHGNN_EUNSUPPORTED, assemble and use the dense form): x == NULL and desc / src / src_bf16 / src_cstride / src_rows / starts / run_ptrs exactly as
 * mshgnn_step_mse_series takes them (desc->run_ptrs_ready vouches the same way); row b is the window of the one node row of the recipe at starts[b], gathered
 * per K chunk from the bf16 series -- no window row is written to memory, the weight-gradient launch gathers the same operand again.  The series form takes a
 * bf16, fast_layout, unstandardised, unsigned descriptor with n_types == 1, type_nodes[0] == 1, type_width[0] == in_channels and one group element; any other
 * descriptor is MSHGNN_EUNSUPPORTED (assemble, then use the dense form: same bits).  y_out / quat_out / labels_out (each nullable): the window labels
 * (fp32 [batch][n_label]), quaternions and contact flags (int32, y != 0) as mshgnn_step_*_series produce them.                                              */
typedef struct mshgnn_mlp_input {
    const void* x; int64_t pitch;
    const mshgnn_window_desc* desc;
    const float* const* src; const void* const* src_bf16; const int64_t* src_cstride; const int64_t* src_rows;
    const int64_t* starts;
    float* y_out; float* quat_out; int32_t* labels_out;
    void* run_ptrs;
} mshgnn_mlp_input;
/* mshgnn_struct_size: 5 = mshgnn_mlp_desc, 6 = mshgnn_mlp_info, 7 = mshgnn_mlp_input */

/* The descriptor check and the info alone, on the host: no device is touched.  loss_kind: -1 (none), 0 (MSE) or 1 (cross entropy: out_channels must be even). */
int mshgnn_mlp_compile_host(const mshgnn_mlp_desc* desc, int loss_kind, mshgnn_mlp_info* info);
int mshgnn_mlp_create(const mshgnn_mlp_desc* desc, mshgnn_mlp_plan** plan_out);
void mshgnn_mlp_destroy(mshgnn_mlp_plan* plan);
int mshgnn_mlp_info_get(const mshgnn_mlp_plan* plan, mshgnn_mlp_info* info);
/* Bytes of the caller-owned workspace for `batch` rows (16-byte aligned base).  training = 0: forward only.  0: bad arguments. */
size_t mshgnn_mlp_workspace_bytes(const mshgnn_mlp_plan* plan, int64_t batch, int training);
/* Byte offset inside a training workspace of the bf16 stash of relu(Z_layer) (layer = 1 .. num_layers - 1, [rows][hidden], MSHGNN_BF16X3: [rows][hi hidden |
 * lo hidden]; rows = batch rounded up to the tile; rows past the batch are zeros) -- for tests / debugging; 0: no such stash.                                                                                  */
size_t mshgnn_mlp_stash_offset(const mshgnn_mlp_plan* plan, int64_t batch, int layer);
/* out: fp32 [batch][out_channels].  training != 0 leaves the bf16 stashes mshgnn_mlp_backward reads. */
int mshgnn_mlp_forward(const mshgnn_mlp_plan* plan, const mshgnn_mlp_input* input, const float* params, float* out, void* workspace, int64_t batch,
                       int training, void* stream);
/* After a training forward on the same workspace, input and params: gout fp32 [batch][out_channels] = dL / d out; grad_params (flat fp32) is fully overwritten. */
int mshgnn_mlp_backward(const mshgnn_mlp_plan* plan, const mshgnn_mlp_input* input, const float* params, const float* gout, float* grad_params,
                        void* workspace, int64_t batch, void* stream);
/* forward + loss + backward in one call, bit for bit the three calls (the same kernels; the loss tail runs inside the stack launch).
 * loss_kind 0: loss = mean((out - y)^2), targets fp32 [batch][out_channels]; loss_kind 1: mean cross entropy over the batch * out_channels / 2 logit pairs,
 * targets int32 [batch][out_channels / 2] in {0, 1}.  Series input with targets == NULL: the targets are the window labels the call gathers (input->y_out,
 * and input->labels_out for loss_kind 1).  loss_out: device float[1].                                                                                      */
int mshgnn_mlp_step(const mshgnn_mlp_plan* plan, const mshgnn_mlp_input* input, int loss_kind, const void* targets, const float* params, float* out,
                    float* loss_out, float* grad_params, void* workspace, int64_t batch, void* stream);
/* What loss_kind 0 computes on this plan: mshgnn_plan_set_regression_loss / _get_regression_loss for an MLP plan (same kinds, same checks, a fresh plan is MSE; read
 * when mshgnn_mlp_step is called and passed by value). */
int mshgnn_mlp_set_regression_loss(mshgnn_mlp_plan* plan, int kind, float delta);
int mshgnn_mlp_get_regression_loss(const mshgnn_mlp_plan* plan, int32_t* kind_out, float* delta_out);

/* ---- symmetrisation over a group orbit (csrc/mshgnn_orbit.hip) -------------------------------------------------------------------------------------------
 * f_sym(x) = 1/|G| sum_g rho_out(g)^-1 f(rho_in(g) x) makes any model exactly equivariant; the reference has no such layer (its symmetric models are
 * equivariant by architecture, its other models are trained on the augmented ConcatDataset([ds, ds_gs, ...])).  An ORBIT-COMPLETE batch has K * windows rows in
 * element-major order -- row e * windows + w is element e of base window w, the order of ConcatDataset -- K = n_elements in [1, MSHGNN_WINDOW_MAX_ELEMENTS].
 * The OUTPUT ACTION of element e is a pair of HOST tables perm[e][k], sign[e][k] in {+1, -1} over n_units units (<= 64) of `width` consecutive floats
 * (1 .. 16), meaning what a recipe's label tables mean: y_e[k] = sign[e][k] y[perm[e][k]].  Element 0 must be the identity with +1.  With
 * out fp32 [K windows][n_units width] and pinv_e the inverse of perm[e]:
 *   mshgnn_orbit_average:           avg[w][j width + s] = (t_0 + t_1 + ... + t_{K-1}) * fl32(1 / K),  t_e = out[e windows + w][pinv_e[j] width + s] with its sign
 *                                   bit flipped when sign[e][pinv_e[j]] = -1: fp32 adds in element order starting from t_0, then the one multiply (K = 1
 *                                   reproduces out bit for bit).
 *   mshgnn_orbit_average_backward:  the exact transpose, grad_out[e windows + w][k width + s] = sign[e][k] (grad_avg[w][perm[e][k] width + s] * fl32(1 / K)).
 *   mshgnn_orbit_defect:            per element e the differences d = t_e - out[w][.] (fp32, t_e as above) over all windows; an fp64 state double[K][4] =
 *                                   {sum d^2, sum out_0^2, max |d|, count} is ADDED TO (max: maxed into) `state` -- a sweep accumulates, the caller zeroes;
 *                                   row 0 gets zeros for sum d^2 and max |d|.  One workgroup per element, every thread adds its elements in index order, then
 *                                   a fixed tree: bit-reproducible, no floating-point atomic.
 * One launch each on `stream`, nothing allocated, nothing read back: the call validates the tables and packs them into a by-value kernel argument (576 bytes),
 * so there are no device tables and a captured graph holds them.  One thread per output element, 16-byte stores where n_units width % 4 == 0 and both pointers
 * are 16-byte aligned (16-byte loads too where width % 4 == 0), element-wise otherwise -- the same bits; grid-stride loops with 64-bit indices: any `windows`.
 * MSHGNN_EINVAL with nothing launched: a null pointer, n_elements outside [1, 8], n_units outside [1, 64], width outside [1, 16], windows < 1, a row of
 * perm that is no permutation of [0, n_units), a sign other than +-1, element 0 not the identity with +1, windows * n_elements * 2^10 beyond the 64-bit element
 * index, a `state` that is not 8-byte aligned.
 * morphsym_hgnn_amd/symmetrise.py: OutputAction, orbit_average, EquivarianceDefect, Symmetrised.                                                              */
int mshgnn_orbit_average(const int32_t* perm, const int32_t* sign, int32_t n_elements, int32_t n_units, int32_t width, const float* out, int64_t windows,
                         float* avg, void* stream);
int mshgnn_orbit_average_backward(const int32_t* perm, const int32_t* sign, int32_t n_elements, int32_t n_units, int32_t width, const float* grad_avg,
                                  int64_t windows, float* grad_out, void* stream);
int mshgnn_orbit_defect(const int32_t* perm, const int32_t* sign, int32_t n_elements, int32_t n_units, int32_t width, const float* out, int64_t windows,
                        double* state, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MSHGNN_H */
