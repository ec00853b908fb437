// Plan-independent entry points of libmshgnn (include/mshgnn.h): what a training loop runs around the engine's step, kernels and entry points together --
// Adam on the flat parameter buffer, the stand-alone MSE / cross-entropy losses, the step metrics of the Lightning wrappers (whole-batch and segmented) and the GRF body -> world rotation.
// None of it reads a plan; it shares only the error string with the rest of the library.
#include "mshgnn_device.hpp"

// ------------------------------------------------------------------------------------------------------
// Adam on the flat fp32 buffers (configure_optimizers: optim.Adam(self.parameters(), lr), gnnLightning.py:258-265;
// torch defaults beta=(0.9, 0.999), eps=1e-8, no weight decay, no amsgrad).  SURVEY.md section 8(f) row 2.
// ------------------------------------------------------------------------------------------------------
// One element-wise sweep of the update, shared by both kernels: 16-byte accesses on whole quads, a scalar tail for the last n % 4 elements (the thread that
// owns the quad that straddles n).  bc1 = fl32(1 - beta1^t), bc2_sqrt = fl32(sqrt(1 - beta2^t)), both formed in fp64 and rounded once by the caller.
__device__ __forceinline__ void adam_sweep(float* p, const float* g, float* m, float* v, int64_t n, float lr, float b1, float b2, float eps,
                                           float bc1, float bc2_sqrt, float gscale) {
    for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += (int64_t)gridDim.x * blockDim.x * 4) {
        if (i + 4 <= n) {
            f32x4 pp = *reinterpret_cast<f32x4*>(p + i), gg = *reinterpret_cast<const f32x4*>(g + i) * gscale;
            f32x4 mm = *reinterpret_cast<f32x4*>(m + i), vv = *reinterpret_cast<f32x4*>(v + i);
            mm = b1 * mm + (1.f - b1) * gg;
            vv = b2 * vv + (1.f - b2) * gg * gg;
#pragma unroll
            for (int e = 0; e < 4; ++e) pp[e] -= lr / bc1 * mm[e] / (sqrtf(vv[e]) / bc2_sqrt + eps);
            *reinterpret_cast<f32x4*>(p + i) = pp; *reinterpret_cast<f32x4*>(m + i) = mm; *reinterpret_cast<f32x4*>(v + i) = vv;
        } else {
            for (int64_t k = i; k < n; ++k) {
                const float gg = g[k] * gscale;
                m[k] = b1 * m[k] + (1.f - b1) * gg; v[k] = b2 * v[k] + (1.f - b2) * gg * gg;
                p[k] -= lr / bc1 * m[k] / (sqrtf(v[k]) / bc2_sqrt + eps);
            }
        }
    }
}

__global__ void k_adam(float* p, const float* g, float* m, float* v, int64_t n, float lr, float b1, float b2, float eps,
                       float bc1, float bc2_sqrt, float gscale) {
    adam_sweep(p, g, m, v, n, lr, b1, b2, eps, bc1, bc2_sqrt, gscale);
}

// The bias corrections are formed in DOUBLE from the fp32 betas and rounded to fp32 once (as torch.optim.Adam forms them in Python floats): in fp32,
// 1 - powf(0.999f, t) cancels -- at t = 2 the difference keeps 17 of its 24 bits and the update is off by 58 units of 2^-24 of its own size.
extern "C" int mshgnn_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, int64_t step,
                                float lr, float beta1, float beta2, float eps, float grad_scale, void* stream) {
    if (!params || !grads || !exp_avg || !exp_avg_sq || n < 1 || step < 1) return set_err(MSHGNN_EINVAL, "bad argument to mshgnn_adam_step");
    if (((uintptr_t)params | (uintptr_t)grads | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) return set_err(MSHGNN_EINVAL, "adam buffers must be 16-byte aligned");
    const double bc1 = 1.0 - std::pow((double)beta1, (double)step), bc2 = 1.0 - std::pow((double)beta2, (double)step);
    const int blocks = (int)std::min<int64_t>((n / 4 + 255) / 256 + 1, 2048);
    hipLaunchKernelGGL(k_adam, dim3(blocks), dim3(256), 0, (hipStream_t)stream, params, grads, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps,
                       (float)bc1, (float)std::sqrt(bc2), grad_scale);
    HIPCHK(hipGetLastError());
    return MSHGNN_OK;
}

// The same update with the step count on the DEVICE (capturable in a HIP graph: nothing of the bias corrections is baked into the launch arguments).  The kernel
// reads t = *step_count + 1 and derives 1 - beta^t itself, in fp64; a one-thread launch behind it stores t.  FlatAdam(graph_safe=True), wrappers.GraphedTrainingStep.
// beta1^t and beta2^t by binary powering in one loop (at most 63 rounds of four fp64 products; relative error <= 2 t 2^-53, nothing against the one fp32
// rounding behind it).  One thread of the workgroup forms the two factors and hands them over through LDS: every wave doing it for itself costs the launch
// ~0.7 us of fp64 issue at 2048 workgroups.
__global__ void k_adam_counted(float* p, const float* g, float* m, float* v, int64_t n, const int64_t* step_count, float lr, float b1, float b2, float eps, float gscale) {
    __shared__ float s_bc[2];
    if (threadIdx.x == 0) {
        double a1 = (double)b1, a2 = (double)b2, r1 = 1.0, r2 = 1.0;
        for (int64_t t = *step_count + 1; t > 0; t >>= 1) {
            if (t & 1) { r1 *= a1; r2 *= a2; }
            a1 *= a1; a2 *= a2;
        }
        s_bc[0] = (float)(1.0 - r1); s_bc[1] = (float)sqrt(1.0 - r2);
    }
    __syncthreads();
    adam_sweep(p, g, m, v, n, lr, b1, b2, eps, s_bc[0], s_bc[1], gscale);
}
__global__ void k_step_count_inc(int64_t* step_count) { *step_count += 1; }

extern "C" int mshgnn_adam_step_counted(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, int64_t* step_count,
                                        float lr, float beta1, float beta2, float eps, float grad_scale, void* stream) {
    if (!params || !grads || !exp_avg || !exp_avg_sq || !step_count || n < 1) return set_err(MSHGNN_EINVAL, "bad argument to mshgnn_adam_step_counted");
    if (((uintptr_t)params | (uintptr_t)grads | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) return set_err(MSHGNN_EINVAL, "adam buffers must be 16-byte aligned");
    const int blocks = (int)std::min<int64_t>((n / 4 + 255) / 256 + 1, 2048);
    hipLaunchKernelGGL(k_adam_counted, dim3(blocks), dim3(256), 0, (hipStream_t)stream, params, grads, exp_avg, exp_avg_sq, n, step_count, lr, beta1, beta2, eps, grad_scale);
    hipLaunchKernelGGL(k_step_count_inc, dim3(1), dim3(1), 0, (hipStream_t)stream, step_count);
    HIPCHK(hipGetLastError());
    return MSHGNN_OK;
}

// ------------------------------------------------------------------------------------------------------
// SGD (torch.optim.SGD: momentum / dampening / nesterov / weight decay) and Adam with weight decay, coupled (torch.optim.Adam(weight_decay)) or decoupled
// (torch.optim.AdamW), on the same flat buffers with the same sweep: the reference's wrappers take optimizer = "adam" | "sgd" (gnnLightning.py:258-265).
// The step count and the learning rate may live on the device (step_count, lr_dev: both read at the head of the sweep, before any store), so that a
// captured step follows a scheduler and a loaded state.
// ------------------------------------------------------------------------------------------------------
constexpr int ADAM_PLAIN = 0, ADAM_COUPLED = 1, ADAM_DECOUPLED = 2;
constexpr int SGD_PLAIN = 0, SGD_MOMENTUM = 1, SGD_NESTEROV = 2;

// one element or one quad of torch.optim.SGD's update (T = float | f32x4); bb is read only on a later step (first: the buffer may hold anything)
template <bool WD, int MOM, class T> __device__ __forceinline__ void sgd_update(T& pp, T gg, T& bb, bool first, float lr, float mom, float keep, float wd, float gscale) {
    T d = gg * gscale;
    if (WD) d += wd * pp;
    if (MOM != SGD_PLAIN) {
        if (first) bb = d;
        else bb = mom * bb + keep * d;
        if (MOM == SGD_NESTEROV) d += mom * bb;
        else d = bb;
    }
    pp -= lr * d;
}

template <bool WD, int MOM> __global__ void k_sgd(float* p, const float* g, float* buf, int64_t n, const int64_t* step_count, int first, float lr,
                                                  const float* lr_dev, float mom, float damp, float wd, float gscale) {
    if (step_count) first = *step_count == 0;
    if (lr_dev) lr = *lr_dev;
    const float keep = 1.f - damp;
    for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += (int64_t)gridDim.x * blockDim.x * 4) {
        if (i + 4 <= n) {
            f32x4 pp = *reinterpret_cast<f32x4*>(p + i), bb = {0.f, 0.f, 0.f, 0.f};
            if (MOM != SGD_PLAIN && !first) bb = *reinterpret_cast<f32x4*>(buf + i);
            sgd_update<WD, MOM>(pp, *reinterpret_cast<const f32x4*>(g + i), bb, first, lr, mom, keep, wd, gscale);
            *reinterpret_cast<f32x4*>(p + i) = pp;
            if (MOM != SGD_PLAIN) *reinterpret_cast<f32x4*>(buf + i) = bb;
        } else {
            for (int64_t k = i; k < n; ++k) {
                float pp = p[k], bb = 0.f;
                if (MOM != SGD_PLAIN && !first) bb = buf[k];
                sgd_update<WD, MOM>(pp, g[k], bb, first, lr, mom, keep, wd, gscale);
                p[k] = pp;
                if (MOM != SGD_PLAIN) buf[k] = bb;
            }
        }
    }
}

static int sweep_blocks(int64_t n) { return (int)std::min<int64_t>((n / 4 + 255) / 256 + 1, 2048); }      // (Adam's grid)

// what the two entry points below check about the device-resident step count and learning rate
static const char* bad_step_or_lr(int64_t step, const int64_t* step_count, float lr, const float* lr_dev) {
    if (!step_count && step < 1) return "step must be >= 1 (or step_count given)";
    if ((uintptr_t)step_count & 7) return "step_count must be 8-byte aligned";
    if ((uintptr_t)lr_dev & 3) return "lr_dev must be 4-byte aligned";
    if (!lr_dev && !(lr >= 0.f)) return "lr must be >= 0";
    return nullptr;
}

extern "C" int mshgnn_sgd_step(float* params, const float* grads, float* momentum_buf, int64_t n, int64_t step, int64_t* step_count, float lr,
                               const float* lr_dev, float momentum, float dampening, float weight_decay, int nesterov, float grad_scale, void* stream) {
    if (!params || !grads || n < 1) return set_err(MSHGNN_EINVAL, "bad argument to mshgnn_sgd_step");
    if (!(momentum >= 0.f) || !(weight_decay >= 0.f) || dampening != dampening) return set_err(MSHGNN_EINVAL, "mshgnn_sgd_step: momentum and weight_decay must be >= 0");
    if ((momentum != 0.f) != (momentum_buf != nullptr)) return set_err(MSHGNN_EINVAL, "mshgnn_sgd_step: momentum_buf must be given exactly when momentum != 0");
    if (nesterov && (momentum <= 0.f || dampening != 0.f)) return set_err(MSHGNN_EINVAL, "mshgnn_sgd_step: nesterov needs momentum > 0 and dampening == 0");
    if (((uintptr_t)params | (uintptr_t)grads | (uintptr_t)momentum_buf) & 15) return set_err(MSHGNN_EINVAL, "sgd buffers must be 16-byte aligned");
    if (const char* why = bad_step_or_lr(step, step_count, lr, lr_dev)) return set_err(MSHGNN_EINVAL, std::string("mshgnn_sgd_step: ") + why);
    const int mom = momentum == 0.f ? SGD_PLAIN : nesterov ? SGD_NESTEROV : SGD_MOMENTUM;
    const bool wd = weight_decay != 0.f;
    auto kernel = mom == SGD_PLAIN ? (wd ? k_sgd<true, SGD_PLAIN> : k_sgd<false, SGD_PLAIN>)
                : mom == SGD_MOMENTUM ? (wd ? k_sgd<true, SGD_MOMENTUM> : k_sgd<false, SGD_MOMENTUM>)
                                      : (wd ? k_sgd<true, SGD_NESTEROV> : k_sgd<false, SGD_NESTEROV>);
    hipLaunchKernelGGL(kernel, dim3(sweep_blocks(n)), dim3(256), 0, (hipStream_t)stream, params, grads, momentum_buf, n, (const int64_t*)step_count,
                       step == 1 ? 1 : 0, lr, lr_dev, momentum, dampening, weight_decay, grad_scale);
    if (step_count) hipLaunchKernelGGL(k_step_count_inc, dim3(1), dim3(1), 0, (hipStream_t)stream, step_count);
    HIPCHK(hipGetLastError());
    return MSHGNN_OK;
}

// Adam with weight decay.  MODE == ADAM_PLAIN runs adam_sweep itself (the bits of k_adam / k_adam_counted); the other two restate it, in its order of
// operations, with g' = g s + wd p entering both moments (coupled) or p scaled by 1 - lr wd first (decoupled).  The bias corrections arrive as arguments
// (formed on the host from `step`) or are formed as k_adam_counted forms them when step_count is given.
template <int MODE> __global__ void k_adamw(float* p, const float* g, float* m, float* v, int64_t n, const int64_t* step_count, float lr, const float* lr_dev,
                                            float b1, float b2, float eps, float wd, float bc1, float bc2_sqrt, float gscale) {
    __shared__ float s_bc[2];
    if (step_count) {
        if (threadIdx.x == 0) {
            double a1 = (double)b1, a2 = (double)b2, r1 = 1.0, r2 = 1.0;
            for (int64_t t = *step_count + 1; t > 0; t >>= 1) {
                if (t & 1) { r1 *= a1; r2 *= a2; }
                a1 *= a1; a2 *= a2;
            }
            s_bc[0] = (float)(1.0 - r1); s_bc[1] = (float)sqrt(1.0 - r2);
        }
        __syncthreads();
        bc1 = s_bc[0]; bc2_sqrt = s_bc[1];
    }
    if (lr_dev) lr = *lr_dev;
    if (MODE == ADAM_PLAIN) {
        adam_sweep(p, g, m, v, n, lr, b1, b2, eps, bc1, bc2_sqrt, gscale);
        return;
    }
    for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += (int64_t)gridDim.x * blockDim.x * 4) {
        if (i + 4 <= n) {
            f32x4 pp = *reinterpret_cast<f32x4*>(p + i), gg = *reinterpret_cast<const f32x4*>(g + i) * gscale;
            f32x4 mm = *reinterpret_cast<f32x4*>(m + i), vv = *reinterpret_cast<f32x4*>(v + i);
            if (MODE == ADAM_COUPLED) gg += wd * pp;
            else pp *= 1.f - lr * wd;
            mm = b1 * mm + (1.f - b1) * gg;
            vv = b2 * vv + (1.f - b2) * gg * gg;
#pragma unroll
            for (int e = 0; e < 4; ++e) pp[e] -= lr / bc1 * mm[e] / (sqrtf(vv[e]) / bc2_sqrt + eps);
            *reinterpret_cast<f32x4*>(p + i) = pp; *reinterpret_cast<f32x4*>(m + i) = mm; *reinterpret_cast<f32x4*>(v + i) = vv;
        } else {
            for (int64_t k = i; k < n; ++k) {
                float pp = p[k], gg = g[k] * gscale;
                if (MODE == ADAM_COUPLED) gg += wd * pp;
                else pp *= 1.f - lr * wd;
                m[k] = b1 * m[k] + (1.f - b1) * gg; v[k] = b2 * v[k] + (1.f - b2) * gg * gg;
                p[k] = pp - lr / bc1 * m[k] / (sqrtf(v[k]) / bc2_sqrt + eps);
            }
        }
    }
}

extern "C" int mshgnn_adamw_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, int64_t step, int64_t* step_count,
                                 float lr, const float* lr_dev, float beta1, float beta2, float eps, float weight_decay, int decoupled, float grad_scale,
                                 void* stream) {
    if (!params || !grads || !exp_avg || !exp_avg_sq || n < 1) return set_err(MSHGNN_EINVAL, "bad argument to mshgnn_adamw_step");
    if (!(weight_decay >= 0.f)) return set_err(MSHGNN_EINVAL, "mshgnn_adamw_step: weight_decay must be >= 0");
    if (((uintptr_t)params | (uintptr_t)grads | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) return set_err(MSHGNN_EINVAL, "adam buffers must be 16-byte aligned");
    if (const char* why = bad_step_or_lr(step, step_count, lr, lr_dev)) return set_err(MSHGNN_EINVAL, std::string("mshgnn_adamw_step: ") + why);
    float bc1 = 1.f, bc2_sqrt = 1.f;
    if (!step_count) {      // (as mshgnn_adam_step forms them)
        bc1 = (float)(1.0 - std::pow((double)beta1, (double)step));
        bc2_sqrt = (float)std::sqrt(1.0 - std::pow((double)beta2, (double)step));
    }
    auto kernel = weight_decay == 0.f ? k_adamw<ADAM_PLAIN> : decoupled ? k_adamw<ADAM_DECOUPLED> : k_adamw<ADAM_COUPLED>;
    hipLaunchKernelGGL(kernel, dim3(sweep_blocks(n)), dim3(256), 0, (hipStream_t)stream, params, grads, exp_avg, exp_avg_sq, n, (const int64_t*)step_count, lr,
                       lr_dev, beta1, beta2, eps, weight_decay, bc1, bc2_sqrt, grad_scale);
    if (step_count) hipLaunchKernelGGL(k_step_count_inc, dim3(1), dim3(1), 0, (hipStream_t)stream, step_count);
    HIPCHK(hipGetLastError());
    return MSHGNN_OK;
}

__global__ void k_mse(const float* out, const float* y, int64_t n, float* loss, float* gout) {
    __shared__ float red[4];
    float s = 0.f;
    const float inv = 1.0f / (float)n;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float dlt = out[i] - y[i];
        s += dlt * dlt;
        if (gout) gout[i] = 2.0f * dlt * inv;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(loss, (red[0] + red[1] + red[2] + red[3]) * inv);
}

extern "C" int mshgnn_mse_loss(const float* out, const float* y, int64_t n, float* loss_out, float* grad_out, void* stream) {
    if (!out || !y || !loss_out || n < 1) return set_err(MSHGNN_EINVAL, "bad argument to mshgnn_mse_loss");
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipMemsetAsync(loss_out, 0, sizeof(float), st));
    const int blocks = (int)std::min<int64_t>((n + 255) / 256, 1024);
    hipLaunchKernelGGL(k_mse, dim3(blocks), dim3(256), 0, st, out, y, n, loss_out, grad_out);
    HIPCHK(hipGetLastError());
    return MSHGNN_OK;
}

// Stand-alone contact cross entropy of the classification wrappers (gnnLightning.py:640-648, customMetrics.py:6-25: CrossEntropyLoss over
// the [rows, 2] per-foot logits, batch value = sum / rows) with its gradient (softmax - onehot) / rows.  One thread per row.
__global__ void k_ce(const float* logits, const int32_t* labels, int64_t rows, float* loss, float* gout) {
    __shared__ float red[4];
    float s = 0.f;
    const float inv = 1.0f / (float)rows;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += (int64_t)gridDim.x * blockDim.x) {
        const float l0 = logits[2 * r], l1 = logits[2 * r + 1];
        const float m = fmaxf(l0, l1);
        const float e0 = expf(l0 - m), e1 = expf(l1 - m), z = e0 + e1;
        const int lab = labels[r] != 0;
        s += logf(z) + m - (lab ? l1 : l0);
        if (gout) {
            gout[2 * r] = (e0 / z - (lab ? 0.f : 1.f)) * inv;
            gout[2 * r + 1] = (e1 / z - (lab ? 1.f : 0.f)) * inv;
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(loss, (red[0] + red[1] + red[2] + red[3]) * inv);
}

extern "C" int mshgnn_ce_loss(const float* logits, const int32_t* labels, int64_t rows, float* loss_out, float* grad_out, void* stream) {
    if (!logits || !labels || !loss_out || rows < 1) return set_err(MSHGNN_EINVAL, "bad argument to mshgnn_ce_loss");
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipMemsetAsync(loss_out, 0, sizeof(float), st));
    const int blocks = (int)std::min<int64_t>((rows + 255) / 256, 1024);
    hipLaunchKernelGGL(k_ce, dim3(blocks), dim3(256), 0, st, logits, labels, rows, loss_out, grad_out);
    HIPCHK(hipGetLastError());
    return MSHGNN_OK;
}

// ------------------------------------------------------------------------------------------------------
// Step metrics of the Lightning wrappers, on device.  The reference keeps
// torchmetrics states that are plain sums across steps (gnnLightning.py:52-63, customMetrics.py:11-54); these kernels
// ADD one step's sums into caller-owned state buffers.  One workgroup, fixed reduction order: deterministic.
// ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}
__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// Both kernels run on up to MET_BLOCKS workgroups: every workgroup leaves its partial sums in the caller's scratch, takes a ticket, and the
// workgroup that draws the last ticket adds the partials IN INDEX ORDER (bit-reproducible whatever the arrival order) and resets the
// ticket.  The one-workgroup entry points (mshgnn_metrics_regression / _classification, no scratch) run the same kernels with one block.
constexpr int MET_COUNTS = 18, MET_BLOCKS = 64, MET_THREADS = 256;
struct MetScratch {
    unsigned int ticket, pad;
    double f[MET_BLOCKS][2];
    long long c[MET_BLOCKS][MET_COUNTS];
};
static_assert(sizeof(MetScratch) <= MSHGNN_METRICS_SCRATCH_BYTES, "include/mshgnn.h promises this scratch size");

__device__ __forceinline__ void met_store(double* p, double v) { __hip_atomic_store(reinterpret_cast<long long*>(p), __double_as_longlong(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ double met_load(const double* p) { return __longlong_as_double(__hip_atomic_load(reinterpret_cast<const long long*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)); }
__device__ __forceinline__ void met_store(long long* p, long long v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ long long met_load(const long long* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// thread 0 of every workgroup, after its partials are stored: true in the workgroup that arrives last (sc == nullptr: a one-block launch)
__device__ __forceinline__ bool met_last_ticket(unsigned int* ticket) {
    __atomic_thread_fence(__ATOMIC_RELEASE);        // (agent scope: the partials reach memory every XCD's L2 sees)
    const unsigned int t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (t != gridDim.x - 1) return false;
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    return true;
}
__device__ __forceinline__ bool met_last_block(MetScratch* sc) { return !sc || met_last_ticket(&sc->ticket); }

// ------------------------------------------------------------------------------------------------------
// L2 norm of the flat gradient and the clipping sweep (torch.nn.utils.clip_grad_norm_, norm_type 2), with the ticket pattern above: no floating-point atomic,
// the same bits for the same n whatever the arrival order.  Grid = norm_blocks(n) workgroups of 256 threads, a function of n alone (include/mshgnn.h).
// A lane adds the squares of its grid-stride quads in ascending order (fp64: an fp32 square is exact), a wave reduces in the fixed butterfly of wave_sum,
// thread 0 adds the four waves in order and leaves the workgroup's partial in the scratch; the last workgroup adds the partials in index order.
// ------------------------------------------------------------------------------------------------------
constexpr int NORM_THREADS = 256, NORM_BLOCKS = 256;
struct NormScratch {
    unsigned int ticket, pad[3];
    double part[NORM_BLOCKS];
};
static int norm_blocks(int64_t n) { return (int)std::min<int64_t>(((n + 3) / 4 + NORM_THREADS - 1) / NORM_THREADS, NORM_BLOCKS); }

__global__ __launch_bounds__(NORM_THREADS) void k_grad_norm(const float* g, int64_t n, double* norm_out, NormScratch* sc) {
    __shared__ double r[NORM_THREADS / 64], pf[NORM_BLOCKS];
    __shared__ int s_last;
    double s = 0.0;
    for (int64_t i = ((int64_t)blockIdx.x * NORM_THREADS + threadIdx.x) * 4; i < n; i += (int64_t)gridDim.x * NORM_THREADS * 4) {
        if (i + 4 <= n) {
            const f32x4 q = *reinterpret_cast<const f32x4*>(g + i);
#pragma unroll
            for (int e = 0; e < 4; ++e) { const double x = (double)q[e]; s += x * x; }
        } else {
            for (int64_t k = i; k < n; ++k) { const double x = (double)g[k]; s += x * x; }
        }
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) r[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int k = 0; k < NORM_THREADS / 64; ++k) t += r[k];
        met_store(&sc->part[blockIdx.x], t);
        s_last = met_last_ticket(&sc->ticket) ? 1 : 0;
    }
    __syncthreads();
    if (!s_last) return;
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    if (threadIdx.x < gridDim.x) pf[threadIdx.x] = met_load(&sc->part[threadIdx.x]);      // (gridDim.x <= NORM_BLOCKS == NORM_THREADS: one partial per thread)
    __syncthreads();
    if (threadIdx.x == 0) {      // index order; eight LDS reads in flight ahead of their (dependent) additions
        double t = 0.0;
        unsigned b = 0;
        for (; b + 8 <= gridDim.x; b += 8) {
            double x[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) x[k] = pf[b + k];
#pragma unroll
            for (int k = 0; k < 8; ++k) t += x[k];
        }
        for (; b < gridDim.x; ++b) t += pf[b];
        __hip_atomic_store(&sc->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        *norm_out = sqrt(t);
    }
}
static_assert(NORM_BLOCKS <= NORM_THREADS, "the last workgroup loads one partial per thread");

// ------------------------------------------------------------------------------------------------------
// mshgnn_regression_loss: MSE / L1 / Huber with their gradient for the two-call routes, ONE launch with the ticket pattern above (no memset, no floating-point atomic:
// two runs give the same bits).  Kind 0 evaluates k_mse's expressions, kinds 1 and 2 reg_loss_terms (mshgnn_device.hpp) -- the function the fused tails call.
// A lane adds the terms of its grid-stride quads in ascending order (fp32), a wave reduces in the fixed butterfly, thread 0 adds the four waves in order; the workgroup that
// finishes last adds the workgroups' partials in index order and multiplies by inv_n once.  VEC: all three pointers are 16-byte aligned (16-byte loads and stores; the same bits).
// ------------------------------------------------------------------------------------------------------
constexpr int REGL_THREADS = 256, REGL_BLOCKS = 256;
struct RegLossScratch {
    unsigned int ticket, pad[3];
    float part[REGL_BLOCKS];
};
static int regl_blocks(int64_t n) { return (int)std::min<int64_t>(((n + 3) / 4 + REGL_THREADS - 1) / REGL_THREADS, REGL_BLOCKS); }
__device__ __forceinline__ void regl_elem(float o, float y, float inv, int kind, float delta, float& g, float& s) {
    const float dlt = o - y;
    if (kind == MSHGNN_REG_LOSS_MSE) { s += dlt * dlt; g = 2.0f * dlt * inv; }
    else { float term; reg_loss_terms(dlt, inv, kind, delta, g, term); s += term; }
}
template <bool VEC> __global__ __launch_bounds__(REGL_THREADS) void k_reg_loss(const float* out, const float* y, int64_t n, int kind, float delta, float* loss, float* gout,
                                                                               RegLossScratch* sc) {
    __shared__ float r[REGL_THREADS / 64], pf[REGL_BLOCKS];
    __shared__ int s_last;
    const float inv = 1.0f / (float)n;
    float s = 0.f;
    for (int64_t i = ((int64_t)blockIdx.x * REGL_THREADS + threadIdx.x) * 4; i < n; i += (int64_t)gridDim.x * REGL_THREADS * 4) {
        if (VEC && i + 4 <= n) {
            const f32x4 o = *reinterpret_cast<const f32x4*>(out + i), t = *reinterpret_cast<const f32x4*>(y + i);
            f32x4 g;
#pragma unroll
            for (int e = 0; e < 4; ++e) { float ge; regl_elem(o[e], t[e], inv, kind, delta, ge, s); g[e] = ge; }
            if (gout) *reinterpret_cast<f32x4*>(gout + i) = g;
        } else {
            for (int64_t k = i; k < min(i + 4, n); ++k) { float ge; regl_elem(out[k], y[k], inv, kind, delta, ge, s); if (gout) gout[k] = ge; }
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
    if ((threadIdx.x & 63) == 0) r[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
        for (int k = 0; k < REGL_THREADS / 64; ++k) t += r[k];
        __hip_atomic_store(reinterpret_cast<unsigned int*>(&sc->part[blockIdx.x]), __float_as_uint(t), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = met_last_ticket(&sc->ticket) ? 1 : 0;
    }
    __syncthreads();
    if (!s_last) return;
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    if (threadIdx.x < gridDim.x)      // (gridDim.x <= REGL_BLOCKS == REGL_THREADS: one partial per thread)
        pf[threadIdx.x] = __uint_as_float(__hip_atomic_load(reinterpret_cast<const unsigned int*>(&sc->part[threadIdx.x]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    __syncthreads();
    if (threadIdx.x == 0) {      // index order
        float t = 0.f;
        for (unsigned b = 0; b < gridDim.x; ++b) t += pf[b];
        __hip_atomic_store(&sc->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        *loss = t * inv;
    }
}
static_assert(REGL_BLOCKS <= REGL_THREADS, "the last workgroup loads one partial per thread");

extern "C" size_t mshgnn_regression_loss_scratch_bytes(int64_t n) { return n < 1 ? 0 : sizeof(RegLossScratch); }
extern "C" int mshgnn_regression_loss(const float* out, const float* y, int64_t n, int kind, float delta, float* loss_out, float* grad_out, void* scratch, void* stream) {
    if (!out || !y || !loss_out || !scratch || n < 1) return set_err(MSHGNN_EINVAL, "bad argument to mshgnn_regression_loss");
    if (const int rc = check_regression_loss(kind, delta, "mshgnn_regression_loss")) return rc;
    if ((uintptr_t)scratch & 15) return set_err(MSHGNN_EINVAL, "mshgnn_regression_loss: the scratch must be 16-byte aligned");
    const bool vec = (((uintptr_t)out | (uintptr_t)y | (uintptr_t)grad_out) & 15) == 0;
    hipLaunchKernelGGL(vec ? k_reg_loss<true> : k_reg_loss<false>, dim3(regl_blocks(n)), dim3(REGL_THREADS), 0, (hipStream_t)stream, out, y, n, kind, delta, loss_out,
                       grad_out, reinterpret_cast<RegLossScratch*>(scratch));
    HIPCHK(hipGetLastError());
    return MSHGNN_OK;
}

// g *= c, c = fl32(min(1, max_norm / (norm + 1e-6))) formed in fp64 by one thread of the workgroup (a NaN norm gives a NaN coefficient, as torch's clamp does)
__global__ void k_grad_clip(float* g, int64_t n, const double* norm, float max_norm) {
    __shared__ float s_c;
    if (threadIdx.x == 0) {
        const double q = (double)max_norm / (*norm + 1e-6);
        s_c = (float)(q > 1.0 ? 1.0 : q);
    }
    __syncthreads();
    const float c = s_c;
    for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += (int64_t)gridDim.x * blockDim.x * 4) {
        if (i + 4 <= n) *reinterpret_cast<f32x4*>(g + i) = *reinterpret_cast<f32x4*>(g + i) * c;
        else for (int64_t k = i; k < n; ++k) g[k] *= c;
    }
}

extern "C" size_t mshgnn_grad_norm_scratch_bytes(int64_t n) {
    return n < 1 ? 0 : offsetof(NormScratch, part) + (((size_t)norm_blocks(n) * sizeof(double) + 15) & ~(size_t)15);
}

extern "C" int mshgnn_grad_norm(const float* grads, int64_t n, double* norm_out, void* scratch, void* stream) {
    if (!grads || !norm_out || !scratch || n < 1) return set_err(MSHGNN_EINVAL, "bad argument to mshgnn_grad_norm");
    if (((uintptr_t)grads | (uintptr_t)scratch) & 15) return set_err(MSHGNN_EINVAL, "mshgnn_grad_norm: grads and scratch must be 16-byte aligned");
    if ((uintptr_t)norm_out & 7) return set_err(MSHGNN_EINVAL, "mshgnn_grad_norm: norm_out must be 8-byte aligned");
    hipLaunchKernelGGL(k_grad_norm, dim3(norm_blocks(n)), dim3(NORM_THREADS), 0, (hipStream_t)stream, grads, n, norm_out, (NormScratch*)scratch);
    HIPCHK(hipGetLastError());
    return MSHGNN_OK;
}

extern "C" int mshgnn_grad_clip(float* grads, int64_t n, const double* norm, float max_norm, void* stream) {
    if (!grads || !norm || n < 1) return set_err(MSHGNN_EINVAL, "bad argument to mshgnn_grad_clip");
    if (!(max_norm >= 0.f)) return set_err(MSHGNN_EINVAL, "mshgnn_grad_clip: max_norm must be >= 0");
    if ((uintptr_t)grads & 15) return set_err(MSHGNN_EINVAL, "mshgnn_grad_clip: grads must be 16-byte aligned");
    if ((uintptr_t)norm & 7) return set_err(MSHGNN_EINVAL, "mshgnn_grad_clip: norm must be 8-byte aligned");
    hipLaunchKernelGGL(k_grad_clip, dim3(sweep_blocks(n)), dim3(256), 0, (hipStream_t)stream, grads, n, norm, max_norm);
    HIPCHK(hipGetLastError());
    return MSHGNN_OK;
}

// regression (calculate_losses_step, gnnLightning.py:124-130): sums of (pred - y)^2, |pred - y| and n; `batch` (nullable) receives this
// step's sums (overwritten), `epoch` (nullable) has them added; gout (nullable) = d mean((pred - y)^2) / d pred = 2 (pred - y) / n
template <int NT> __global__ __launch_bounds__(NT) void k_metrics_reg(const float* pred, const float* y, int64_t n, double* batch, double* epoch, float* gout,
                                                             MetScratch* sc) {
    __shared__ double r0[NT / 64], r1[NT / 64], pf[MET_BLOCKS][2];
    __shared__ int s_last;
    double s = 0.0, a = 0.0;
    const double inv2 = 2.0 / (double)n;
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) {
        const double dlt = (double)pred[i] - (double)y[i];
        s += dlt * dlt; a += fabs(dlt);
        if (gout) gout[i] = (float)(dlt * inv2);
    }
    s = wave_sum(s); a = wave_sum(a);
    if ((threadIdx.x & 63) == 0) { r0[threadIdx.x >> 6] = s; r1[threadIdx.x >> 6] = a; }
    __syncthreads();
    double ts = 0.0, ta = 0.0;
    if (threadIdx.x == 0) {
        for (int k = 0; k < NT / 64; ++k) { ts += r0[k]; ta += r1[k]; }
        if (sc) { met_store(&sc->f[blockIdx.x][0], ts); met_store(&sc->f[blockIdx.x][1], ta); }
        s_last = met_last_block(sc) ? 1 : 0;
    }
    if (sc) {
        __syncthreads();
        if (!s_last) return;
        __atomic_thread_fence(__ATOMIC_ACQUIRE);
        // the last workgroup: one partial per thread (all loads in flight at once), then thread 0 adds them in workgroup order
        if (threadIdx.x < gridDim.x) { pf[threadIdx.x][0] = met_load(&sc->f[threadIdx.x][0]); pf[threadIdx.x][1] = met_load(&sc->f[threadIdx.x][1]); }
        __syncthreads();
        if (threadIdx.x == 0) {
            ts = ta = 0.0;
            for (unsigned b = 0; b < gridDim.x; ++b) { ts += pf[b][0]; ta += pf[b][1]; }
            __hip_atomic_store(&sc->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (threadIdx.x == 0) {
        if (batch) {      // the sums, then the step's published values: MSE, RMSE, L1 (gnnLightning.py:124-130)
            batch[0] = ts; batch[1] = ta; batch[2] = (double)n; batch[3] = ts / (double)n; batch[4] = sqrt(ts / (double)n); batch[5] = ta / (double)n;
            batch[6] = batch[7] = 0.0;
        }
        if (epoch) { epoch[0] += ts; epoch[1] += ta; epoch[2] += (double)n; }
    }
}

// one window of the classification metrics: its four per-foot cross entropies added to `ce`, its counters to `c` (layout below), its gradient
// rows to gout (nullable).  Shared by k_metrics_cls and k_metrics_cls_seg.
__device__ __forceinline__ void met_cls_window(const float* logits, const int32_t* y, int64_t w, int64_t B, float* gout, double& ce, long long (&c)[MET_COUNTS]) {
    double p1[4];
    int state = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double l0 = (double)logits[(w * 4 + k) * 2], l1 = (double)logits[(w * 4 + k) * 2 + 1];
        const double m = fmax(l0, l1), e0 = exp(l0 - m), e1 = exp(l1 - m), se = e0 + e1;
        const int lab = y[w * 4 + k] != 0;
        ce += (m + log(se)) - (lab ? l1 : l0);
        const double p0 = e0 / se; p1[k] = e1 / se;
        if (gout) {
            const double inv = 1.0 / (double)(4 * B);
            gout[(w * 4 + k) * 2] = (float)((p0 - (lab ? 0.0 : 1.0)) * inv);
            gout[(w * 4 + k) * 2 + 1] = (float)((p1[k] - (lab ? 1.0 : 0.0)) * inv);
        }
        const int pred = p1[k] > p0 ? 1 : 0;             // argmax over (p0, p1): the first maximum wins
        const int cell = pred ? (lab ? 0 : 1) : (lab ? 2 : 3);      // tp, fp, fn, tn -- added by compare, not by a run-time index (the counters stay in registers)
#pragma unroll
        for (int j = 0; j < 4; ++j) c[2 + 4 * k + j] += (cell == j);
        state = state * 2 + lab;
    }
    int best = 0; double bestv = -1.0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const double f0 = (j & 8) ? p1[0] : 1.0 - p1[0], f1 = (j & 4) ? p1[1] : 1.0 - p1[1];
        const double f2 = (j & 2) ? p1[2] : 1.0 - p1[2], f3 = (j & 1) ? p1[3] : 1.0 - p1[3];
        const double v = (f0 * f1) * (f2 * f3);
        if (v > bestv) { bestv = v; best = j; }
    }
    c[0] += 1; c[1] += (best == state);
}

// classification (gnnLightning.py:132-151, 285-348): logits [B*4][2], labels [B][4] in {0,1}.
//   ce_state[0] += sum of per-foot cross entropies, ce_state[1] += 4 B                      (customMetrics.py:17-24)
//   counts[0] += B, counts[1] += windows whose 16-class argmax equals the label state       (Accuracy, 16 classes)
//   counts[2 + 4 k + {0,1,2,3}] += tp, fp, fn, tn of leg k                                   (BinaryF1Score)
// The 16-class probabilities are the reference's products (p or 1 - p per foot, ((f0 f1)(f2 f3)), first maximum wins).
// ce_b / counts_b (nullable): this step's sums, overwritten; ce_state / counts (nullable): added into; gout (nullable) [B*4][2] = d ce / d logits
// = (softmax - onehot) / (4 B)
template <int NT> __global__ __launch_bounds__(NT) void k_metrics_cls(const float* logits, const int32_t* y, int64_t B, double* ce_b, long long* counts_b,
                                                             double* ce_state, long long* counts, float* gout, MetScratch* sc) {
    __shared__ double rce[NT / 64];
    __shared__ long long rc[NT / 64][MET_COUNTS], pc[MET_BLOCKS][MET_COUNTS];
    __shared__ double pce[MET_BLOCKS];
    __shared__ int s_last;
    double ce = 0.0;
    long long c[MET_COUNTS];
#pragma unroll
    for (int k = 0; k < MET_COUNTS; ++k) c[k] = 0;
    for (int64_t w = (int64_t)blockIdx.x * NT + threadIdx.x; w < B; w += (int64_t)gridDim.x * NT) met_cls_window(logits, y, w, B, gout, ce, c);
    ce = wave_sum(ce);
#pragma unroll
    for (int k = 0; k < MET_COUNTS; ++k) c[k] = wave_sum(c[k]);
    if ((threadIdx.x & 63) == 0) {
        rce[threadIdx.x >> 6] = ce;
#pragma unroll
        for (int k = 0; k < MET_COUNTS; ++k) rc[threadIdx.x >> 6][k] = c[k];
    }
    __syncthreads();
    // this workgroup's sums: thread 0 the cross entropy, threads 0..17 one count each
    double tce = 0.0; long long tc = 0;
    if (threadIdx.x == 0) for (int k = 0; k < NT / 64; ++k) tce += rce[k];
    if (threadIdx.x < MET_COUNTS) for (int k = 0; k < NT / 64; ++k) tc += rc[k][threadIdx.x];
    if (sc) {
        if (threadIdx.x == 0) met_store(&sc->f[blockIdx.x][0], tce);
        if (threadIdx.x < MET_COUNTS) met_store(&sc->c[blockIdx.x][threadIdx.x], tc);
        __syncthreads();                                    // every partial of this workgroup is stored before thread 0 takes the ticket
        if (threadIdx.x == 0) s_last = met_last_block(sc) ? 1 : 0;
        __syncthreads();
        if (!s_last) return;
        __atomic_thread_fence(__ATOMIC_ACQUIRE);
        // the last workgroup: thread b fetches workgroup b's partials (all loads in flight at once), then one thread per sum adds them in workgroup order
        if (threadIdx.x < gridDim.x) {
            pce[threadIdx.x] = met_load(&sc->f[threadIdx.x][0]);
#pragma unroll
            for (int k = 0; k < MET_COUNTS; ++k) pc[threadIdx.x][k] = met_load(&sc->c[threadIdx.x][k]);
        }
        __syncthreads();
        tce = 0.0; tc = 0;
        if (threadIdx.x == 0) for (unsigned b = 0; b < gridDim.x; ++b) tce += pce[b];
        if (threadIdx.x < MET_COUNTS) for (unsigned b = 0; b < gridDim.x; ++b) tc += pc[b][threadIdx.x];
        if (threadIdx.x == 0) __hip_atomic_store(&sc->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (threadIdx.x == 0) {
        if (ce_b) { ce_b[0] = tce; ce_b[1] = (double)(4 * B); ce_b[2] = (double)(float)tce / (double)(4 * B); }      // [2]: this step's CE, `summed_loss.float() / total_num` (customMetrics.py:24)
        if (ce_state) { ce_state[0] += tce; ce_state[1] += (double)(4 * B); }
    }
    if (threadIdx.x < MET_COUNTS) {
        if (counts_b) counts_b[threadIdx.x] = tc;
        if (counts) counts[threadIdx.x] += tc;
        if (ce_b) pc[0][threadIdx.x] = tc;                  // (pc: free again -- every partial has been added)
    }
    if (ce_b) {      // the step's published values next to its sums: [3] 16-class accuracy, [4..7] F1 of leg 0..3 (customMetrics.py:51-54, 0/0 -> 0)
        __syncthreads();
        if (threadIdx.x == 0) ce_b[3] = (double)pc[0][1] / (double)pc[0][0];
        if (threadIdx.x >= 1 && threadIdx.x <= 4) {
            const int k = threadIdx.x - 1;
            const double tp = (double)pc[0][2 + 4 * k], fp = (double)pc[0][3 + 4 * k], fn = (double)pc[0][4 + 4 * k];
            const double precision = tp / (tp + fp), recall = tp / (tp + fn);
            const double f1 = 2.0 * (precision * recall) / (precision + recall);
            ce_b[4 + k] = f1 != f1 ? 0.0 : f1;
        }
    }
}

// centroidal-momentum wrappers (gnnLightning_com.py:96-121): y / y_pred [B][nb][6] = per base node (lin(3) | ang(3)), standardised.
//   state[0] += sum sq err of the lin halves, [1] += of the ang halves, [2] += 3 nb B, [3] += 3 nb B,
//   [4] += sum over windows of cos(lin_pred, lin) of base node 0 after un-standardising (v * y_std + y_mean), [5] += the same for ang,
//   [6] += B.  Cosine similarity as torch.nn.CosineSimilarity(dim=1, eps=1e-8): sum (a / max(|a|, eps)) (b / max(|b|, eps))
//   (customMetrics.py:56-95).  One thread per window; multi-workgroup with the ticket scheme above.
struct MetScratchCom { unsigned int ticket, pad; double f[MET_BLOCKS][4]; };
static_assert(sizeof(MetScratchCom) <= MSHGNN_METRICS_SCRATCH_BYTES, "include/mshgnn.h promises this scratch size");
struct ComStats { double mean[6], std[6]; };

// window w's terms added into a = {sq lin, sq ang, cos lin, cos ang}: the squared differences over (base, k) in index order, then each cosine
// (shared by the whole-batch kernel and the segmented one below: one statement of a window's operations)
__device__ __forceinline__ void com_window_add(const float* pred, const float* y, int64_t w, int nb, const ComStats& st, double (&a)[4]) {
    for (int b = 0; b < nb; ++b)
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const double d = (double)pred[(w * nb + b) * 6 + k] - (double)y[(w * nb + b) * 6 + k];
            a[k < 3 ? 0 : 1] += d * d;
        }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        double pp = 0.0, yy = 0.0, py = 0.0, pv[3], yv[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            pv[k] = (double)pred[w * nb * 6 + 3 * h + k] * st.std[3 * h + k] + st.mean[3 * h + k];
            yv[k] = (double)y[w * nb * 6 + 3 * h + k] * st.std[3 * h + k] + st.mean[3 * h + k];
            pp += pv[k] * pv[k]; yy += yv[k] * yv[k];
        }
        const double pn = fmax(sqrt(pp), 1e-8), yn = fmax(sqrt(yy), 1e-8);
#pragma unroll
        for (int k = 0; k < 3; ++k) py += (pv[k] / pn) * (yv[k] / yn);
        a[2 + h] += py;
    }
}

__global__ __launch_bounds__(MET_THREADS) void k_metrics_com(const float* pred, const float* y, int64_t B, int nb, ComStats st, double* batch, double* epoch,
                                                             MetScratchCom* sc) {
    __shared__ double r[MET_THREADS / 64][4], pf[MET_BLOCKS][4];
    __shared__ int s_last;
    double a[4] = {0.0, 0.0, 0.0, 0.0};      // sq lin, sq ang, cos lin, cos ang
    for (int64_t w = (int64_t)blockIdx.x * MET_THREADS + threadIdx.x; w < B; w += (int64_t)gridDim.x * MET_THREADS) com_window_add(pred, y, w, nb, st, a);
#pragma unroll
    for (int k = 0; k < 4; ++k) a[k] = wave_sum(a[k]);
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int k = 0; k < 4; ++k) r[threadIdx.x >> 6][k] = a[k];
    __syncthreads();
    double t[4] = {0.0, 0.0, 0.0, 0.0};
    if (threadIdx.x == 0) {
        for (int v = 0; v < MET_THREADS / 64; ++v)
#pragma unroll
            for (int k = 0; k < 4; ++k) t[k] += r[v][k];
        if (sc)
#pragma unroll
            for (int k = 0; k < 4; ++k) met_store(&sc->f[blockIdx.x][k], t[k]);
        s_last = 1;
        if (sc) {
            __atomic_thread_fence(__ATOMIC_RELEASE);
            const unsigned int tk = __hip_atomic_fetch_add(&sc->ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
            s_last = tk == gridDim.x - 1;
        }
    }
    if (sc) {
        __syncthreads();
        if (!s_last) return;
        __atomic_thread_fence(__ATOMIC_ACQUIRE);
        if (threadIdx.x < gridDim.x)
#pragma unroll
            for (int k = 0; k < 4; ++k) pf[threadIdx.x][k] = met_load(&sc->f[threadIdx.x][k]);
        __syncthreads();
        if (threadIdx.x == 0) {
#pragma unroll
            for (int k = 0; k < 4; ++k) t[k] = 0.0;
            for (unsigned b = 0; b < gridDim.x; ++b)
#pragma unroll
                for (int k = 0; k < 4; ++k) t[k] += pf[b][k];
            __hip_atomic_store(&sc->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (threadIdx.x == 0) {
        const double n3 = 3.0 * (double)nb * (double)B;
        const double v[8] = {t[0], t[1], n3, n3, t[2], t[3], (double)B, 0.0};
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (batch) batch[k] = v[k];
            if (epoch) epoch[k] += v[k];
        }
    }
}

// GRF body frame -> world frame (gnnLightning.py:663-676): quat = world->body rotation, scalar-last (x, y, z, w) as scipy's
// Rotation.from_quat takes it (normalised here as scipy does); world = R(quat)^-1 f for each of the 4 feet.
__global__ void k_grf_to_world(const float* quat, const float* body, float* world, int64_t B) {
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= B) return;
    double x = quat[w * 4], yq = quat[w * 4 + 1], z = quat[w * 4 + 2], s = quat[w * 4 + 3];
    const double nrm = sqrt(x * x + yq * yq + z * z + s * s);
    x /= nrm; yq /= nrm; z /= nrm; s /= nrm;
    // R = matrix of the unit quaternion; its inverse is the transpose
    const double R[3][3] = {{1 - 2 * (yq * yq + z * z), 2 * (x * yq - z * s), 2 * (x * z + yq * s)},
                            {2 * (x * yq + z * s), 1 - 2 * (x * x + z * z), 2 * (yq * z - x * s)},
                            {2 * (x * z - yq * s), 2 * (yq * z + x * s), 1 - 2 * (x * x + yq * yq)}};
    for (int f = 0; f < 4; ++f) {
        const double b0 = body[w * 12 + f * 3], b1 = body[w * 12 + f * 3 + 1], b2 = body[w * 12 + f * 3 + 2];
#pragma unroll
        for (int i = 0; i < 3; ++i) world[w * 12 + f * 3 + i] = (float)(R[0][i] * b0 + R[1][i] * b1 + R[2][i] * b2);
    }
}

// ------------------------------------------------------------------------------------------------------
// Segmented step metrics (include/mshgnn.h): the same sums per SEGMENT -- window b's sums go to row segment[b] of the state, ids outside
// [0, n_segments) to the extra row n_segments.  Bit-reproducible for any arrangement of ids and without a floating-point atomic:
//   * a lane owns a window and adds its terms in index order;
//   * a wave groups its 64 lanes by id: while lanes remain it takes the first remaining lane's id and sums the lanes that hold it (the xor
//     butterfly of wave_sum over the masked values: every lane ends with the same bits; a group of one lane is copied, not summed) -- one
//     entry (id, windows, sums) per distinct id, in order of first appearance, into slot (window index / 64) of the caller's scratch;
//   * the workgroup that draws the last ticket merges: thread t owns the ids == t (mod SEG_THREADS) and walks ALL entries in (slot, entry)
//     order -- staged through LDS behind a prefix sum of the slots' entry counts, with a bit mask per thread that marks its entries -- adding the entries of its ids;
//     consecutive entries of one id are summed in a register and added to the state's row when the id changes.
// The order of every addition is fixed by the window indices and the ids alone, whichever wave or workgroup arrives first.  An evaluation sweep
// has one or two ids per wave: one or two entries per slot, a merge of 2 .. 3 entries per 64 windows.
// ------------------------------------------------------------------------------------------------------
constexpr int SEG_THREADS = 256, SEG_MAX_BLOCKS = 1024, SEG_STAGE = 1024;
template <int NF> struct SegSlotN { unsigned int n, pad; int id[64]; int cnt[64]; double f[64][NF]; };      // an entry = id, windows and NF sums
using SegSlot = SegSlotN<2>;         // the regression table (squared and absolute error) and the classification table (cross entropy: the first sum alone)
using SegSlotCom = SegSlotN<4>;      // the centroidal-momentum table
struct SegScratch { unsigned int ticket, pad[3]; };      // followed by SegSlot[ceil(batch / 64)]
static_assert(sizeof(SegSlot) == 1544 && sizeof(SegScratch) == 16, "include/mshgnn.h documents 16 + 1544 * ceil(batch / 64) bytes");
static_assert(sizeof(SegSlotCom) == 2568, "include/mshgnn.h documents 16 + 2568 * ceil(batch / 64) bytes");

__device__ __forceinline__ void met_store(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int met_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void met_store(unsigned int* p, unsigned int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ unsigned int met_load(const unsigned int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int seg_row(int32_t id, int32_t n_segments) { return (unsigned)id < (unsigned)n_segments ? id : n_segments; }

// One wave's windows -> its slot.  Every lane of the wave calls this (valid: the lane holds a window); id is a row already (seg_row).
// extra(mine, cnt, leader, row): per-group work of the caller, wave-uniform control flow (the classification counters).
template <int NF, class Extra> __device__ __forceinline__ void seg_wave_emit(SegSlot* slot, bool valid, int id, double f0, double f1, Extra&& extra) {
    const int lane = threadIdx.x & 63;
    unsigned long long rem = __ballot(valid);
    int e = 0, e_id = 0, e_cnt = 0;
    double e0 = 0.0, e1 = 0.0;
    while (rem) {
        const int leader = __ffsll((unsigned long long)rem) - 1;
        const int row = __shfl(id, leader, 64);
        const bool mine = valid && id == row;
        const unsigned long long m = __ballot(mine);
        const int cnt = __popcll(m);
        double s0, s1 = 0.0;
        if (cnt == 1) {
            s0 = __shfl(f0, leader, 64);
            if (NF > 1) s1 = __shfl(f1, leader, 64);
        } else {
            s0 = wave_sum(mine ? f0 : 0.0);
            if (NF > 1) s1 = wave_sum(mine ? f1 : 0.0);
        }
        extra(mine, cnt, leader, row);
        if (lane == e) { e_id = row; e_cnt = cnt; e0 = s0; e1 = s1; }
        ++e;
        rem &= ~m;
    }
    // e <= 64: every pass retires at least the leader's lane
    if (lane < e) {
        met_store(&slot->id[lane], e_id); met_store(&slot->cnt[lane], e_cnt);
        met_store(&slot->f[lane][0], e0);
        if (NF > 1) met_store(&slot->f[lane][1], e1);
    }
    if (lane == 0) met_store(&slot->n, (unsigned)e);
}

// The last workgroup: state[row][0 .. NF - 1] += the entries' sums, state[row][NF] += windows * per_entry, rows 0 .. n_segments.
// Per SEG_THREADS slots: every thread fetches its slot's entry count AND its first two entries in one round of loads (an evaluation sweep's slots hold
// one or two), the counts are prefix-summed, and the entries are staged in LDS in (slot, entry) order -- at once where they fit (the rest of a slot's
// entries in a second round of loads), else SEG_STAGE at a time.  Staging entry j also sets bit j of its owner's row of s_mask (an integer OR: any
// order, the same bits); thread t then walks the set bits of ITS row in increasing j, so it meets the entries of its ids in (slot, entry) order
// without reading anyone else's.
template <int NF> __device__ __forceinline__ void seg_merge(const SegSlot* slots, int64_t n_slots, int32_t n_segments, double* state, int64_t per_entry) {
    __shared__ int s_off[SEG_THREADS + 1], s_wave[SEG_THREADS / 64], s_id[SEG_STAGE], s_cnt[SEG_STAGE];
    __shared__ double s_f[SEG_STAGE][NF];
    __shared__ unsigned int s_mask[SEG_THREADS][SEG_STAGE / 32 + 1];          // (+ 1: the rows start in different banks)
    const int t = threadIdx.x, lane = t & 63;
    for (int w = 0; w < SEG_STAGE / 32; ++w) s_mask[t][w] = 0;          // (its own row; the others set bits in it behind the next barrier)
    int cur = -1;
    long long ccnt = 0;
    double a0 = 0.0, a1 = 0.0;
    auto flush = [&]() {
        if (cur < 0) return;
        double* row = state + (int64_t)cur * (NF + 1);
        const double r0 = row[0], r1 = NF > 1 ? row[1] : 0.0, rn = row[NF];
        row[0] = r0 + a0;
        if (NF > 1) row[1] = r1 + a1;
        row[NF] = rn + (double)(ccnt * per_entry);
    };
    auto stage = [&](int j, int id, int cnt, double f0, double f1) {
        id = seg_row(id, n_segments);
        s_id[j] = id; s_cnt[j] = cnt; s_f[j][0] = f0;
        if (NF > 1) s_f[j][NF - 1] = f1;
        atomicOr(&s_mask[id & (SEG_THREADS - 1)][j >> 5], 1u << (j & 31));
    };
    auto stage_from = [&](int j, const SegSlot* sl, int k) {
        stage(j, met_load(&sl->id[k]), met_load(&sl->cnt[k]), met_load(&sl->f[k][0]), NF > 1 ? met_load(&sl->f[k][1]) : 0.0);
    };
    auto slot_of = [&](int e) {          // s_off[lo] <= e < s_off[lo + 1]: the last slot that starts at or before e holds it
        int lo = 0, hi = SEG_THREADS;
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (s_off[mid] <= e) lo = mid; else hi = mid; }
        return lo;
    };
    auto consume = [&](int te) {
        for (int w = 0; w < (te + 31) >> 5; ++w) {
            unsigned int m = s_mask[t][w];
            if (!m) continue;
            s_mask[t][w] = 0;
            while (m) {
                const int j = (w << 5) + __ffs(m) - 1;
                m &= m - 1;
                const int id = s_id[j];
                if (id != cur) { flush(); cur = id; ccnt = 0; a0 = a1 = 0.0; }
                a0 += s_f[j][0];
                if (NF > 1) a1 += s_f[j][NF - 1];
                ccnt += s_cnt[j];
            }
        }
    };
    for (int64_t c0 = 0; c0 < n_slots; c0 += SEG_THREADS) {
        const bool have = c0 + t < n_slots;
        const SegSlot* mine = slots + (have ? c0 + t : 0);
        int n = 0, pid[2] = {0, 0}, pcnt[2] = {0, 0};
        double pf[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
        if (have) {
            n = (int)min(met_load(&mine->n), 64u);
#pragma unroll
            for (int k = 0; k < 2; ++k) {          // (entry k of a slot with fewer entries: whatever an earlier call left, never used)
                pid[k] = met_load(&mine->id[k]); pcnt[k] = met_load(&mine->cnt[k]);
                pf[k][0] = met_load(&mine->f[k][0]);
                if (NF > 1) pf[k][1] = met_load(&mine->f[k][1]);
            }
        }
        int incl = n;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const int v = __shfl_up(incl, d, 64); if (lane >= d) incl += v; }
        if (lane == 63) s_wave[t >> 6] = incl;
        __syncthreads();
        for (int w = 0; w < (t >> 6); ++w) incl += s_wave[w];
        s_off[t + 1] = incl;
        if (t == 0) s_off[0] = 0;
        const int more = __syncthreads_or(n > 2);
        const int total = s_off[SEG_THREADS];
        if (total <= SEG_STAGE) {
#pragma unroll
            for (int k = 0; k < 2; ++k) if (k < n) stage(incl - n + k, pid[k], pcnt[k], pf[k][0], pf[k][1]);
            if (more) {
                for (int j = t; j < total; j += SEG_THREADS) {
                    const int lo = slot_of(j), k = j - s_off[lo];
                    if (k >= 2) stage_from(j, slots + c0 + lo, k);
                }
            }
            __syncthreads();
            consume(total);
            __syncthreads();
        } else {
            for (int e0 = 0; e0 < total; e0 += SEG_STAGE) {
                const int te = min(SEG_STAGE, total - e0);
                for (int j = t; j < te; j += SEG_THREADS) {
                    const int lo = slot_of(e0 + j);
                    stage_from(j, slots + c0 + lo, e0 + j - s_off[lo]);
                }
                __syncthreads();
                consume(te);
                __syncthreads();
            }
        }
    }
    flush();
}

// every wave's entries are stored and drained, then one ticket per workgroup; true in all threads of the workgroup that arrives last
__device__ __forceinline__ bool seg_last_block(SegScratch* sc) {
    __shared__ int s_last;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) s_last = met_last_ticket(&sc->ticket) ? 1 : 0;
    __syncthreads();
    if (!s_last) return false;
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    return true;
}

__global__ __launch_bounds__(SEG_THREADS) void k_metrics_reg_seg(const float* pred, const float* y, int64_t batch, int per_window, int vec4, const int32_t* segment,
                                                                 int32_t n_segments, double* state, SegScratch* sc) {
    SegSlot* slots = reinterpret_cast<SegSlot*>(sc + 1);
    const int64_t n_slots = (batch + 63) / 64;
    for (int64_t base = (int64_t)blockIdx.x * SEG_THREADS; base < batch; base += (int64_t)gridDim.x * SEG_THREADS) {
        const int64_t w = base + threadIdx.x, wave0 = base + (threadIdx.x & ~63);
        if (wave0 >= batch) continue;          // (wave-uniform: this wave has no window, and no slot)
        const bool valid = w < batch;
        double s = 0.0, a = 0.0;
        int id = 0;
        if (valid) {          // the window's terms in index order, four loads of each operand in flight (vec4: 16-byte loads, the same additions in the same order)
            id = seg_row(segment[w], n_segments);
            const float* p = pred + w * per_window; const float* q = y + w * per_window;
            if (vec4) {
                const f32x4* p4 = reinterpret_cast<const f32x4*>(p); const f32x4* q4 = reinterpret_cast<const f32x4*>(q);
                const int n4 = per_window >> 2;
                for (int i = 0; i < n4; i += 4) {
                    f32x4 pv[4], qv[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) if (i + u < n4) { pv[u] = p4[i + u]; qv[u] = q4[i + u]; }
#pragma unroll
                    for (int u = 0; u < 4; ++u) if (i + u < n4) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) { const double dlt = (double)pv[u][e] - (double)qv[u][e]; s += dlt * dlt; a += fabs(dlt); }
                    }
                }
            } else {
                for (int i = 0; i < per_window; i += 4) {
                    float pv[4], qv[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) if (i + u < per_window) { pv[u] = p[i + u]; qv[u] = q[i + u]; }
#pragma unroll
                    for (int u = 0; u < 4; ++u) if (i + u < per_window) { const double dlt = (double)pv[u] - (double)qv[u]; s += dlt * dlt; a += fabs(dlt); }
                }
            }
        }
        seg_wave_emit<2>(slots + (wave0 >> 6), valid, id, s, a, [](bool, int, int, int) {});
    }
    if (!seg_last_block(sc)) return;
    seg_merge<2>(slots, n_slots, n_segments, state, per_window);
    if (threadIdx.x == 0) __hip_atomic_store(&sc->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// classification: the cross entropies go through the entries like the regression sums; the 18 int64 counters of a group are added to its row
// with integer atomics (exact in any order), lane k the counter k
__global__ __launch_bounds__(SEG_THREADS) void k_metrics_cls_seg(const float* logits, const int32_t* y, int64_t batch, const int32_t* segment, int32_t n_segments,
                                                                 double* ce_state, long long* counts, SegScratch* sc) {
    SegSlot* slots = reinterpret_cast<SegSlot*>(sc + 1);
    const int64_t n_slots = (batch + 63) / 64;
    const int lane = threadIdx.x & 63;
    for (int64_t base = (int64_t)blockIdx.x * SEG_THREADS; base < batch; base += (int64_t)gridDim.x * SEG_THREADS) {
        const int64_t w = base + threadIdx.x, wave0 = base + (threadIdx.x & ~63);
        if (wave0 >= batch) continue;
        const bool valid = w < batch;
        double ce = 0.0;
        long long c[MET_COUNTS];
#pragma unroll
        for (int k = 0; k < MET_COUNTS; ++k) c[k] = 0;
        int id = 0;
        if (valid) {
            id = seg_row(segment[w], n_segments);
            met_cls_window(logits, y, w, batch, nullptr, ce, c);
        }
        seg_wave_emit<1>(slots + (wave0 >> 6), valid, id, ce, 0.0, [&](bool mine, int cnt, int leader, int row) {
            long long v = 0;
#pragma unroll
            for (int k = 0; k < MET_COUNTS; ++k) {
                const long long sum = cnt == 1 ? __shfl(c[k], leader, 64) : wave_sum(mine ? c[k] : 0ll);
                if (lane == k) v = sum;
            }
            if (lane < MET_COUNTS && v) __hip_atomic_fetch_add(counts + (int64_t)row * MET_COUNTS + lane, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        });
    }
    if (!seg_last_block(sc)) return;
    seg_merge<1>(slots, n_slots, n_segments, ce_state, 4);
    if (threadIdx.x == 0) __hip_atomic_store(&sc->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- four sums per entry: the centroidal-momentum sums per segment --------------------------------------------------------------------------
// The same three steps with a wave step and a merge of their own (kept separate from the two-sum ones above: HISTORY.md, "Twin kernels") and the merge's stage depth as a
// template parameter: at
// four sums SEG_STAGE entries of s_f plus the mask rows would pass 64 KB of static LDS, 512 fit in 38 KB.  The merge always takes the
// staged walk, STAGE entries at a time (the two-entry prefetch of seg_merge is a tuning of the evaluation sweeps' regression table, not part of
// the order of additions): thread t adds the entries of the ids == t (mod SEG_THREADS) in (slot, entry) order and hands every finished id to
// `flush_row(row, sums, windows)`.

template <int NF> __device__ __forceinline__ void seg_wave_emit_n(SegSlotN<NF>* slot, bool valid, int id, const double (&f)[NF]) {
    const int lane = threadIdx.x & 63;
    unsigned long long rem = __ballot(valid);
    int e = 0, e_id = 0, e_cnt = 0;
    double ef[NF];
#pragma unroll
    for (int k = 0; k < NF; ++k) ef[k] = 0.0;
    while (rem) {
        const int leader = __ffsll((unsigned long long)rem) - 1;
        const int row = __shfl(id, leader, 64);
        const bool mine = valid && id == row;
        const unsigned long long m = __ballot(mine);
        const int cnt = __popcll(m);
        double s[NF];
#pragma unroll
        for (int k = 0; k < NF; ++k) s[k] = cnt == 1 ? __shfl(f[k], leader, 64) : wave_sum(mine ? f[k] : 0.0);
        if (lane == e) {
            e_id = row; e_cnt = cnt;
#pragma unroll
            for (int k = 0; k < NF; ++k) ef[k] = s[k];
        }
        ++e;
        rem &= ~m;
    }
    if (lane < e) {          // e <= 64: every pass retires at least the leader's lane
        met_store(&slot->id[lane], e_id); met_store(&slot->cnt[lane], e_cnt);
#pragma unroll
        for (int k = 0; k < NF; ++k) met_store(&slot->f[lane][k], ef[k]);
    }
    if (lane == 0) met_store(&slot->n, (unsigned)e);
}

template <int NF, int STAGE, class Flush>
__device__ __forceinline__ void seg_merge_n(const SegSlotN<NF>* slots, int64_t n_slots, int32_t n_segments, Flush&& flush_row) {
    static_assert(STAGE % 32 == 0 && STAGE >= 64, "whole mask words, and room for one slot's entries");
    __shared__ int s_off[SEG_THREADS + 1], s_wave[SEG_THREADS / 64], s_id[STAGE], s_cnt[STAGE];
    __shared__ double s_f[STAGE][NF];
    __shared__ unsigned int s_mask[SEG_THREADS][STAGE / 32 + 1];          // (+ 1: the rows start in different banks)
    const int t = threadIdx.x, lane = t & 63;
    for (int w = 0; w < STAGE / 32; ++w) s_mask[t][w] = 0;          // (its own row; the others set bits in it behind the next barrier)
    int cur = -1;
    long long ccnt = 0;
    double a[NF];
#pragma unroll
    for (int k = 0; k < NF; ++k) a[k] = 0.0;
    auto slot_of = [&](int e) {          // s_off[lo] <= e < s_off[lo + 1]: the last slot that starts at or before e holds it
        int lo = 0, hi = SEG_THREADS;
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (s_off[mid] <= e) lo = mid; else hi = mid; }
        return lo;
    };
    auto consume = [&](int te) {
        for (int w = 0; w < (te + 31) >> 5; ++w) {
            unsigned int m = s_mask[t][w];
            if (!m) continue;
            s_mask[t][w] = 0;
            while (m) {
                const int j = (w << 5) + __ffs(m) - 1;
                m &= m - 1;
                const int id = s_id[j];
                if (id != cur) {
                    if (cur >= 0) flush_row(cur, a, ccnt);
                    cur = id; ccnt = 0;
#pragma unroll
                    for (int k = 0; k < NF; ++k) a[k] = 0.0;
                }
#pragma unroll
                for (int k = 0; k < NF; ++k) a[k] += s_f[j][k];
                ccnt += s_cnt[j];
            }
        }
    };
    for (int64_t c0 = 0; c0 < n_slots; c0 += SEG_THREADS) {
        const bool have = c0 + t < n_slots;
        const int n = have ? (int)min(met_load(&slots[c0 + t].n), 64u) : 0;
        int incl = n;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const int v = __shfl_up(incl, d, 64); if (lane >= d) incl += v; }
        if (lane == 63) s_wave[t >> 6] = incl;
        __syncthreads();
        for (int w = 0; w < (t >> 6); ++w) incl += s_wave[w];
        s_off[t + 1] = incl;
        if (t == 0) s_off[0] = 0;
        __syncthreads();
        const int total = s_off[SEG_THREADS];
        for (int e0 = 0; e0 < total; e0 += STAGE) {
            const int te = min(STAGE, total - e0);
            for (int j = t; j < te; j += SEG_THREADS) {
                const int lo = slot_of(e0 + j), k = e0 + j - s_off[lo];          // (k < the slot's n <= 64; a slot past n_slots has n = 0 and holds no e)
                const SegSlotN<NF>* sl = slots + c0 + lo;
                const int id = seg_row(met_load(&sl->id[k]), n_segments);
                s_id[j] = id; s_cnt[j] = met_load(&sl->cnt[k]);
#pragma unroll
                for (int q = 0; q < NF; ++q) s_f[j][q] = met_load(&sl->f[k][q]);
                atomicOr(&s_mask[id & (SEG_THREADS - 1)][j >> 5], 1u << (j & 31));
            }
            __syncthreads();
            consume(te);
            __syncthreads();
        }
    }
    if (cur >= 0) flush_row(cur, a, ccnt);
}

// centroidal-momentum sums per segment: row s of state [n_segments + 1][8] in the layout of k_metrics_com, a window's terms from com_window_add
__global__ __launch_bounds__(SEG_THREADS) void k_metrics_com_seg(const float* pred, const float* y, int64_t batch, int nb, ComStats st, const int32_t* segment,
                                                                 int32_t n_segments, double* state, SegScratch* sc) {
    SegSlotCom* slots = reinterpret_cast<SegSlotCom*>(sc + 1);
    const int64_t n_slots = (batch + 63) / 64;
    for (int64_t base = (int64_t)blockIdx.x * SEG_THREADS; base < batch; base += (int64_t)gridDim.x * SEG_THREADS) {
        const int64_t w = base + threadIdx.x, wave0 = base + (threadIdx.x & ~63);
        if (wave0 >= batch) continue;          // (wave-uniform: this wave has no window, and no slot)
        const bool valid = w < batch;
        double a[4] = {0.0, 0.0, 0.0, 0.0};
        int id = 0;
        if (valid) {
            id = seg_row(segment[w], n_segments);
            com_window_add(pred, y, w, nb, st, a);
        }
        seg_wave_emit_n<4>(slots + (wave0 >> 6), valid, id, a);
    }
    if (!seg_last_block(sc)) return;
    const double n3 = 3.0 * (double)nb;
    seg_merge_n<4, 512>(slots, n_slots, n_segments, [&](int row, const double (&a)[4], long long cnt) {
        double* r = state + (int64_t)row * 8;
        const double c = (double)cnt;
        r[0] += a[0]; r[1] += a[1]; r[2] += n3 * c; r[3] += n3 * c; r[4] += a[2]; r[5] += a[3]; r[6] += c;
    });
    if (threadIdx.x == 0) __hip_atomic_store(&sc->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

static int met_blocks(int64_t items, int per_thread) {
    return (int)std::max<int64_t>(1, std::min<int64_t>(MET_BLOCKS, (items + per_thread * MET_THREADS - 1) / (per_thread * MET_THREADS)));
}

extern "C" int mshgnn_metrics_regression(const float* y_pred, const float* y, int64_t n, double* state, void* stream) {
    if (!y_pred || !y || !state || n < 1) return set_err(MSHGNN_EINVAL, "bad argument to mshgnn_metrics_regression");
    if ((uintptr_t)state & 7) return set_err(MSHGNN_EINVAL, "mshgnn_metrics_regression: the state must be 8-byte aligned");
    hipLaunchKernelGGL(k_metrics_reg<1024>, dim3(1), dim3(1024), 0, (hipStream_t)stream, y_pred, y, n, (double*)nullptr, state, (float*)nullptr, (MetScratch*)nullptr);
    HIPCHK(hipGetLastError());
    return MSHGNN_OK;
}

extern "C" int mshgnn_metrics_regression_step(const float* y_pred, const float* y, int64_t n, double* batch_state, double* epoch_state, float* grad_out,
                                              void* scratch, void* stream) {
    if (!y_pred || !y || (!batch_state && !epoch_state) || !scratch || n < 1) return set_err(MSHGNN_EINVAL, "bad argument to mshgnn_metrics_regression_step");
    if (((uintptr_t)batch_state | (uintptr_t)epoch_state | (uintptr_t)scratch) & 7)
        return set_err(MSHGNN_EINVAL, "mshgnn_metrics_regression_step: the states and the scratch must be 8-byte aligned");
    hipLaunchKernelGGL(k_metrics_reg<MET_THREADS>, dim3(met_blocks(n, 16)), dim3(MET_THREADS), 0, (hipStream_t)stream, y_pred, y, n, batch_state, epoch_state, grad_out,
                       reinterpret_cast<MetScratch*>(scratch));
    HIPCHK(hipGetLastError());
    return MSHGNN_OK;
}

extern "C" int mshgnn_metrics_classification(const float* logits, const int32_t* y, int64_t batch, double* ce_state, int64_t* counts, void* stream) {
    if (!logits || !y || !ce_state || !counts || batch < 1) return set_err(MSHGNN_EINVAL, "bad argument to mshgnn_metrics_classification");
    if (((uintptr_t)ce_state | (uintptr_t)counts) & 7) return set_err(MSHGNN_EINVAL, "mshgnn_metrics_classification: the states must be 8-byte aligned");
    hipLaunchKernelGGL(k_metrics_cls<1024>, dim3(1), dim3(1024), 0, (hipStream_t)stream, logits, y, batch, (double*)nullptr, (long long*)nullptr, ce_state,
                       reinterpret_cast<long long*>(counts), (float*)nullptr, (MetScratch*)nullptr);
    HIPCHK(hipGetLastError());
    return MSHGNN_OK;
}

extern "C" int mshgnn_metrics_classification_step(const float* logits, const int32_t* y, int64_t batch, double* batch_ce, int64_t* batch_counts,
                                                  double* epoch_ce, int64_t* epoch_counts, float* grad_out, void* scratch, void* stream) {
    if (!logits || !y || batch < 1 || !scratch || (!batch_ce != !batch_counts) || (!epoch_ce != !epoch_counts) || (!batch_ce && !epoch_ce))
        return set_err(MSHGNN_EINVAL, "bad argument to mshgnn_metrics_classification_step");
    if (((uintptr_t)batch_ce | (uintptr_t)batch_counts | (uintptr_t)epoch_ce | (uintptr_t)epoch_counts | (uintptr_t)scratch) & 7)
        return set_err(MSHGNN_EINVAL, "mshgnn_metrics_classification_step: the states and the scratch must be 8-byte aligned");
    hipLaunchKernelGGL(k_metrics_cls<MET_THREADS>, dim3(met_blocks(batch, 1)), dim3(MET_THREADS), 0, (hipStream_t)stream, logits, y, batch, batch_ce,
                       reinterpret_cast<long long*>(batch_counts), epoch_ce, reinterpret_cast<long long*>(epoch_counts), grad_out,
                       reinterpret_cast<MetScratch*>(scratch));
    HIPCHK(hipGetLastError());
    return MSHGNN_OK;
}

extern "C" int mshgnn_metrics_com_step(const float* y_pred, const float* y, int64_t batch, int n_bases, const double* y_mean, const double* y_std,
                                       double* batch_state, double* epoch_state, void* scratch, void* stream) {
    if (!y_pred || !y || !y_mean || !y_std || batch < 1 || n_bases < 1 || !scratch || (!batch_state && !epoch_state))
        return set_err(MSHGNN_EINVAL, "bad argument to mshgnn_metrics_com_step");
    if (((uintptr_t)batch_state | (uintptr_t)epoch_state | (uintptr_t)scratch) & 7)
        return set_err(MSHGNN_EINVAL, "mshgnn_metrics_com_step: the states and the scratch must be 8-byte aligned");
    ComStats st;
    for (int k = 0; k < 6; ++k) { st.mean[k] = y_mean[k]; st.std[k] = y_std[k]; }
    hipLaunchKernelGGL(k_metrics_com, dim3(met_blocks(batch, 1)), dim3(MET_THREADS), 0, (hipStream_t)stream, y_pred, y, batch, n_bases, st, batch_state,
                       epoch_state, reinterpret_cast<MetScratchCom*>(scratch));
    HIPCHK(hipGetLastError());
    return MSHGNN_OK;
}

extern "C" size_t mshgnn_metrics_segmented_scratch_bytes(int64_t batch) {
    return batch < 1 ? 0 : sizeof(SegScratch) + sizeof(SegSlot) * (size_t)((batch + 63) / 64);
}

static int seg_blocks(int64_t batch) { return (int)std::min<int64_t>(SEG_MAX_BLOCKS, (batch + SEG_THREADS - 1) / SEG_THREADS); }

extern "C" int mshgnn_metrics_regression_segmented(const float* y_pred, const float* y, int64_t batch, int32_t per_window, const int32_t* segment,
                                                   int32_t n_segments, double* state, void* scratch, void* stream) {
    if (!y_pred || !y || !segment || !state || !scratch) return set_err(MSHGNN_EINVAL, "null argument to mshgnn_metrics_regression_segmented");
    if (batch < 1 || per_window < 1 || n_segments < 1) return set_err(MSHGNN_EINVAL, "mshgnn_metrics_regression_segmented: batch, per_window and n_segments must be >= 1");
    if ((uintptr_t)scratch & 7) return set_err(MSHGNN_EINVAL, "mshgnn_metrics_regression_segmented: the scratch must be 8-byte aligned");
    hipLaunchKernelGGL(k_metrics_reg_seg, dim3(seg_blocks(batch)), dim3(SEG_THREADS), 0, (hipStream_t)stream, y_pred, y, batch, (int)per_window,
                       (int)(per_window % 4 == 0 && (((uintptr_t)y_pred | (uintptr_t)y) & 15) == 0), segment, n_segments, state, reinterpret_cast<SegScratch*>(scratch));
    HIPCHK(hipGetLastError());
    return MSHGNN_OK;
}

extern "C" int mshgnn_metrics_classification_segmented(const float* logits, const int32_t* y, int64_t batch, const int32_t* segment, int32_t n_segments,
                                                       double* ce_state, int64_t* counts, void* scratch, void* stream) {
    if (!logits || !y || !segment || !ce_state || !counts || !scratch) return set_err(MSHGNN_EINVAL, "null argument to mshgnn_metrics_classification_segmented");
    if (batch < 1 || n_segments < 1) return set_err(MSHGNN_EINVAL, "mshgnn_metrics_classification_segmented: batch and n_segments must be >= 1");
    if ((uintptr_t)scratch & 7) return set_err(MSHGNN_EINVAL, "mshgnn_metrics_classification_segmented: the scratch must be 8-byte aligned");
    hipLaunchKernelGGL(k_metrics_cls_seg, dim3(seg_blocks(batch)), dim3(SEG_THREADS), 0, (hipStream_t)stream, logits, y, batch, segment, n_segments, ce_state,
                       reinterpret_cast<long long*>(counts), reinterpret_cast<SegScratch*>(scratch));
    HIPCHK(hipGetLastError());
    return MSHGNN_OK;
}

extern "C" size_t mshgnn_metrics_com_segmented_scratch_bytes(int64_t batch) {
    return batch < 1 ? 0 : sizeof(SegScratch) + sizeof(SegSlotCom) * (size_t)((batch + 63) / 64);
}

extern "C" int mshgnn_metrics_com_segmented(const float* y_pred, const float* y, int64_t batch, int n_bases, const double* y_mean, const double* y_std,
                                            const int32_t* segment, int32_t n_segments, double* state, void* scratch, void* stream) {
    if (!y_pred || !y || !y_mean || !y_std || !segment || !state || !scratch) return set_err(MSHGNN_EINVAL, "null argument to mshgnn_metrics_com_segmented");
    if (batch < 1 || n_bases < 1 || n_segments < 1) return set_err(MSHGNN_EINVAL, "mshgnn_metrics_com_segmented: batch, n_bases and n_segments must be >= 1");
    if (((uintptr_t)state | (uintptr_t)scratch) & 7) return set_err(MSHGNN_EINVAL, "mshgnn_metrics_com_segmented: the state and the scratch must be 8-byte aligned");
    ComStats st;
    for (int k = 0; k < 6; ++k) { st.mean[k] = y_mean[k]; st.std[k] = y_std[k]; }
    hipLaunchKernelGGL(k_metrics_com_seg, dim3(seg_blocks(batch)), dim3(SEG_THREADS), 0, (hipStream_t)stream, y_pred, y, batch, n_bases, st, segment, n_segments,
                       state, reinterpret_cast<SegScratch*>(scratch));
    HIPCHK(hipGetLastError());
    return MSHGNN_OK;
}

extern "C" int mshgnn_grf_body_to_world(const float* quat, const float* grf_body, float* grf_world, int64_t batch, void* stream) {
    if (!quat || !grf_body || !grf_world || batch < 1) return set_err(MSHGNN_EINVAL, "bad argument to mshgnn_grf_body_to_world");
    hipLaunchKernelGGL(k_grf_to_world, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, (hipStream_t)stream, quat, grf_body, grf_world, batch);
    HIPCHK(hipGetLastError());
    return MSHGNN_OK;
}
