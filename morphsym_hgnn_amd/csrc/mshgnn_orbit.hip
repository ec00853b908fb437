// Symmetrisation over a group orbit (include/mshgnn.h, "orbit averaging"): the average of a model's outputs over the K elements of an orbit-complete batch,
// its exact transpose, and the equivariance defect of the raw outputs.  Plan-independent like mshgnn_train_ops.hip: the three entry points read fp32 outputs
// [K B][n_units width] and host tables, nothing of a plan; they share only the error string with the rest of the library.
//
// The tables travel BY VALUE in the kernel arguments (OrbitTab, 576 bytes): the host call validates perm / sign, packs one index byte per (element, unit)
// and one sign bit per (element, unit), and launches once -- no device tables to own, and a captured graph holds them.  Each workgroup copies the table
// to LDS before its sweep (a lane's unit index is data dependent).  Signs are applied as an XOR of the fp32 sign bit, never as a multiply.
#include "mshgnn_device.hpp"

constexpr int ORBIT_MAX_UNITS = 64, ORBIT_MAX_WIDTH = 16, ORBIT_THREADS = 256, ORBIT_DEFECT_THREADS = 1024;

struct OrbitTab {
    uint64_t neg[MSHGNN_WINDOW_MAX_ELEMENTS];                      // bit u of neg[e]: the term read through idx[e][u] is negated
    uint8_t idx[MSHGNN_WINDOW_MAX_ELEMENTS][ORBIT_MAX_UNITS];      // average / defect: pinv_e[u]; backward: perm[e][u]
};
static_assert(sizeof(OrbitTab) <= 1024, "the orbit tables must fit a by-value kernel argument of 1 KB");

__device__ __forceinline__ void orbit_stage(OrbitTab& s, const OrbitTab& tab) {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(&tab);
    uint32_t* dst = reinterpret_cast<uint32_t*>(&s);
    for (int i = threadIdx.x; i < (int)(sizeof(OrbitTab) / 4); i += blockDim.x) dst[i] = src[i];
    __syncthreads();
}

__device__ __forceinline__ float orbit_signed(float v, const OrbitTab& s, int e, int u) {
    return __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, v) ^ ((uint32_t)((s.neg[e] >> u) & 1) << 31));
}

// V consecutive elements c .. c + V - 1 of one row of `src` read through element e's table: out[v] = +- src[idx[e][u] * width + s], (u, s) = divmod(c + v, width).
// V == 4 is only instantiated for rows of whole quads on 16-byte aligned pointers: a unit of whole quads (width % 4 == 0) then moves as one 16-byte load.
template <int V> __device__ __forceinline__ void orbit_gather(const float* src, const OrbitTab& s, int e, int c, int width, float (&out)[V]) {
    if constexpr (V == 4) {
        if ((width & 3) == 0) {
            const int u = c / width;
            const f32x4 q = *reinterpret_cast<const f32x4*>(src + (int)s.idx[e][u] * width + (c - u * width));
#pragma unroll
            for (int v = 0; v < V; ++v) out[v] = orbit_signed(q[v], s, e, u);
            return;
        }
    }
#pragma unroll
    for (int v = 0; v < V; ++v) {
        const int u = (c + v) / width;
        out[v] = orbit_signed(src[(int)s.idx[e][u] * width + (c + v - u * width)], s, e, u);
    }
}

template <int V> __device__ __forceinline__ void orbit_store(float* dst, const float (&v)[V]) {
    if constexpr (V == 4) *reinterpret_cast<f32x4*>(dst) = f32x4{v[0], v[1], v[2], v[3]};
    else dst[0] = v[0];
}

// avg[w][c] = (t_0 + t_1 + ... + t_{K-1}) * inv_k, t_e = +- o[e B + w][pinv_e[u] width + s]: e ascending, plain fp32 adds starting FROM t_0 (K = 1 keeps every
// bit, the sign of a zero included), then the one multiply.  One thread per output element (V = 1) or per aligned quad of them (V = 4); same bits.
template <int V> __global__ void __launch_bounds__(ORBIT_THREADS) k_orbit_average(const OrbitTab tab, int K, int width, int row, const float* __restrict__ o,
                                                                                  int64_t B, float* __restrict__ avg, float inv_k) {
    __shared__ OrbitTab s;
    orbit_stage(s, tab);
    const int64_t n = B * row;
    for (int64_t i = ((int64_t)blockIdx.x * ORBIT_THREADS + threadIdx.x) * V; i < n; i += (int64_t)gridDim.x * ORBIT_THREADS * V) {
        const int64_t w = i / row;
        const int c = (int)(i - w * row);
        float acc[V], t[V];
        orbit_gather<V>(o + w * row, s, 0, c, width, acc);
        for (int e = 1; e < K; ++e) {
            orbit_gather<V>(o + ((int64_t)e * B + w) * row, s, e, c, width, t);
#pragma unroll
            for (int v = 0; v < V; ++v) acc[v] = acc[v] + t[v];
        }
#pragma unroll
        for (int v = 0; v < V; ++v) acc[v] = acc[v] * inv_k;
        orbit_store<V>(avg + i, acc);
    }
}

// The transpose: g_o[e B + w][k width + s] = sign[e][k] (g_avg[w][perm[e][k] width + s] * inv_k) -- one thread per element (or aligned quad) of g_o.
template <int V> __global__ void __launch_bounds__(ORBIT_THREADS) k_orbit_average_bwd(const OrbitTab tab, int K, int width, int row, const float* __restrict__ g_avg,
                                                                                      int64_t B, float* __restrict__ g_o, float inv_k) {
    __shared__ OrbitTab s;
    orbit_stage(s, tab);
    const int64_t per_el = B * row, n = per_el * K;
    for (int64_t i = ((int64_t)blockIdx.x * ORBIT_THREADS + threadIdx.x) * V; i < n; i += (int64_t)gridDim.x * ORBIT_THREADS * V) {
        const int e = (int)(i / per_el);
        const int64_t r = i - (int64_t)e * per_el, w = r / row;
        const int c = (int)(r - w * row);
        float g[V];
        orbit_gather<V>(g_avg + w * row, s, e, c, width, g);      // (the sign is an XOR: it commutes bit for bit with the multiply behind it)
#pragma unroll
        for (int v = 0; v < V; ++v) g[v] = g[v] * inv_k;
        orbit_store<V>(g_o + i, g);
    }
}

// Equivariance defect: workgroup e compares element e, mapped back, with element 0 over all B row values: d = t_e - o_0 in fp32, then in fp64
// {sum d^2, sum o_0^2, max |d|}.  Bit-reproducible: thread t adds its elements t, t + 1024, ... in that order, the 1024 partials fold in a fixed tree
// (stride 512, 256, ..., 1), thread 0 adds the result into state[e] (max: maxes).  Row 0 writes zeros for sum d^2 and max |d|.  No floating-point atomic.
// One workgroup per element is the contract (K <= 8 workgroups: a diagnostic, not a hot path); 1024 threads and four loads in flight keep its serial sweep short.
__global__ void __launch_bounds__(ORBIT_DEFECT_THREADS) k_orbit_defect(const OrbitTab tab, int width, int row, const float* __restrict__ o, int64_t B, double* __restrict__ state) {
    __shared__ OrbitTab s;
    __shared__ double red[3][ORBIT_DEFECT_THREADS];
    orbit_stage(s, tab);
    const int e = blockIdx.x, tid = threadIdx.x;
    const int64_t n = B * row;
    double sd = 0.0, s0 = 0.0, mx = 0.0;
#pragma unroll 4
    for (int64_t i = tid; i < n; i += ORBIT_DEFECT_THREADS) {
        const int64_t w = i / row;
        const int c = (int)(i - w * row);
        float t[1];
        orbit_gather<1>(o + ((int64_t)e * B + w) * row, s, e, c, width, t);
        const float x0 = o[i], d = t[0] - x0;
        const double dd = (double)d, x = (double)x0;
        sd += dd * dd;      // (an fp32 square is exact in fp64: fused or not, the same bits)
        s0 += x * x;
        mx = fmax(mx, fabs(dd));
    }
    red[0][tid] = sd; red[1][tid] = s0; red[2][tid] = mx;
    __syncthreads();
    for (int st = ORBIT_DEFECT_THREADS / 2; st > 0; st >>= 1) {
        if (tid < st) {
            red[0][tid] += red[0][tid + st];
            red[1][tid] += red[1][tid + st];
            red[2][tid] = fmax(red[2][tid], red[2][tid + st]);
        }
        __syncthreads();
    }
    if (tid == 0) {
        double* out = state + 4 * e;
        if (e == 0) { out[0] = 0.0; out[2] = 0.0; }
        else { out[0] += red[0][0]; out[2] = fmax(out[2], red[2][0]); }
        out[1] += red[1][0];
        out[3] += (double)n;
    }
}

// Validates the host tables and packs them.  inverse: idx[e][u] = pinv_e[u], bit u of neg[e] = (sign[e][pinv_e[u]] < 0) -- what a gather INTO unit u of the
// identity frame reads; else idx = perm, neg = sign -- what a scatter written as a gather into unit k of element e reads.
static int orbit_pack(const char* fn, const int32_t* perm, const int32_t* sign, int32_t K, int32_t U, int32_t width, int64_t windows, bool inverse, OrbitTab& tab) {
    const std::string who(fn);
    if (!perm || !sign) return set_err(MSHGNN_EINVAL, who + ": null table pointer");
    if (K < 1 || K > MSHGNN_WINDOW_MAX_ELEMENTS) return set_err(MSHGNN_EINVAL, who + ": n_elements " + std::to_string(K) + " outside [1, 8]");
    if (U < 1 || U > ORBIT_MAX_UNITS) return set_err(MSHGNN_EINVAL, who + ": n_units " + std::to_string(U) + " outside [1, 64]");
    if (width < 1 || width > ORBIT_MAX_WIDTH) return set_err(MSHGNN_EINVAL, who + ": width " + std::to_string(width) + " outside [1, 16]");
    if (windows < 1) return set_err(MSHGNN_EINVAL, who + ": windows must be >= 1");
    if (windows > (INT64_MAX >> 14) / K) return set_err(MSHGNN_EINVAL, who + ": windows * n_elements * n_units * width does not fit the 64-bit element index");
    std::memset(&tab, 0, sizeof(tab));
    for (int e = 0; e < K; ++e) {
        int pinv[ORBIT_MAX_UNITS];
        for (int u = 0; u < U; ++u) pinv[u] = -1;
        for (int k = 0; k < U; ++k) {
            const int32_t p = perm[e * U + k], c = sign[e * U + k];
            if (p < 0 || p >= U || pinv[p] >= 0) return set_err(MSHGNN_EINVAL, who + ": row " + std::to_string(e) + " of perm is not a permutation of [0, n_units)");
            if (c != 1 && c != -1) return set_err(MSHGNN_EINVAL, who + ": sign[" + std::to_string(e) + "][" + std::to_string(k) + "] = " + std::to_string(c) + " is not +-1");
            if (e == 0 && (p != k || c != 1)) return set_err(MSHGNN_EINVAL, who + ": element 0 must be the identity with sign +1");
            pinv[p] = k;
        }
        for (int u = 0; u < U; ++u) {
            const int src = inverse ? pinv[u] : perm[e * U + u];
            tab.idx[e][u] = (uint8_t)src;
            if (sign[e * U + (inverse ? src : u)] < 0) tab.neg[e] |= (uint64_t)1 << u;
        }
    }
    return MSHGNN_OK;
}

static int orbit_blocks(int64_t n, int V) { return (int)std::min<int64_t>((n / V + ORBIT_THREADS - 1) / ORBIT_THREADS, 4096); }
static bool orbit_quads(int row, const void* a, const void* b) { return row % 4 == 0 && (((uintptr_t)a | (uintptr_t)b) & 15) == 0; }

extern "C" int mshgnn_orbit_average(const int32_t* perm, const int32_t* sign, int32_t n_elements, int32_t n_units, int32_t width, const float* out,
                                    int64_t windows, float* avg, void* stream) {
    if (!out || !avg) return set_err(MSHGNN_EINVAL, "mshgnn_orbit_average: null buffer");
    OrbitTab tab;
    if (int rc = orbit_pack("mshgnn_orbit_average", perm, sign, n_elements, n_units, width, windows, true, tab)) return rc;
    const int row = n_units * width;
    const int64_t n = windows * row;
    const float inv_k = 1.0f / (float)n_elements;
    if (orbit_quads(row, out, avg))
        hipLaunchKernelGGL(k_orbit_average<4>, dim3(orbit_blocks(n, 4)), dim3(ORBIT_THREADS), 0, (hipStream_t)stream, tab, n_elements, width, row, out, windows, avg, inv_k);
    else
        hipLaunchKernelGGL(k_orbit_average<1>, dim3(orbit_blocks(n, 1)), dim3(ORBIT_THREADS), 0, (hipStream_t)stream, tab, n_elements, width, row, out, windows, avg, inv_k);
    HIPCHK(hipGetLastError());
    return MSHGNN_OK;
}

extern "C" int mshgnn_orbit_average_backward(const int32_t* perm, const int32_t* sign, int32_t n_elements, int32_t n_units, int32_t width, const float* grad_avg,
                                             int64_t windows, float* grad_out, void* stream) {
    if (!grad_avg || !grad_out) return set_err(MSHGNN_EINVAL, "mshgnn_orbit_average_backward: null buffer");
    OrbitTab tab;
    if (int rc = orbit_pack("mshgnn_orbit_average_backward", perm, sign, n_elements, n_units, width, windows, false, tab)) return rc;
    const int row = n_units * width;
    const int64_t n = windows * row * n_elements;
    const float inv_k = 1.0f / (float)n_elements;
    if (orbit_quads(row, grad_avg, grad_out))
        hipLaunchKernelGGL(k_orbit_average_bwd<4>, dim3(orbit_blocks(n, 4)), dim3(ORBIT_THREADS), 0, (hipStream_t)stream, tab, n_elements, width, row, grad_avg, windows,
                           grad_out, inv_k);
    else
        hipLaunchKernelGGL(k_orbit_average_bwd<1>, dim3(orbit_blocks(n, 1)), dim3(ORBIT_THREADS), 0, (hipStream_t)stream, tab, n_elements, width, row, grad_avg, windows,
                           grad_out, inv_k);
    HIPCHK(hipGetLastError());
    return MSHGNN_OK;
}

extern "C" int mshgnn_orbit_defect(const int32_t* perm, const int32_t* sign, int32_t n_elements, int32_t n_units, int32_t width, const float* out, int64_t windows,
                                   double* state, void* stream) {
    if (!out || !state) return set_err(MSHGNN_EINVAL, "mshgnn_orbit_defect: null buffer");
    if ((uintptr_t)state & 7) return set_err(MSHGNN_EINVAL, "mshgnn_orbit_defect: state must be 8-byte aligned");
    OrbitTab tab;
    if (int rc = orbit_pack("mshgnn_orbit_defect", perm, sign, n_elements, n_units, width, windows, true, tab)) return rc;
    hipLaunchKernelGGL(k_orbit_defect, dim3(n_elements), dim3(ORBIT_DEFECT_THREADS), 0, (hipStream_t)stream, tab, width, n_units * width, out, windows, state);
    HIPCHK(hipGetLastError());
    return MSHGNN_OK;
}
