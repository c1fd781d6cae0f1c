// TRPO's policy update around the Fisher-vector product (pfrl/agents/trpo.py:415-699,
// pfrl/utils/conjugate_gradient.py).  The product itself stays autograd's double backward; what
// surrounds it in the reference is a chain of small launches that each end in a host read
// (`if torch.norm(residual) < tol`, `float(new_gain)`, `float(new_kl)`).  Here:
//   pfrl_trpo_gaussian_eval   gain, KL(old || new), entropy of a state-independent-scale Gaussian
//                             policy over the whole dataset (+ the gradient of the gain), one launch
//                             + a one-workgroup finish
//   pfrl_cg_init / _step      conjugate gradient with every scalar in a device state block
//   pfrl_trpo_scale_step      full_step = sqrt(2 max_kl / (d.Fd + 1e-8)) d
//   pfrl_params_axpy          param_i = base + step_size * full_step over all parameter tensors
// All sums are f64 in a fixed order (wave shuffles, LDS in wave order, partials in block order):
// two runs give the same bits.  No float atomics.
#include <hip/hip_runtime.h>

#include "common.h"
#include "gaussian_rows.h"

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = 4096;                 // elements of a vector per workgroup (16 per thread)
constexpr int kOneWgThreads = 1024;
constexpr int kOneWgReach = 8192;            // a whole CG step in ONE workgroup up to this length

// Sum of `v` over the workgroup, the same value in every thread: shuffles inside a wave, the wave
// sums through LDS, added in wave order.  `s_w` holds blockDim.x / 64 doubles and is free again after
// the next __syncthreads() of the caller.
__device__ __forceinline__ double block_sum_f64(double v, double *s_w) {
    v = wave_sum_f64(v);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    const int waves = (int)(blockDim.x >> 6);
    for (int w = 0; w < waves; ++w) s += s_w[w];
    return s;
}

// Sum of partial[0 .. n) over the workgroup: thread t takes t, t + blockDim, ... in index order.
// Every workgroup of the same size gets the same bits from the same partials.
__device__ __forceinline__ double fold_partials(const double *__restrict__ partial, int n, double *s_w) {
    double acc = 0.0;
    for (int b = threadIdx.x; b < n; b += blockDim.x) acc += partial[b];
    return block_sum_f64(acc, s_w);
}

// ---------------------------------------------------------------------------------------------
// gain / KL / entropy of Independent(Normal(mean [M][A], scale [A])) against the old policy
//   gain    = mean_m exp(log pi(a_m) - log pi_old(a_m)) adv_m + entropy_coef * H     (trpo.py:415-420)
//   KL      = mean_m sum_j [ 0.5 ((mo_mj - m_mj) / s_j)^2 ] + sum_j 0.5 (v_j - 1 - log v_j),
//             v_j = (so_j / s_j)^2                          (torch.distributions kl_normal_normal)
//   d gain / d mean_mj = g_m (a_mj - m_mj) / s_j^2,   g_m = ratio_m adv_m / M
//   d gain / d scale_j = sum_m g_m ((a_mj - m_mj)^2 / s_j^3 - 1 / s_j) + entropy_coef / s_j
// partial[block][2 + A]: sum of ratio adv, sum of the row part of the KL, the A scale-gradient sums.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_trpo_gaussian_eval(
    const float *__restrict__ mean, const float *__restrict__ scale, const float *__restrict__ mean_old,
    const float *__restrict__ action, const float *__restrict__ adv, const float *__restrict__ logp_old,
    int M, int A, float *__restrict__ dmean, double *__restrict__ partial) {
    __shared__ double s_red[2 + kMaxA][kThreads / 64];
    const int m = blockIdx.x * kThreads + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool live = m < M;
    const size_t base = (size_t)(live ? m : 0) * A;
    double sur = 0.0, kl = 0.0;
    float g = 0.f;
    if (live) {
        const float lpa = row_log_prob(action + base, mean + base, scale, A);
        const float ratio = expf(lpa - logp_old[m]);
        const float term = ratio * adv[m];
        sur = (double)term;
        g = term / (float)M;
        for (int j = 0; j < A; ++j) {
            const double t = ((double)mean_old[base + j] - (double)mean[base + j]) / (double)scale[j];
            kl += 0.5 * (t * t);
        }
    }
    sur = wave_sum_f64(sur);
    kl = wave_sum_f64(kl);
    if (lane == 0) {
        s_red[0][wave] = sur;
        s_red[1][wave] = kl;
    }
    const int cols = dmean != nullptr ? 2 + A : 2;
    if (dmean != nullptr) gaussian_grad_columns(live, g, action, mean, scale, base, A, dmean, s_red, 2);
    block_fold(s_red, cols, partial, 2 + A);
}

// out3 = {gain, mean KL, mean entropy}; dscale[j] when asked for
__global__ __launch_bounds__(64) void k_trpo_gaussian_finish(
    const double *__restrict__ partial, int nblk, int M, int A, float ent_coef,
    const float *__restrict__ scale, const float *__restrict__ scale_old, float *__restrict__ out3,
    float *__restrict__ dscale) {
    const int lane = threadIdx.x;
    const int cols = dscale != nullptr ? 2 + A : 2;
    double head[2] = {0.0, 0.0};
    for (int k = 0; k < cols; ++k) {
        const double s = fold_column(partial, nblk, 2 + A, k);
        if (k < 2) head[k] = s;
        else if (lane == 0)
            dscale[k - 2] = (float)(s + (double)ent_coef / (double)scale[k - 2]);
    }
    if (lane == 0) {
        // (the terms and the order of gaussian_entropy, inside the one pass over scale that this
        // single lane makes: a second loop costs it 32 more dependent loads)
        double H = 0.0, kl_scale = 0.0;
        for (int j = 0; j < A; ++j) {
            H += (double)(kEntropyConst + logf(scale[j]));
            if (scale_old[j] != scale[j]) {     // (equal scales contribute exactly 0)
                const double q = (double)scale_old[j] / (double)scale[j];
                const double v = q * q;
                kl_scale += 0.5 * (v - 1.0 - log(v));
            }
        }
        const float Hf = (float)H;
        out3[0] = (float)(head[0] / M) + ent_coef * Hf;
        out3[1] = (float)(head[1] / M + kl_scale);
        out3[2] = Hf;
    }
}

// ---------------------------------------------------------------------------------------------
// conjugate gradient (pfrl/utils/conjugate_gradient.py).  state = {rr, pAp, step, done}.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_cg_init(const float *__restrict__ b, float *__restrict__ x,
                                                      float *__restrict__ r, float *__restrict__ p,
                                                      int64_t n, double *__restrict__ partial) {
    __shared__ double s_w[kThreads / 64];
    const int64_t lo = (int64_t)blockIdx.x * kChunk;
    double acc = 0.0;
#pragma unroll
    for (int u = 0; u < kChunk / kThreads; ++u) {
        const int64_t i = lo + u * kThreads + threadIdx.x;
        if (i < n) {
            const float v = b[i];
            x[i] = 0.f;
            r[i] = v;
            p[i] = v;
            acc += (double)v * (double)v;
        }
    }
    acc = block_sum_f64(acc, s_w);
    if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

__global__ __launch_bounds__(kThreads) void k_cg_init_finish(const double *__restrict__ partial, int nblk,
                                                             double *__restrict__ state) {
    __shared__ double s_w[kThreads / 64];
    const double rr = fold_partials(partial, nblk, s_w);
    if (threadIdx.x == 0) {
        state[0] = rr;
        state[1] = 0.0;
        state[2] = 0.0;
        state[3] = 0.0;
    }
}

// a whole step in one workgroup (n <= kOneWgReach)
__global__ __launch_bounds__(kOneWgThreads) void k_cg_step_one(float *__restrict__ x, float *__restrict__ r,
                                                               float *__restrict__ p,
                                                               const float *__restrict__ Ap,
                                                               double *__restrict__ state, int n, float tol) {
    __shared__ double s_a[kOneWgThreads / 64], s_b[kOneWgThreads / 64];
    if (state[3] != 0.0) return;            // converged earlier: nothing changes (uniform branch)
    const double rr = state[0];
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += kOneWgThreads) acc += (double)Ap[i] * (double)p[i];
    const double pAp = block_sum_f64(acc, s_a);
    const float alpha = (float)(rr / pAp);
    acc = 0.0;
    for (int i = threadIdx.x; i < n; i += kOneWgThreads) {
        const float pi = p[i];
        x[i] = x[i] + alpha * pi;
        const float ri = r[i] - alpha * Ap[i];
        r[i] = ri;
        acc += (double)ri * (double)ri;
    }
    const double rr1 = block_sum_f64(acc, s_b);
    const bool done = sqrt(rr1) < (double)tol;
    if (!done) {
        const float beta = (float)(rr1 / rr);
        // (thread t reads back exactly the r[i] it wrote above)
        for (int i = threadIdx.x; i < n; i += kOneWgThreads) p[i] = r[i] + beta * p[i];
    }
    if (threadIdx.x == 0) {
        if (!done) state[0] = rr1;
        state[1] = pAp;
        state[2] = (double)alpha;
        state[3] = done ? 1.0 : 0.0;
    }
}

// the same step for longer vectors: partial sums + every workgroup folding them identically
__global__ __launch_bounds__(kThreads) void k_cg_dot(const float *__restrict__ a, const float *__restrict__ b,
                                                     const double *__restrict__ state, int64_t n,
                                                     double *__restrict__ partial) {
    __shared__ double s_w[kThreads / 64];
    if (state != nullptr && state[3] != 0.0) return;
    const int64_t lo = (int64_t)blockIdx.x * kChunk;
    double acc = 0.0;
#pragma unroll
    for (int u = 0; u < kChunk / kThreads; ++u) {
        const int64_t i = lo + u * kThreads + threadIdx.x;
        if (i < n) acc += (double)a[i] * (double)b[i];
    }
    acc = block_sum_f64(acc, s_w);
    if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

__global__ __launch_bounds__(kThreads) void k_cg_update_xr(float *__restrict__ x, float *__restrict__ r,
                                                           const float *__restrict__ p,
                                                           const float *__restrict__ Ap,
                                                           const double *__restrict__ state, int64_t n,
                                                           const double *__restrict__ partial_pAp, int nblk,
                                                           double *__restrict__ partial_rr) {
    __shared__ double s_a[kThreads / 64], s_b[kThreads / 64];
    if (state[3] != 0.0) return;
    const double pAp = fold_partials(partial_pAp, nblk, s_a);
    const float alpha = (float)(state[0] / pAp);
    const int64_t lo = (int64_t)blockIdx.x * kChunk;
    double acc = 0.0;
#pragma unroll
    for (int u = 0; u < kChunk / kThreads; ++u) {
        const int64_t i = lo + u * kThreads + threadIdx.x;
        if (i < n) {
            x[i] = x[i] + alpha * p[i];
            const float ri = r[i] - alpha * Ap[i];
            r[i] = ri;
            acc += (double)ri * (double)ri;
        }
    }
    acc = block_sum_f64(acc, s_b);
    if (threadIdx.x == 0) partial_rr[blockIdx.x] = acc;
}

__global__ __launch_bounds__(kThreads) void k_cg_update_p(const float *__restrict__ r, float *__restrict__ p,
                                                          const double *__restrict__ state, int64_t n,
                                                          const double *__restrict__ partial_rr, int nblk,
                                                          float tol) {
    __shared__ double s_w[kThreads / 64];
    if (state[3] != 0.0) return;
    const double rr1 = fold_partials(partial_rr, nblk, s_w);
    if (sqrt(rr1) < (double)tol) return;
    const float beta = (float)(rr1 / state[0]);
    const int64_t lo = (int64_t)blockIdx.x * kChunk;
#pragma unroll
    for (int u = 0; u < kChunk / kThreads; ++u) {
        const int64_t i = lo + u * kThreads + threadIdx.x;
        if (i < n) p[i] = r[i] + beta * p[i];
    }
}

// the state block of the long-vector step, written once every workgroup above has read it (a launch
// of its own: the stream orders it behind them)
__global__ __launch_bounds__(kThreads) void k_cg_step_finish(double *__restrict__ state,
                                                             const double *__restrict__ partial_pAp,
                                                             const double *__restrict__ partial_rr, int nblk,
                                                             float tol) {
    __shared__ double s_a[kThreads / 64], s_b[kThreads / 64];
    if (state[3] != 0.0) return;
    const double pAp = fold_partials(partial_pAp, nblk, s_a);
    const double rr1 = fold_partials(partial_rr, nblk, s_b);
    if (threadIdx.x == 0) {
        const double rr = state[0];
        const bool done = sqrt(rr1) < (double)tol;
        if (!done) state[0] = rr1;
        state[1] = pAp;
        state[2] = (double)(float)(rr / pAp);
        state[3] = done ? 1.0 : 0.0;
    }
}

// full_step = sqrt(2 max_kl / (d.Fd + 1e-8)) d  (trpo.py:596-598: the dot product a float32 made a
// Python float, the scale a Python float that multiplies a float32 tensor); out2 = {scale, d.Fd}
__global__ __launch_bounds__(kThreads) void k_trpo_scale_step(const float *__restrict__ d, int64_t n,
                                                              const double *__restrict__ partial, int nblk,
                                                              double max_kl, float *__restrict__ full_step,
                                                              float *__restrict__ out2) {
    __shared__ double s_w[kThreads / 64];
    const float dFd = (float)fold_partials(partial, nblk, s_w);
    const float scale = (float)sqrt(2.0 * max_kl / ((double)dFd + 1e-8));
    const int64_t lo = (int64_t)blockIdx.x * kChunk;
#pragma unroll
    for (int u = 0; u < kChunk / kThreads; ++u) {
        const int64_t i = lo + u * kThreads + threadIdx.x;
        if (i < n) full_step[i] = scale * d[i];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        out2[0] = scale;
        out2[1] = dFd;
    }
}

// param_t[i] = base[off_t + i] + step_size * full_step[off_t + i]: a multiply, then an add, each
// rounded (what `flat_params + step_size * full_step` gives).  step_size == 0 copies base, which is
// what the reference does when the line search fails (trpo.py:694-699), also where full_step is not
// finite.
struct AxpyArgs {
    float *p[PFRL_OPT_MAX_TENSORS];
    int64_t numel[PFRL_OPT_MAX_TENSORS];
    int64_t offset[PFRL_OPT_MAX_TENSORS];
    int32_t chunk_end[PFRL_OPT_MAX_TENSORS];
    int32_t n;
};

__global__ __launch_bounds__(kThreads) void k_params_axpy(AxpyArgs a, const float *__restrict__ base,
                                                          const float *__restrict__ full_step,
                                                          float step_size) {
    int t = 0;
    const int b = blockIdx.x;
    while (t < a.n - 1 && b >= a.chunk_end[t]) ++t;
    const int64_t lo = (int64_t)(b - (t == 0 ? 0 : a.chunk_end[t - 1])) * kChunk;
    float *__restrict__ out = a.p[t];
    const int64_t n = a.numel[t], off = a.offset[t];
#pragma unroll
    for (int u = 0; u < kChunk / kThreads; ++u) {
        const int64_t i = lo + u * kThreads + threadIdx.x;
        if (i < n) {
            const float v = base[off + i];
            out[i] = step_size == 0.f ? v : __fadd_rn(v, __fmul_rn(step_size, full_step[off + i]));
        }
    }
}

inline int chunks_of(int64_t n) { return (int)((n + kChunk - 1) / kChunk); }

}  // namespace

extern "C" int pfrl_trpo_gaussian_eval(const float *mean, const float *scale, const float *mean_old,
                                       const float *scale_old, const float *action, const float *adv,
                                       const float *log_prob_old, int32_t M, int32_t A,
                                       float entropy_coef, float *dmean, float *dscale,
                                       double *partial_ws, float *out3, void *stream) {
    PFRL_CHECK_ARG(M >= 1 && A >= 1 && A <= kMaxA, "pfrl_trpo_gaussian_eval: 1 <= A <= 32, M >= 1");
    PFRL_CHECK_ARG(mean && scale && mean_old && scale_old && action && adv && log_prob_old &&
                       partial_ws && out3,
                   "pfrl_trpo_gaussian_eval: null pointer");
    PFRL_CHECK_ARG((dmean == nullptr) == (dscale == nullptr),
                   "pfrl_trpo_gaussian_eval: dmean and dscale come together");
    const unsigned blocks = (unsigned)((M + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(k_trpo_gaussian_eval, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, mean,
                       scale, mean_old, action, adv, log_prob_old, M, A, dmean, partial_ws);
    hipLaunchKernelGGL(k_trpo_gaussian_finish, dim3(1), dim3(64), 0, (hipStream_t)stream, partial_ws,
                       (int)blocks, M, A, entropy_coef, scale, scale_old, out3, dscale);
    PFRL_LAUNCH_CHECK();
}

extern "C" int pfrl_cg_workgroup_reach(void) { return kOneWgReach; }

extern "C" int pfrl_cg_init(const float *b, float *x, float *r, float *p, double *state,
                            double *partial_ws, int64_t n, void *stream) {
    PFRL_CHECK_ARG(n >= 1 && n <= ((int64_t)1 << 40) && b && x && r && p && state && partial_ws,
                   "pfrl_cg_init: n >= 1, non-null pointers");
    const int nblk = chunks_of(n);
    hipLaunchKernelGGL(k_cg_init, dim3(nblk), dim3(kThreads), 0, (hipStream_t)stream, b, x, r, p, n,
                       partial_ws);
    hipLaunchKernelGGL(k_cg_init_finish, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, partial_ws, nblk,
                       state);
    PFRL_LAUNCH_CHECK();
}

extern "C" int pfrl_cg_step(float *x, float *r, float *p, const float *Ap, double *state,
                            double *partial_ws, int64_t n, float tol, void *stream) {
    PFRL_CHECK_ARG(n >= 1 && n <= ((int64_t)1 << 40) && x && r && p && Ap && state && partial_ws,
                   "pfrl_cg_step: n >= 1, non-null pointers");
    if (n <= kOneWgReach) {
        hipLaunchKernelGGL(k_cg_step_one, dim3(1), dim3(kOneWgThreads), 0, (hipStream_t)stream, x, r, p, Ap,
                           state, (int)n, tol);
        PFRL_LAUNCH_CHECK();
    }
    const int nblk = chunks_of(n);
    double *part_pAp = partial_ws, *part_rr = partial_ws + nblk;
    hipLaunchKernelGGL(k_cg_dot, dim3(nblk), dim3(kThreads), 0, (hipStream_t)stream, Ap, (const float *)p,
                       (const double *)state, n, part_pAp);
    hipLaunchKernelGGL(k_cg_update_xr, dim3(nblk), dim3(kThreads), 0, (hipStream_t)stream, x, r,
                       (const float *)p, Ap, (const double *)state, n, (const double *)part_pAp, nblk,
                       part_rr);
    hipLaunchKernelGGL(k_cg_update_p, dim3(nblk), dim3(kThreads), 0, (hipStream_t)stream, (const float *)r,
                       p, (const double *)state, n, (const double *)part_rr, nblk, tol);
    hipLaunchKernelGGL(k_cg_step_finish, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, state,
                       (const double *)part_pAp, (const double *)part_rr, nblk, tol);
    PFRL_LAUNCH_CHECK();
}

extern "C" int pfrl_trpo_scale_step(const float *d, const float *Fd, double max_kl, float *full_step,
                                    float *out_scale_dfd, double *partial_ws, int64_t n,
                                    void *stream) {
    PFRL_CHECK_ARG(n >= 1 && n <= ((int64_t)1 << 40) && d && Fd && full_step && out_scale_dfd && partial_ws,
                   "pfrl_trpo_scale_step: n >= 1, non-null pointers");
    const int nblk = chunks_of(n);
    hipLaunchKernelGGL(k_cg_dot, dim3(nblk), dim3(kThreads), 0, (hipStream_t)stream, d, Fd,
                       (const double *)nullptr, n, partial_ws);
    hipLaunchKernelGGL(k_trpo_scale_step, dim3(nblk), dim3(kThreads), 0, (hipStream_t)stream, d, n,
                       (const double *)partial_ws, nblk, max_kl, full_step, out_scale_dfd);
    PFRL_LAUNCH_CHECK();
}

extern "C" int pfrl_params_axpy(int32_t n_tensors, float *const *params, const int64_t *numel,
                                const float *base, const float *full_step, float step_size,
                                void *stream) {
    PFRL_CHECK_ARG(n_tensors >= 1 && n_tensors <= PFRL_OPT_MAX_TENSORS && params && numel && base &&
                       full_step,
                   "pfrl_params_axpy: 1 <= tensors <= 24, non-null pointers");
    AxpyArgs a;
    int chunks = 0;
    int64_t off = 0;
    for (int t = 0; t < n_tensors; ++t) {
        PFRL_CHECK_ARG(numel[t] >= 0 && params[t], "pfrl_params_axpy: null parameter tensor");
        a.p[t] = params[t];
        a.numel[t] = numel[t];
        a.offset[t] = off;
        off += numel[t];
        chunks += chunks_of(numel[t]);
        a.chunk_end[t] = chunks;
    }
    a.n = n_tensors;
    if (chunks == 0) return 0;
    hipLaunchKernelGGL(k_params_axpy, dim3(chunks), dim3(kThreads), 0, (hipStream_t)stream, a, base,
                       full_step, step_size);
    PFRL_LAUNCH_CHECK();
}
