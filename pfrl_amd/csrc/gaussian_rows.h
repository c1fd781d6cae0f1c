// Row arithmetic of a diagonal Gaussian policy whose scale does not depend on the state, shared by
// the PPO launches (ppo_gaussian.hip), the TRPO evaluation (trpo.hip), REINFORCE (reinforce.hip) and
// A2C (a2c.hip): all four must produce the same log pi(a | s) bit for bit, because a ratio
// exp(log pi - log pi_old) of an unchanged policy has to be exactly 1, and the same entropy and
// gradient columns, so that a bound derived for one of them holds for the others.
#pragma once
#include <hip/hip_runtime.h>

#include "row_reduce.h"

namespace {

constexpr int kMaxA = 32;
// Normal.entropy(): 0.5 + 0.5 log(2 pi) + log(scale);  Normal.log_prob(): ... - log(sqrt(2 pi))
constexpr float kEntropyConst = 1.4189385332046727f;
constexpr float kLogSqrt2Pi = 0.9189385332046727f;

// One element of Normal(mu, s).log_prob(a) in torch's order of operations:
//   -((a - mu) ** 2) / (2 * s ** 2) - log(s) - log(sqrt(2 pi))
__device__ __forceinline__ float normal_log_prob(float a, float mu, float s, float log_s) {
    const float d = a - mu;
    const float var = s * s;
    return (-(d * d) / (2.f * var) - log_s) - kLogSqrt2Pi;
}

// The Independent sum over the action dimension in the order ATen's reduction kernel adds a
// contiguous innermost dimension of A <= 32 floats (ATen/native/cuda/Reduce.cuh): W = the largest
// power of two <= A lanes, lane t takes x[t] + x[t + W], then a shuffle-down tree over the W lanes
// (offsets 1, 2, 4, ...).  log pi(a|s) is ~1.2 A in magnitude and enters the loss through
// exp(log pi - log pi_old): with another order its last bit (4e-6 at A = 32) would be the largest
// difference between this kernel and the torch expression.
template <int W>
__device__ __forceinline__ float tree_sum_w(const float (&x)[kMaxA], int A) {
    float s[W];
#pragma unroll
    for (int t = 0; t < W; ++t) s[t] = (W < kMaxA && t + W < A) ? x[t] + x[(t + W) % kMaxA] : x[t];
#pragma unroll
    for (int off = 1; off < W; off <<= 1) {
#pragma unroll
        for (int i = 0; i + off < W; i += 2 * off) s[i] = s[i] + s[i + off];
    }
    return s[0];
}

__device__ __forceinline__ float tree_sum(const float (&x)[kMaxA], int A) {
    if (A >= 32) return tree_sum_w<32>(x, A);
    if (A >= 16) return tree_sum_w<16>(x, A);
    if (A >= 8) return tree_sum_w<8>(x, A);
    if (A >= 4) return tree_sum_w<4>(x, A);
    if (A >= 2) return tree_sum_w<2>(x, A);
    return x[0];
}

// log pi(act | s) of one row: the A terms, then their sum
__device__ __forceinline__ float row_log_prob(const float *__restrict__ act,
                                              const float *__restrict__ mean,
                                              const float *scale, int A) {
    float x[kMaxA];
#pragma unroll
    for (int j = 0; j < kMaxA; ++j) {
        const int jj = j < A ? j : 0;
        const float s = scale[jj];
        const float t = normal_log_prob(act[jj], mean[jj], s, logf(s));
        x[j] = j < A ? t : 0.f;
    }
    return tree_sum(x, A);
}

// Independent(Normal(mean, scale), 1).entropy() of any row: the A terms fl(c + log(s_j)), each one
// float32 as Normal.entropy() rounds it, added in index order in f64.  The caller rounds the sum to
// float32 where it stores or uses it.
__device__ __forceinline__ double gaussian_entropy(const float *scale, int A) {
    double H = 0.0;
    for (int j = 0; j < A; ++j) H += (double)(kEntropyConst + logf(scale[j]));
    return H;
}

// The gradient of g log pi(a | s) of one row (g = d loss / d log pi, 0 for a dead row) with
// respect to the mean, written, and its scale-gradient terms summed over the wave:
//   dmean_j = fl(g fl(d / fl(s s))),  d = fl(a_j - mu_j)                              (float32)
//   t_j = g (fl(d d) / s^3 - 1 / s)  (f64 on the float32 operands), wave sum -> s_red[first_row + j]
// A is uniform: every lane of every wave takes part in the shuffles, dead rows add zero.
template <int ROWS, int WAVES>
__device__ __forceinline__ void gaussian_grad_columns(bool live, float g,
                                                      const float *action,
                                                      const float *mean,
                                                      const float *scale, size_t base,
                                                      int A, float *dmean,
                                                      double (&s_red)[ROWS][WAVES], int first_row) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int j = 0; j < A; ++j) {
        double t = 0.0;
        if (live) {
            const float s = scale[j];
            const float d = action[base + j] - mean[base + j];
            dmean[base + j] = g * (d / (s * s));
            t = (double)g * ((double)(d * d) / ((double)s * (double)s * (double)s) - 1.0 / (double)s);
        }
        t = wave_sum_f64(t);
        if (lane == 0) s_red[first_row + j][wave] = t;
    }
}

}  // namespace
