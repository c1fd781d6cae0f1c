// Row arithmetic of a diagonal Gaussian policy whose scale does not depend on the state, shared by
// the PPO launches (ppo_gaussian.hip) and the TRPO evaluation (trpo.hip): both must produce the same
// log pi(a | s) bit for bit, because a ratio exp(log pi - log pi_old) of an unchanged policy has to
// be exactly 1.
#pragma once
#include <hip/hip_runtime.h>

namespace {

constexpr int kMaxA = 32;
// Normal.entropy(): 0.5 + 0.5 log(2 pi) + log(scale);  Normal.log_prob(): ... - log(sqrt(2 pi))
constexpr float kEntropyConst = 1.4189385332046727f;
constexpr float kLogSqrt2Pi = 0.9189385332046727f;

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

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
                                              const float *__restrict__ scale, int A) {
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

}  // namespace
