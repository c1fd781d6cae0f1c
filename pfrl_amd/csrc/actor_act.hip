// The acting step of the continuous replay agents for gfx950: the policy's last nn.Linear and
// everything behind it as ONE launch per batched env step.
//
//   SAC          x = h w^T + b, (mean | log_scale) = chunk(x), a = tanh(mean + eps * scale) -- or
//                tanh(mean), the mode -- of the example head (pfrl/agents/soft_actor_critic.py:317-334
//                with examples/mujoco/reproduction/soft_actor_critic/train_soft_actor_critic.py:128-141):
//                linear + chunk / clamp / mul / exp / sqrt / normal / tanh -> 1
//   TD3 / DDPG   y = h w^T + b, g = tanh(y) * scale + shift (BoundByTanh), a = clip(g + noise, low, high)
//                with the explorer's noise rows from the host (pfrl/agents/td3.py:262-281,
//                pfrl/explorers/additive_gaussian.py:26-36, additive_ou.py:49-66)
//
// M is the number of envs (1 .. a few hundred), K a hidden width, the output a few dozen columns: a
// launch is a handful of dependent memory round trips and nothing else, so the mapping is chosen for
// time to first result.  One workgroup per row; each of its four waves owns every fourth output
// column and takes the whole reduction of a column: the row of h once into registers (K / 64 values
// per lane), then per column one batch of independent loads of w, K / 64 FMAs per lane and a
// butterfly over the wave.  No LDS traffic inside the reduction and no barrier before the one in
// front of the epilogue; the order of the sum over K is fixed by K alone (k = lane + 64 u, u
// ascending, then the xor butterfly 32, 16, .. 1), so a row's result is a function of that row.
// Everything behind the product is one rounded f32 operation per source operation
// (-ffp-contract=off), in the order of the torch / NumPy code it replaces.
#include "common.h"
#include "squashed_row.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxA = 32;            // action width
constexpr int kMaxK = 1024;          // hidden width
constexpr int kMaxM = 4096;          // envs
constexpr int kKU = kMaxK / 64;      // k values per lane

// Lane's share of a K-vector: v[u] = p[lane + 64 u], 0 past K.  Loads in uniform groups of four on
// clamped addresses (a load inside its own branch gets its own wait and the batch serialises).
__device__ __forceinline__ void load_k(const float *__restrict__ p, const int K, const int nk, const int lane,
                                       float (&v)[kKU]) {
#pragma unroll
    for (int g = 0; g < kKU / 4; ++g) {
        if (4 * g < nk) {   // (uniform)
            float t[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int k = lane + 64 * (4 * g + q);
                t[q] = p[k < K ? k : K - 1];
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) v[4 * g + q] = (lane + 64 * (4 * g + q)) < K ? t[q] : 0.f;
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) v[4 * g + q] = 0.f;
        }
    }
}

// xrow[n] = sum_k h_row[k] w[n][k] + bias[n] for n < n_out (LDS, valid after the caller's barrier)
__device__ __forceinline__ void head_row_linear(const float *__restrict__ h_row, const float *__restrict__ w,
                                                const float *__restrict__ bias, const int K, const int n_out,
                                                float *xrow) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nk = (K + 63) >> 6;
    float hv[kKU];
    load_k(h_row, K, nk, lane, hv);
    for (int n = wave; n < n_out; n += kWaves) {
        float wv[kKU];
        load_k(w + (size_t)n * K, K, nk, lane, wv);
        const float b = bias[n];
        float acc = 0.f;
#pragma unroll
        for (int g = 0; g < kKU / 4; ++g)
            if (4 * g < nk) {
#pragma unroll
                for (int q = 0; q < 4; ++q) acc = fmaf(hv[4 * g + q], wv[4 * g + q], acc);
            }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
        if (lane == 0) xrow[n] = acc + b;
    }
}

template <int MODE>
__global__ __launch_bounds__(kThreads) void k_squashed_head_act(
    const float *__restrict__ h, const float *__restrict__ w, const float *__restrict__ bias, float lo, float hi,
    const float *__restrict__ eps, float *__restrict__ x_out, float *__restrict__ action, int K, int A) {
    __shared__ float xrow[2 * kMaxA];
    const int m = blockIdx.x, tid = threadIdx.x;
    // (requested before the row product: nothing waits for it until the epilogue)
    const float e = (eps != nullptr && tid < A) ? eps[(size_t)m * A + tid] : 0.f;
    head_row_linear(h + (size_t)m * K, w, bias, K, 2 * A, xrow);
    __syncthreads();
    if (x_out != nullptr && tid < 2 * A) x_out[(size_t)m * 2 * A + tid] = xrow[tid];
    if (tid < A) {
        float s, u;
        action[(size_t)m * A + tid] =
            squashed_head_action<MODE>(xrow[tid], xrow[A + tid], lo, hi, eps != nullptr, e, s, u);
    }
}

__global__ __launch_bounds__(kThreads) void k_deterministic_head_act(
    const float *__restrict__ h, const float *__restrict__ w, const float *__restrict__ bias,
    const float *__restrict__ bound_scale, const float *__restrict__ bound_shift,
    const float *__restrict__ noise, const float *__restrict__ low, const float *__restrict__ high,
    float *__restrict__ y_out, float *__restrict__ greedy_out, float *__restrict__ action, int K, int A) {
    __shared__ float yrow[kMaxA];
    const int m = blockIdx.x, tid = threadIdx.x;
    const bool mine = tid < A;
    const float bs = (bound_scale != nullptr && mine) ? bound_scale[tid] : 1.f;
    const float sh = (bound_scale != nullptr && mine) ? bound_shift[tid] : 0.f;
    const float nz = (noise != nullptr && mine) ? noise[(size_t)m * A + tid] : 0.f;
    const float lo = (noise != nullptr && mine) ? low[tid] : 0.f;
    const float hi = (noise != nullptr && mine) ? high[tid] : 0.f;
    head_row_linear(h + (size_t)m * K, w, bias, K, A, yrow);
    __syncthreads();
    if (!mine) return;
    const size_t i = (size_t)m * A + tid;
    const float y = yrow[tid];
    if (y_out != nullptr) y_out[i] = y;
    // BoundByTanh: torch.tanh(x) * ((high - low) / 2) + (high + low) / 2, the two vectors as uploaded
    const float g = bound_scale != nullptr ? tanhf(y) * bs + sh : y;
    if (greedy_out != nullptr) greedy_out[i] = g;
    float a = g;
    if (noise != nullptr) {
        // a + noise, then np.clip = minimum(maximum(t, low), high): a NaN passes through
        float t = g + nz;
        t = t < lo ? lo : t;
        t = t > hi ? hi : t;
        a = t;
    }
    action[i] = a;
}

bool act_gates(int32_t M, int32_t K, int32_t A) {
    return A >= 1 && A <= kMaxA && K >= 1 && K <= kMaxK && M >= 0 && M <= kMaxM;
}

}  // namespace

extern "C" int pfrl_squashed_head_act(const float *h, const float *w, const float *bias, float clamp_lo,
                                      float clamp_hi, int32_t mode, const float *eps, float *x_out,
                                      float *action, int32_t M, int32_t K, int32_t A, void *stream) {
    PFRL_CHECK_ARG(act_gates(M, K, A), "pfrl_squashed_head_act: 1 <= A <= 32, 1 <= K <= 1024, 0 <= M <= 4096");
    PFRL_CHECK_ARG((mode == 0 || mode == 1) && clamp_lo <= clamp_hi, "pfrl_squashed_head_act: bad head");
    PFRL_CHECK_ARG(h != nullptr && w != nullptr && bias != nullptr && action != nullptr,
                   "pfrl_squashed_head_act: null argument");
    if (M == 0) return 0;
    if (mode == 0)
        hipLaunchKernelGGL(k_squashed_head_act<0>, dim3(M), dim3(kThreads), 0, (hipStream_t)stream, h, w, bias,
                           clamp_lo, clamp_hi, eps, x_out, action, K, A);
    else
        hipLaunchKernelGGL(k_squashed_head_act<1>, dim3(M), dim3(kThreads), 0, (hipStream_t)stream, h, w, bias,
                           clamp_lo, clamp_hi, eps, x_out, action, K, A);
    PFRL_LAUNCH_CHECK();
}

extern "C" int pfrl_deterministic_head_act(const float *h, const float *w, const float *bias,
                                           const float *bound_scale, const float *bound_shift,
                                           const float *noise, const float *low, const float *high,
                                           float *y_out, float *greedy_out, float *action, int32_t M,
                                           int32_t K, int32_t A, void *stream) {
    PFRL_CHECK_ARG(act_gates(M, K, A), "pfrl_deterministic_head_act: 1 <= A <= 32, 1 <= K <= 1024, 0 <= M <= 4096");
    PFRL_CHECK_ARG(h != nullptr && w != nullptr && bias != nullptr && action != nullptr,
                   "pfrl_deterministic_head_act: null argument");
    PFRL_CHECK_ARG((bound_scale == nullptr) == (bound_shift == nullptr),
                   "pfrl_deterministic_head_act: both bound vectors or neither");
    PFRL_CHECK_ARG(noise == nullptr || (low != nullptr && high != nullptr),
                   "pfrl_deterministic_head_act: noise needs low and high");
    if (M == 0) return 0;
    hipLaunchKernelGGL(k_deterministic_head_act, dim3(M), dim3(kThreads), 0, (hipStream_t)stream, h, w, bias,
                       bound_scale, bound_shift, noise, low, high, y_out, greedy_out, action, K, A);
    PFRL_LAUNCH_CHECK();
}
