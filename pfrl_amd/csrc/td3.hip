// TD3 / DDPG update helpers for gfx950: what sits between the network outputs and backward() in
// pfrl/agents/td3.py:191-211, 238-242 and pfrl/agents/ddpg.py:158-168, 179-182 as single launches.
//
//   target-policy smoothing   clamp(a + clamp(sigma * noise, -c, c), lo, hi) (td3.py:22-25): the four
//                             elementwise launches behind the draw -> 1, in place on the draw
//   critic target and loss    t = r + d (1 - terminal) min(nq1, nq2), mean((t - pred_k)^2) for one or
//                             two critics and the gradients for dL/dloss = 1: ~5 + 2 x 7 launches -> 1
//   actor loss                -mean(q) and its gradient: 2 + 3 launches -> 1
//
// B is the minibatch (100 .. 256): the cost is the launch, not the arithmetic (as for the SAC losses
// of actor.hip, whose layout these follow: 256 threads, one workgroup per reduction, lane-strided
// partial sums, wave butterfly, four-way fold -- one fixed order, the same bits on every launch).
// Every arithmetic step is one rounded f32 operation in the order of the PyTorch expression it
// replaces (built with -ffp-contract=off).
#include "common.h"
#include "row_reduce.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxB = 65536;

// torch.clamp: min(max(x, lo), hi), a NaN passes through
__device__ __forceinline__ float torch_clamp(float x, float lo, float hi) {
    float c = x < lo ? lo : x;
    c = c > hi ? hi : c;
    return c;
}

// out may be noise: every thread reads its own element of both inputs before it writes
__global__ __launch_bounds__(kThreads) void k_td3_smooth_action(const float *action, const float *noise,
                                                                float sigma, float noise_clip, float low,
                                                                float high, float *out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const float e = torch_clamp(sigma * noise[i], -noise_clip, noise_clip);
    out[i] = torch_clamp(action[i] + e, low, high);
}

// pointer pairs by value (as HalfMseArgs of actor.hip): nothing on the host has to outlive the call,
// so the launches capture into a HIP graph
struct CriticArgs {
    const float *next_q[2], *pred[2], *g_loss[2];
    float *loss[2], *g_pred[2];
};

// blockIdx.y picks the critic; each workgroup recomputes the target (the same operations on the same
// operands: the same bits), workgroup 0 stores it.  g_pred given: the gradient for dL/dloss = 1, the
// arithmetic of k_td3_critic_loss_bwd at g = 1.
__global__ __launch_bounds__(kThreads) void k_td3_critic_loss(
    const float *__restrict__ reward, const float *__restrict__ discount, float gamma,
    const float *__restrict__ terminal, CriticArgs a, int n_q, float *__restrict__ target_q, int B) {
    __shared__ float sh[4];
    const int k = blockIdx.y;
    const float *__restrict__ pred = a.pred[k];
    float *__restrict__ unit = a.g_pred[k];
    float *__restrict__ tq = k == 0 ? target_q : nullptr;
    const float inv_b = 1.0f / (float)B;
    float s = 0.f;
    for (int i = threadIdx.x; i < B; i += kThreads) {
        const float nq = n_q == 2 ? torch_min(a.next_q[0][i], a.next_q[1][i]) : a.next_q[0][i];
        const float d = discount != nullptr ? discount[i] : gamma;
        const float t = reward[i] + (d * (1.0f - terminal[i])) * nq;
        if (tq != nullptr) tq[i] = t;
        const float diff = t - pred[i];
        s += diff * diff;
        if (unit != nullptr) unit[i] = -((2.0f * diff) * inv_b);
    }
    s = block_sum(s, sh);
    if (threadIdx.x == 0) a.loss[k][0] = s / (float)B;
}

// d mean((t - pred)^2) / d pred_i = -2 (t_i - pred_i) / B, times the upstream scalar: the unit
// gradient scaled by g in one more rounding (g = 1: the unit gradient's bits)
__global__ __launch_bounds__(kThreads) void k_td3_critic_loss_bwd(const float *__restrict__ target_q,
                                                                  CriticArgs a, int B) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= B) return;
    const int k = blockIdx.y;
    const float *g_loss = a.g_loss[k];
    if (g_loss == nullptr) {
        a.g_pred[k][i] = 0.f;
        return;
    }
    const float inv_b = 1.0f / (float)B;
    a.g_pred[k][i] = -(g_loss[0] * ((2.0f * (target_q[i] - a.pred[k][i])) * inv_b));
}

__global__ __launch_bounds__(kThreads) void k_neg_mean(const float *__restrict__ q, float *__restrict__ loss,
                                                       float *__restrict__ unit, int B) {
    __shared__ float sh[4];
    const float g = -(1.0f / (float)B);
    float s = 0.f;
    for (int i = threadIdx.x; i < B; i += kThreads) {
        s += q[i];
        if (unit != nullptr) unit[i] = g;
    }
    s = block_sum(s, sh);
    if (threadIdx.x == 0) loss[0] = -(s / (float)B);
}

}  // namespace

extern "C" int pfrl_td3_smooth_action(const float *action, const float *noise, float sigma,
                                      float noise_clip, float low, float high, float *out, int64_t n,
                                      void *stream) {
    // (written so that a NaN bound fails its comparison)
    PFRL_CHECK_ARG(n >= 1 && n <= (int64_t)0x7fffffff * kThreads && sigma >= 0.f && noise_clip >= 0.f &&
                       low <= high,
                   "pfrl_td3_smooth_action: n >= 1, sigma >= 0, noise_clip >= 0, low <= high");
    PFRL_CHECK_ARG(action && noise && out, "pfrl_td3_smooth_action: null pointer");
    hipLaunchKernelGGL(k_td3_smooth_action, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads),
                       0, (hipStream_t)stream, action, noise, sigma, noise_clip, low, high, out, n);
    PFRL_LAUNCH_CHECK();
}

extern "C" int pfrl_td3_critic_loss(const float *reward, const float *discount, float gamma,
                                    const float *terminal, const float *const *next_q,
                                    const float *const *pred, int32_t n_q, float *target_q,
                                    float *const *loss, float *const *unit_g_pred, int32_t B,
                                    void *stream) {
    PFRL_CHECK_ARG(B >= 1 && B <= kMaxB && (n_q == 1 || n_q == 2),
                   "pfrl_td3_critic_loss: 1 <= B <= 65536, n_q 1 or 2");
    PFRL_CHECK_ARG(reward && terminal && next_q && pred && loss, "pfrl_td3_critic_loss: null pointer");
    CriticArgs a{};
    for (int k = 0; k < n_q; ++k) {
        PFRL_CHECK_ARG(next_q[k] && pred[k] && loss[k], "pfrl_td3_critic_loss: null pointer");
        a.next_q[k] = next_q[k];
        a.pred[k] = pred[k];
        a.loss[k] = loss[k];
        a.g_pred[k] = unit_g_pred != nullptr ? unit_g_pred[k] : nullptr;
    }
    hipLaunchKernelGGL(k_td3_critic_loss, dim3(1, n_q), dim3(kThreads), 0, (hipStream_t)stream, reward,
                       discount, gamma, terminal, a, (int)n_q, target_q, (int)B);
    PFRL_LAUNCH_CHECK();
}

extern "C" int pfrl_td3_critic_loss_bwd(const float *const *g_loss, const float *target_q,
                                        const float *const *pred, float *const *g_pred, int32_t n_q,
                                        int32_t B, void *stream) {
    PFRL_CHECK_ARG(B >= 1 && B <= kMaxB && (n_q == 1 || n_q == 2),
                   "pfrl_td3_critic_loss_bwd: 1 <= B <= 65536, n_q 1 or 2");
    PFRL_CHECK_ARG(g_loss && target_q && pred && g_pred, "pfrl_td3_critic_loss_bwd: null pointer");
    CriticArgs a{};
    for (int k = 0; k < n_q; ++k) {
        PFRL_CHECK_ARG(pred[k] && g_pred[k], "pfrl_td3_critic_loss_bwd: null pointer");
        a.pred[k] = pred[k];
        a.g_loss[k] = g_loss[k];
        a.g_pred[k] = g_pred[k];
    }
    hipLaunchKernelGGL(k_td3_critic_loss_bwd, dim3((B + kThreads - 1) / kThreads, n_q), dim3(kThreads), 0,
                       (hipStream_t)stream, target_q, a, (int)B);
    PFRL_LAUNCH_CHECK();
}

extern "C" int pfrl_neg_mean(const float *q, float *loss, float *unit_g_q, int32_t B, void *stream) {
    PFRL_CHECK_ARG(B >= 1 && B <= kMaxB && q && loss, "pfrl_neg_mean: 1 <= B <= 65536, no null pointer");
    hipLaunchKernelGGL(k_neg_mean, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, q, loss, unit_g_q, (int)B);
    PFRL_LAUNCH_CHECK();
}
