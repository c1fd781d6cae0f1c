// REINFORCE (pfrl/agents/reinforce.py:176-195): the loss of the M stored steps of a batch of episodes
//   total = sum_m (-R_m log pi(a_m | s_m) - beta H_m) / batchsize
// and its gradient with respect to what the policy's last layer produced, in ONE launch + a
// one-workgroup finish, where the reference stacks M scalar losses and runs backward through M
// batch-1 graphs of torch.distributions.  R_m is the return column the host computed (float64 /
// int64 cumsum, cast to f32 once: -R * log_prob is an f32 product there, R a scalar).
// One thread per row; row = fl(fl(-R) lp_a) - fl(beta H), summed in f64 per wave (shuffles), per
// workgroup (LDS), then folded in block order by the finish kernel both entry points share.
// Row kernels bound by launch latency and one read of the logits: no MFMA.
#include <hip/hip_runtime.h>

#include "common.h"
#include "gaussian_rows.h"
#include "row_reduce.h"
#include "softmax_rows.h"

namespace {

constexpr int kThreads = 256;

// Categorical(logits): lp = log_softmax(z), H = -sum p lp (softmax_row), and by softmax_grad_row
//   dlogits_j = inv_b (-R (1[j = a] - p_j) + beta p_j (lp_j + H))
template <int A>
__global__ __launch_bounds__(kThreads) void k_reinforce_loss(
    const float *__restrict__ logits, const int64_t *__restrict__ action,
    const float *__restrict__ ret, int M, float inv_b, float beta, float *__restrict__ dlogits,
    double *__restrict__ partial) {
    __shared__ double s_red[2][kThreads / 64];
    const int m = blockIdx.x * kThreads + threadIdx.x;
    double loss = 0.0, ent = 0.0;
    if (m < M) {
        float z[A];
#pragma unroll
        for (int j = 0; j < A; ++j) z[j] = logits[(size_t)m * A + j];
        const int a = (int)action[m];
        float H, lpa, p[A], lp[A], g[A];
        softmax_row<A>(z, a, lp, p, H, lpa);
        const float neg_r = -ret[m];
        // (a NaN return reaches every entry of the row: NaN * 0 is NaN)
        softmax_grad_row<A>(inv_b * neg_r, beta * inv_b, a, p, lp, H, g);
#pragma unroll
        for (int j = 0; j < A; ++j) dlogits[(size_t)m * A + j] = g[j];
        loss = (double)(neg_r * lpa - beta * H);
        ent = (double)H;
    }
    loss = wave_sum_f64(loss);
    ent = wave_sum_f64(ent);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        s_red[0][wave] = loss;
        s_red[1][wave] = ent;
    }
    block_fold(s_red, 2, partial);
}

// Independent(Normal(mean, scale), 1) with a scale shared by all rows; log pi and the entropy as
// pfrl_ppo_gaussian_act computes them (gaussian_rows.h).  g = inv_b (-R) = d total / d log pi:
//   dmean_j = g (a_j - mu_j) / s_j^2,   d total / d scale_j = sum_m g ((a_j - mu_j)^2 / s_j^3 - 1 / s_j)
//                                                             - beta M inv_b / s_j    (finish)
__global__ __launch_bounds__(kThreads) void k_reinforce_gaussian_loss(
    const float *__restrict__ mean, const float *__restrict__ scale,
    const float *__restrict__ action, const float *__restrict__ ret, int M, int A, float inv_b,
    float beta, float *__restrict__ dmean, double *__restrict__ partial) {
    __shared__ double s_red[2 + kMaxA][kThreads / 64];
    const int m = blockIdx.x * kThreads + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool live = m < M;
    const size_t base = (size_t)(live ? m : 0) * A;
    double loss = 0.0, ent = 0.0;
    float g = 0.f;
    if (live) {
        const float lpa = row_log_prob(action + base, mean + base, scale, A);
        const float Hf = (float)gaussian_entropy(scale, A);
        const float neg_r = -ret[m];
        g = inv_b * neg_r;
        loss = (double)(neg_r * lpa - beta * Hf);
        ent = (double)Hf;
    }
    loss = wave_sum_f64(loss);
    ent = wave_sum_f64(ent);
    if (lane == 0) {
        s_red[0][wave] = loss;
        s_red[1][wave] = ent;
    }
    gaussian_grad_columns(live, g, action, mean, scale, base, A, dmean, s_red, 2);
    block_fold(s_red, 2 + A, partial);
}

// partial[nblk][2 + A] (A = 0 for the categorical kernel), folded in block order:
// out[0] = sum of the rows / batchsize, out[1] = mean entropy, dscale[j] (may be NULL)
__global__ __launch_bounds__(64) void k_reinforce_finish(const double *__restrict__ partial, int nblk,
                                                         int M, int A, float inv_b, float beta,
                                                         const float *__restrict__ scale,
                                                         float *__restrict__ out,
                                                         float *__restrict__ dscale) {
    const int lane = threadIdx.x;
    for (int k = 0; k < 2 + A; ++k) {
        const double s = fold_column(partial, nblk, 2 + A, k);
        if (lane != 0) continue;
        if (k == 0) out[0] = (float)(s * (double)inv_b);
        else if (k == 1) out[1] = (float)(s / M);
        else if (dscale != nullptr)
            dscale[k - 2] = (float)(s - (double)beta * (double)M * (double)inv_b / (double)scale[k - 2]);
    }
}

}  // namespace

extern "C" int pfrl_reinforce_loss(const float *logits, const int64_t *action, const float *ret,
                                   int32_t M, int32_t A, float inv_batchsize, float beta,
                                   float *dlogits, double *partial_ws, float *out2, void *stream) {
    PFRL_CHECK_ARG(M >= 1 && A >= 1 && A <= kMaxSoftmaxA, "pfrl_reinforce_loss: 1 <= A <= 31, M >= 1");
    PFRL_CHECK_ARG(logits && action && ret && dlogits && partial_ws && out2,
                   "pfrl_reinforce_loss: null pointer");
    const unsigned blocks = (unsigned)((M + kThreads - 1) / kThreads);
#define LOSS_CALL(AA)                                                                                \
    case AA:                                                                                         \
        hipLaunchKernelGGL(k_reinforce_loss<AA>, dim3(blocks), dim3(kThreads), 0,                    \
                           (hipStream_t)stream, logits, action, ret, M, inv_batchsize, beta, dlogits, \
                           partial_ws);                                                              \
        break;
    PFRL_SWITCH_SOFTMAX_A(A, LOSS_CALL)
#undef LOSS_CALL
    hipLaunchKernelGGL(k_reinforce_finish, dim3(1), dim3(64), 0, (hipStream_t)stream, partial_ws,
                       (int)blocks, M, 0, inv_batchsize, beta, (const float *)nullptr, out2,
                       (float *)nullptr);
    PFRL_LAUNCH_CHECK();
}

extern "C" int pfrl_reinforce_gaussian_loss(const float *mean, const float *scale, const float *action,
                                            const float *ret, int32_t M, int32_t A,
                                            float inv_batchsize, float beta, float *dmean,
                                            float *dscale, double *partial_ws, float *out2,
                                            void *stream) {
    PFRL_CHECK_ARG(M >= 1 && A >= 1 && A <= kMaxA,
                   "pfrl_reinforce_gaussian_loss: 1 <= A <= 32, M >= 1");
    PFRL_CHECK_ARG(mean && scale && action && ret && dmean && partial_ws && out2,
                   "pfrl_reinforce_gaussian_loss: null pointer");
    const unsigned blocks = (unsigned)((M + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(k_reinforce_gaussian_loss, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream,
                       mean, scale, action, ret, M, A, inv_batchsize, beta, dmean, partial_ws);
    hipLaunchKernelGGL(k_reinforce_finish, dim3(1), dim3(64), 0, (hipStream_t)stream, partial_ws,
                       (int)blocks, M, A, inv_batchsize, beta, scale, out2, dscale);
    PFRL_LAUNCH_CHECK();
}
