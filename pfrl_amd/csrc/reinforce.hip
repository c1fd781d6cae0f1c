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

namespace {

constexpr int kThreads = 256;
constexpr int kMaxSoftmaxA = 31;

// writes the workgroup's 2 + extra sums: partial[block][2 + extra]
template <int ROWS>
__device__ __forceinline__ void block_fold(double (&s_red)[ROWS][kThreads / 64], int n,
                                           double *__restrict__ partial) {
    __syncthreads();
    if ((int)threadIdx.x < n) {
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < kThreads / 64; ++w) t += s_red[threadIdx.x][w];
        partial[(size_t)blockIdx.x * n + threadIdx.x] = t;
    }
}

// Categorical(logits): lp = log_softmax(z), H = -sum p lp (the row arithmetic of k_ppo_loss),
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
        float mx = z[0];
#pragma unroll
        for (int j = 1; j < A; ++j) mx = fmaxf(mx, z[j]);
        float e[A], sum = 0.f;
#pragma unroll
        for (int j = 0; j < A; ++j) {
            e[j] = expf(z[j] - mx);
            sum += e[j];
        }
        const float lse = mx + logf(sum);
        float H = 0.f, lpa = 0.f, p[A], lp[A];
#pragma unroll
        for (int j = 0; j < A; ++j) {
            lp[j] = z[j] - lse;
            p[j] = e[j] / sum;
            H -= p[j] > 0.f ? p[j] * lp[j] : 0.f;
            if (j == a) lpa = lp[j];
        }
        const float neg_r = -ret[m];
        // (a NaN return reaches every entry of the row: NaN * 0 is NaN)
        const float gl = inv_b * neg_r, ge = beta * inv_b;
#pragma unroll
        for (int j = 0; j < A; ++j) {
            const float onehot = j == a ? 1.f : 0.f;
            float gj = gl * (onehot - p[j]);
            gj += p[j] > 0.f ? ge * p[j] * (lp[j] + H) : 0.f;
            dlogits[(size_t)m * A + j] = gj;
        }
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
        double H = 0.0;
        for (int j = 0; j < A; ++j) H += (double)(kEntropyConst + logf(scale[j]));
        const float Hf = (float)H;
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
    // (A is uniform: every lane of every wave takes part in the shuffles, dead rows add zero)
    for (int j = 0; j < A; ++j) {
        double t = 0.0;
        if (live) {
            const float s = scale[j];
            const float d = action[base + j] - mean[base + j];
            dmean[base + j] = g * (d / (s * s));
            t = (double)g * ((double)(d * d) / ((double)s * (double)s * (double)s) - 1.0 / (double)s);
        }
        t = wave_sum_f64(t);
        if (lane == 0) s_red[2 + j][wave] = t;
    }
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
        double s = 0.0;
        for (int b = lane; b < nblk; b += 64) s += partial[(size_t)b * (2 + A) + k];
        s = wave_sum_f64(s);
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
    switch (A) {
        LOSS_CALL(1) LOSS_CALL(2) LOSS_CALL(3) LOSS_CALL(4) LOSS_CALL(5) LOSS_CALL(6) LOSS_CALL(7)
        LOSS_CALL(8) LOSS_CALL(9) LOSS_CALL(10) LOSS_CALL(11) LOSS_CALL(12) LOSS_CALL(13) LOSS_CALL(14)
        LOSS_CALL(15) LOSS_CALL(16) LOSS_CALL(17) LOSS_CALL(18) LOSS_CALL(19) LOSS_CALL(20)
        LOSS_CALL(21) LOSS_CALL(22) LOSS_CALL(23) LOSS_CALL(24) LOSS_CALL(25) LOSS_CALL(26)
        LOSS_CALL(27) LOSS_CALL(28) LOSS_CALL(29) LOSS_CALL(30) LOSS_CALL(31)
    }
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
