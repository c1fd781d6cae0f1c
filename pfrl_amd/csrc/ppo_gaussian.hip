// PPO with a diagonal Gaussian policy whose scale does not depend on the state
// (pfrl/policies/gaussian_policy.py: GaussianHeadWithStateIndependentCovariance,
// GaussianHeadWithFixedCovariance; examples/mujoco/reproduction/ppo/train_ppo.py): sampling,
// entropy and log-probability behind the network (pfrl/agents/ppo.py:759-778, :110-142), the loss of
// a minibatch with its gradient (:634-671), and the minibatch assembly with a float action column
// (:483-511).  Minibatches there are 64 rows of a few numbers: every launch here is latency, so each
// of the three is ONE launch (+ the one-workgroup finish of the loss) that a captured graph replays.
// One thread per row, the action dimension A <= 32 a run-time loop; sums over the batch are f64 per
// wave (shuffles), per workgroup (LDS), then folded in block order by the finish kernel.
#include <hip/hip_runtime.h>

#include "common.h"
#include "gaussian_rows.h"
#include "ppo_rows.h"

namespace {

constexpr int kThreads = 256;

// z != NULL: action = fl(fl(z scale) + mean) -- torch.normal(mean, std) on the device is
// normal_(0, 1).mul_(std).add_(mean): two roundings, never an fma -- and the row's entropy.
// given != NULL: log pi(given | s), the Independent(Normal) sum over the action dimension.
__global__ __launch_bounds__(kThreads) void k_ppo_gaussian_act(
    const float *__restrict__ mean, const float *__restrict__ scale, const float *__restrict__ z,
    const float *__restrict__ given, float *__restrict__ action, float *__restrict__ entropy,
    float *__restrict__ log_prob, int N, int A) {
    const int row = blockIdx.x * kThreads + threadIdx.x;
    if (row >= N) return;
    const size_t base = (size_t)row * A;
    if (z != nullptr) {
        for (int j = 0; j < A; ++j)
            action[base + j] = __fadd_rn(__fmul_rn(z[base + j], scale[j]), mean[base + j]);
        if (entropy != nullptr) entropy[row] = (float)gaussian_entropy(scale, A);
    }
    if (given != nullptr) {
        log_prob[row] = row_log_prob(given + base, mean + base, scale, A);
    }
}

// PPO._lossfun on (mean, scale, value) of a minibatch and its gradient with respect to all three.
//   d log pi / d mean_j  = (a_j - mu_j) / s_j^2
//   d log pi / d scale_j = (a_j - mu_j)^2 / s_j^3 - 1 / s_j
//   d H / d scale_j      = 1 / s_j                       (H does not depend on the row)
// partial[block][3 + A]: (-surrogate, value loss, entropy) and the A row sums of
// g_lpa * d log pi / d scale_j, where g_lpa = d loss / d log pi of the row (1 / M included).
__global__ __launch_bounds__(kThreads) void k_ppo_gaussian_loss(
    const float *__restrict__ mean, const float *__restrict__ scale, const float *__restrict__ value,
    const float *__restrict__ action, const float *__restrict__ adv,
    const float *__restrict__ logp_old, const float *__restrict__ v_old,
    const float *__restrict__ v_teacher, int M, int A, float clip_eps, float clip_eps_vf,
    float vf_coef, float *__restrict__ dmean, float *__restrict__ dvalue,
    double *__restrict__ partial) {
    __shared__ double s_red[3 + kMaxA][kThreads / 64];
    const int m = blockIdx.x * kThreads + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool live = m < M;
    const size_t base = (size_t)(live ? m : 0) * A;
    const float inv_m = 1.0f / (float)M;
    double pol = 0.0, val = 0.0, ent = 0.0;
    float g_lpa = 0.f;
    if (live) {
        const float lpa = row_log_prob(action + base, mean + base, scale, A);
        const double H = gaussian_entropy(scale, A);
        float surr;
        ppo_surrogate_row(lpa, logp_old[m], adv[m], inv_m, clip_eps, surr, g_lpa);
        float lv, gv;
        ppo_value_row(value[m], clip_eps_vf >= 0.f ? v_old[m] : 0.f, v_teacher[m], clip_eps_vf, lv, gv);
        dvalue[m] = vf_coef * inv_m * gv;
        pol = -(double)surr;
        val = (double)lv;
        ent = (double)(float)H;
    }
    pol = wave_sum_f64(pol);
    val = wave_sum_f64(val);
    ent = wave_sum_f64(ent);
    if (lane == 0) {
        s_red[0][wave] = pol;
        s_red[1][wave] = val;
        s_red[2][wave] = ent;
    }
    gaussian_grad_columns(live, g_lpa, action, mean, scale, base, A, dmean, s_red, 3);
    block_fold(s_red, 3 + A, partial);
}

// out[0] = loss, out[1] = loss_policy, out[2] = loss_value, out[3] = mean entropy
// (ppo_total_loss, as the categorical finish); dscale[j] = sum over rows - entropy_coef / scale_j
__global__ __launch_bounds__(64) void k_ppo_gaussian_finish(
    const double *__restrict__ partial, int nblk, int M, int A, float vf_coef, float ent_coef,
    const float *__restrict__ scale, float *__restrict__ out, float *__restrict__ dscale) {
    const int lane = threadIdx.x;
    float head[3] = {0.f, 0.f, 0.f};
    for (int k = 0; k < 3 + A; ++k) {
        const double s = fold_column(partial, nblk, 3 + A, k);
        if (k < 3) head[k] = (float)(s / M);
        else if (lane == 0 && dscale != nullptr)
            dscale[k - 3] = (float)(s - (double)ent_coef / (double)scale[k - 3]);
    }
    if (lane == 0) {
        out[1] = head[0];
        out[2] = head[1];
        out[3] = head[2];
        out[0] = ppo_total_loss(head[0], head[1], head[2], vf_coef, ent_coef);
    }
}

// k_ppo_minibatch (rollout.hip) with an action column of A floats per position
__global__ __launch_bounds__(kThreads) void k_ppo_minibatch_f32act(
    int64_t M, const int64_t *__restrict__ idx, const float *__restrict__ adv,
    const float *__restrict__ mean_std, int standardize, const float *__restrict__ log_prob,
    const float *__restrict__ v_pred, const float *__restrict__ v_teacher,
    const float *__restrict__ action, int32_t A, const int32_t *__restrict__ state_refs, int32_t k,
    float *__restrict__ out_adv, float *__restrict__ out_logp, float *__restrict__ out_v,
    float *__restrict__ out_vt, float *__restrict__ out_action, int32_t *__restrict__ out_refs) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= M) return;
    const int64_t p = idx[i];
    float a = adv[p];
    if (standardize) {
        // ppo.py:494-495  (advs - mean_advs) / (std_advs + 1e-8)
        const float den = __fadd_rn(mean_std[1], 1e-8f);
        a = __fdiv_rn(__fsub_rn(a, mean_std[0]), den);
    }
    out_adv[i] = a;
    out_logp[i] = log_prob[p];
    out_v[i] = v_pred[p];
    out_vt[i] = v_teacher[p];
    for (int j = 0; j < A; ++j) out_action[i * A + j] = action[p * A + j];
    for (int j = 0; j < k; ++j) out_refs[i * k + j] = state_refs[p * k + j];
}

}  // namespace

extern "C" int pfrl_ppo_gaussian_act(const float *mean, const float *scale, const float *z,
                                     const float *given_action, float *out_action,
                                     float *out_entropy, float *out_log_prob, int32_t N, int32_t A,
                                     void *stream) {
    PFRL_CHECK_ARG(N >= 0 && A >= 1 && A <= kMaxA, "pfrl_ppo_gaussian_act: 1 <= A <= 32");
    PFRL_CHECK_ARG(mean && scale && (z || given_action), "pfrl_ppo_gaussian_act: null pointer");
    PFRL_CHECK_ARG(!z || out_action, "pfrl_ppo_gaussian_act: sampling needs out_action");
    PFRL_CHECK_ARG(!given_action || out_log_prob, "pfrl_ppo_gaussian_act: given_action needs out_log_prob");
    if (N == 0) return 0;
    const unsigned blocks = (unsigned)((N + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(k_ppo_gaussian_act, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, mean,
                       scale, z, given_action, out_action, out_entropy, out_log_prob, N, A);
    PFRL_LAUNCH_CHECK();
}

extern "C" int pfrl_ppo_gaussian_loss(const float *mean, const float *scale, const float *value,
                                      const float *action, const float *adv,
                                      const float *log_prob_old, const float *v_pred_old,
                                      const float *v_teacher, int32_t M, int32_t A, float clip_eps,
                                      float clip_eps_vf, float value_func_coef, float entropy_coef,
                                      float *dmean, float *dvalue, float *dscale, double *partial_ws,
                                      float *out4, void *stream) {
    PFRL_CHECK_ARG(M >= 1 && A >= 1 && A <= kMaxA, "pfrl_ppo_gaussian_loss: 1 <= A <= 32, M >= 1");
    PFRL_CHECK_ARG(mean && scale && value && action && adv && log_prob_old && v_teacher && dmean &&
                       dvalue && partial_ws && out4 && (clip_eps_vf < 0.f || v_pred_old),
                   "pfrl_ppo_gaussian_loss: null pointer");
    const unsigned blocks = (unsigned)((M + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(k_ppo_gaussian_loss, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, mean,
                       scale, value, action, adv, log_prob_old, v_pred_old, v_teacher, M, A, clip_eps,
                       clip_eps_vf, value_func_coef, dmean, dvalue, partial_ws);
    hipLaunchKernelGGL(k_ppo_gaussian_finish, dim3(1), dim3(64), 0, (hipStream_t)stream, partial_ws,
                       (int)blocks, M, A, value_func_coef, entropy_coef, scale, out4, dscale);
    PFRL_LAUNCH_CHECK();
}

extern "C" int pfrl_ppo_minibatch_f32act(int64_t M, const int64_t *idx, const float *adv,
                                         const float *mean_std, int standardize,
                                         const float *log_prob, const float *v_pred,
                                         const float *v_teacher, const float *action, int32_t A,
                                         const int32_t *state_refs, int32_t k, float *out_adv,
                                         float *out_logp, float *out_v, float *out_vt,
                                         float *out_action, int32_t *out_refs, void *stream) {
    PFRL_CHECK_ARG(A >= 1 && k >= 0, "pfrl_ppo_minibatch_f32act: A >= 1");
    if (M <= 0) return 0;
    const unsigned blocks = (unsigned)((M + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(k_ppo_minibatch_f32act, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, M,
                       idx, adv, mean_std, standardize, log_prob, v_pred, v_teacher, action, A,
                       state_refs, k, out_adv, out_logp, out_v, out_vt, out_action, out_refs);
    PFRL_LAUNCH_CHECK();
}
