// A2C (pfrl/agents/a2c.py:169-213): the three loss terms of one update over the M = T N stored steps
//   value_loss = mean adv^2,  action_loss = -mean(adv log pi(a | s)),  entropy = mean H,   adv = R - v
// and the gradient of  v_coef value_loss + pi_coef action_loss - ent_coef entropy  with respect to
// what the policy's last layer and the value layer produced (adv is a constant in the action loss, as
// the reference's advantages.detach() makes it), in ONE launch + a one-workgroup finish that also
// advances the agent's three moving statistics.  The reference runs ~25 torch kernels for the
// expression, its statistics and their backward.
// One thread per row; the row arithmetic is float32 in the order written here, the three sums are f64
// per wave (shuffles), per workgroup (LDS), then folded in block order by the finish kernel both
// entry points share.  Row kernels bound by launch latency and one read of the logits: no MFMA.
#include <hip/hip_runtime.h>

#include "common.h"
#include "gaussian_rows.h"
#include "row_reduce.h"
#include "softmax_rows.h"

namespace {

constexpr int kThreads = 256;
constexpr int kSums = 3;        // sum adv^2, sum adv lp_a, sum H

// The per-row scale factors, each one rounding: inv_m = fl(1 / M), c_pi = fl(pi_coef inv_m),
// c_v = fl(fl(2 v_coef) inv_m) (the doubling is exact), c_e = fl(ent_coef inv_m).
struct Coefs {
    float c_pi, c_v, c_e;
};

__device__ __forceinline__ Coefs coefs_of(int M, float pi_coef, float v_coef, float ent_coef) {
    const float inv_m = 1.f / (float)M;
    Coefs c;
    c.c_pi = pi_coef * inv_m;
    c.c_v = (2.f * v_coef) * inv_m;
    c.c_e = ent_coef * inv_m;
    return c;
}

// Categorical(logits): lp = log_softmax(z), H = -sum p lp (softmax_row), and by softmax_grad_row
//   dlogits_j = c_pi (-adv) (1[j = a] - p_j) + c_e p_j (lp_j + H),   dvalue = c_v (-adv)
// The action is the float32 A2C.actions stores; it enters through j == a only.
template <int A>
__global__ __launch_bounds__(kThreads) void k_a2c_loss(
    const float *__restrict__ logits, const float *__restrict__ value,
    const float *__restrict__ action, const float *__restrict__ ret, int M, float pi_coef,
    float v_coef, float ent_coef, float *__restrict__ dlogits, float *__restrict__ dvalue,
    double *__restrict__ partial) {
    __shared__ double s_red[kSums][kThreads / 64];
    const int m = blockIdx.x * kThreads + threadIdx.x;
    double sq = 0.0, pol = 0.0, ent = 0.0;
    if (m < M) {
        const Coefs c = coefs_of(M, pi_coef, v_coef, ent_coef);
        float z[A];
#pragma unroll
        for (int j = 0; j < A; ++j) z[j] = logits[(size_t)m * A + j];
        const float af = action[m];
        const int a = (af >= 0.f && af < (float)A) ? (int)af : -1;
        float H, lpa, p[A], lp[A], g[A];
        softmax_row<A>(z, a, lp, p, H, lpa);
        const float adv = ret[m] - value[m];
        const float neg_adv = -adv;
        softmax_grad_row<A>(c.c_pi * neg_adv, c.c_e, a, p, lp, H, g);
#pragma unroll
        for (int j = 0; j < A; ++j) dlogits[(size_t)m * A + j] = g[j];
        dvalue[m] = c.c_v * neg_adv;
        sq = (double)(adv * adv);
        pol = (double)(adv * lpa);
        ent = (double)H;
    }
    sq = wave_sum_f64(sq);
    pol = wave_sum_f64(pol);
    ent = wave_sum_f64(ent);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        s_red[0][wave] = sq;
        s_red[1][wave] = pol;
        s_red[2][wave] = ent;
    }
    block_fold(s_red, kSums, partial);
}

// Independent(Normal(mean, scale), 1) with a scale shared by all rows; log pi and the entropy as
// pfrl_ppo_gaussian_act computes them (gaussian_rows.h).  g = c_pi (-adv) = d total / d log pi:
//   dmean_j = g (a_j - mu_j) / s_j^2,   d total / d scale_j = sum_m g ((a_j - mu_j)^2 / s_j^3 - 1 / s_j)
//                                                             - ent_coef / s_j    (finish)
__global__ __launch_bounds__(kThreads) void k_a2c_gaussian_loss(
    const float *__restrict__ mean, const float *__restrict__ scale,
    const float *__restrict__ value, const float *__restrict__ action,
    const float *__restrict__ ret, int M, int A, float pi_coef, float v_coef, float ent_coef,
    float *__restrict__ dmean, float *__restrict__ dvalue, double *__restrict__ partial) {
    __shared__ double s_red[kSums + kMaxA][kThreads / 64];
    const int m = blockIdx.x * kThreads + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool live = m < M;
    const size_t base = (size_t)(live ? m : 0) * A;
    double sq = 0.0, pol = 0.0, ent = 0.0;
    float g = 0.f;
    if (live) {
        const Coefs c = coefs_of(M, pi_coef, v_coef, ent_coef);
        const float lpa = row_log_prob(action + base, mean + base, scale, A);
        const double H = gaussian_entropy(scale, A);
        const float adv = ret[m] - value[m];
        const float neg_adv = -adv;
        g = c.c_pi * neg_adv;
        dvalue[m] = c.c_v * neg_adv;
        sq = (double)(adv * adv);
        pol = (double)(adv * lpa);
        ent = (double)(float)H;
    }
    sq = wave_sum_f64(sq);
    pol = wave_sum_f64(pol);
    ent = wave_sum_f64(ent);
    if (lane == 0) {
        s_red[0][wave] = sq;
        s_red[1][wave] = pol;
        s_red[2][wave] = ent;
    }
    gaussian_grad_columns(live, g, action, mean, scale, base, A, dmean, s_red, kSums);
    block_fold(s_red, kSums + A, partial);
}

// partial[nblk][3 + A] (A = 0 for the categorical kernel), folded in block order:
// out3 = {value_loss, action_loss, entropy} (the order of A2C._last_losses), dscale[j] (may be NULL),
// and, when avg is not NULL, avg[i] += fl(fl(1 - decay_i) fl(x_i - avg[i])) on x = {action_loss,
// value_loss, entropy} (the order of A2C._avg), the float32 values just written.
__global__ __launch_bounds__(64) void k_a2c_finish(const double *__restrict__ partial, int nblk, int M,
                                                   int A, float ent_coef,
                                                   const float *__restrict__ scale,
                                                   float *__restrict__ out3, float *__restrict__ dscale,
                                                   float *__restrict__ avg, float decay_actor,
                                                   float decay_value, float decay_entropy) {
    const int lane = threadIdx.x;
    float x[kSums] = {0.f, 0.f, 0.f};
    for (int k = 0; k < kSums + A; ++k) {
        double s = fold_column(partial, nblk, kSums + A, k);
        if (lane != 0) continue;
        if (k == 1) s = -s;
        if (k < kSums) {
            x[k] = (float)(s / M);
            out3[k] = x[k];
        } else if (dscale != nullptr) {
            dscale[k - kSums] = (float)(s - (double)ent_coef / (double)scale[k - kSums]);
        }
    }
    if (lane == 0 && avg != nullptr) {
        avg[0] = avg[0] + (1.f - decay_actor) * (x[1] - avg[0]);
        avg[1] = avg[1] + (1.f - decay_value) * (x[0] - avg[1]);
        avg[2] = avg[2] + (1.f - decay_entropy) * (x[2] - avg[2]);
    }
}

}  // namespace

extern "C" int pfrl_a2c_loss(const float *logits, const float *value, const float *action,
                             const float *ret, int32_t M, int32_t A, float pi_coef, float v_coef,
                             float ent_coef, float *dlogits, float *dvalue, double *partial_ws,
                             float *out3, float *avg, float decay_actor, float decay_value,
                             float decay_entropy, void *stream) {
    PFRL_CHECK_ARG(M >= 1 && A >= 1 && A <= kMaxSoftmaxA, "pfrl_a2c_loss: 1 <= A <= 31, M >= 1");
    PFRL_CHECK_ARG(logits && value && action && ret && dlogits && dvalue && partial_ws && out3,
                   "pfrl_a2c_loss: null pointer");
    const unsigned blocks = (unsigned)((M + kThreads - 1) / kThreads);
#define LOSS_CALL(AA)                                                                              \
    case AA:                                                                                       \
        hipLaunchKernelGGL(k_a2c_loss<AA>, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream,   \
                           logits, value, action, ret, M, pi_coef, v_coef, ent_coef, dlogits,      \
                           dvalue, partial_ws);                                                    \
        break;
    PFRL_SWITCH_SOFTMAX_A(A, LOSS_CALL)
#undef LOSS_CALL
    hipLaunchKernelGGL(k_a2c_finish, dim3(1), dim3(64), 0, (hipStream_t)stream, partial_ws, (int)blocks,
                       M, 0, ent_coef, (const float *)nullptr, out3, (float *)nullptr, avg, decay_actor,
                       decay_value, decay_entropy);
    PFRL_LAUNCH_CHECK();
}

extern "C" int pfrl_a2c_gaussian_loss(const float *mean, const float *scale, const float *value,
                                      const float *action, const float *ret, int32_t M, int32_t A,
                                      float pi_coef, float v_coef, float ent_coef, float *dmean,
                                      float *dvalue, float *dscale, double *partial_ws, float *out3,
                                      float *avg, float decay_actor, float decay_value,
                                      float decay_entropy, void *stream) {
    PFRL_CHECK_ARG(M >= 1 && A >= 1 && A <= kMaxA, "pfrl_a2c_gaussian_loss: 1 <= A <= 32, M >= 1");
    PFRL_CHECK_ARG(mean && scale && value && action && ret && dmean && dvalue && partial_ws && out3,
                   "pfrl_a2c_gaussian_loss: null pointer");
    const unsigned blocks = (unsigned)((M + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(k_a2c_gaussian_loss, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, mean,
                       scale, value, action, ret, M, A, pi_coef, v_coef, ent_coef, dmean, dvalue,
                       partial_ws);
    hipLaunchKernelGGL(k_a2c_finish, dim3(1), dim3(64), 0, (hipStream_t)stream, partial_ws, (int)blocks,
                       M, A, ent_coef, scale, out3, dscale, avg, decay_actor, decay_value,
                       decay_entropy);
    PFRL_LAUNCH_CHECK();
}
