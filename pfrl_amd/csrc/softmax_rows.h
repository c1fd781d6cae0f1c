// Row arithmetic of a Categorical(logits) policy with A <= kMaxSoftmaxA (common.h) actions, one row
// in the registers of one thread, shared by the PPO kernels (rollout.hip), A2C (a2c.hip) and
// REINFORCE (reinforce.hip): the three produce the same log-probabilities, entropy and gradient
// bit for bit from the same logits.  Every line is one rounded float32 operation, in this order.
#pragma once
#include <hip/hip_runtime.h>

namespace {

// torch.logsumexp(z): mx = max_j z_j, e_j = exp(z_j - mx), sum = e_0 + e_1 + ... (in index order),
// lse = mx + log(sum).  z may be longer than A (a value column behind the logits).
template <int A, int N>
__device__ __forceinline__ float softmax_lse(const float (&z)[N], float (&e)[A], float &sum) {
    static_assert(N >= A, "softmax_lse: A logits");
    float mx = z[0];
#pragma unroll
    for (int j = 1; j < A; ++j) mx = fmaxf(mx, z[j]);
    sum = 0.f;
#pragma unroll
    for (int j = 0; j < A; ++j) {
        e[j] = expf(z[j] - mx);
        sum += e[j];
    }
    const float lse = mx + logf(sum);
    return lse;
}

// Categorical(logits = z): lp = z - lse (log_softmax), p = e / sum (softmax),
// H = -sum_j p_j lp_j subtracted term by term in index order (Categorical.entropy(); a probability
// of exactly zero contributes nothing, where p lp would be 0 * -inf), lpa = lp[a] (0 when a is not
// an index of the row).
template <int A>
__device__ __forceinline__ void softmax_row(const float (&z)[A], int a, float (&lp)[A], float (&p)[A],
                                            float &H, float &lpa) {
    float e[A], sum;
    const float lse = softmax_lse<A>(z, e, sum);
    H = 0.f;
    lpa = 0.f;
#pragma unroll
    for (int j = 0; j < A; ++j) {
        lp[j] = z[j] - lse;
        p[j] = e[j] / sum;
        H -= p[j] > 0.f ? p[j] * lp[j] : 0.f;
        if (j == a) lpa = lp[j];
    }
}

// Gradient with respect to the logits of a row's loss, given gl = d loss / d lp_a and
// ge = -d loss / d H (d lp_a / d z_j = 1[j = a] - p_j, d H / d z_j = -p_j (lp_j + H)):
//   g_j = gl (1[j = a] - p_j) + (p_j > 0 ? (ge p_j) (lp_j + H) : 0)
template <int A>
__device__ __forceinline__ void softmax_grad_row(float gl, float ge, int a, const float (&p)[A],
                                                 const float (&lp)[A], float H, float (&g)[A]) {
#pragma unroll
    for (int j = 0; j < A; ++j) {
        const float onehot = j == a ? 1.f : 0.f;
        float gj = gl * (onehot - p[j]);
        gj += p[j] > 0.f ? ge * p[j] * (lp[j] + H) : 0.f;
        g[j] = gj;
    }
}

}  // namespace
