// Implicit Quantile Network loss, fused: greedy next action from the mean of the target
// network's quantiles at taus~, Bellman target at taus', quantile Huber loss of every
// (prediction, target) pair, both batch accumulators, the gradient w.r.t. the online
// network's quantiles and the per-sample priorities -- one launch instead of two
// advanced-index gathers, the broadcast pointwise chain over (B, N, N'), its means / sums /
// matmul and autograd's backward through all of it (pfrl/agents/iqn.py:176-255 element-wise
// loss and both accumulators, :340-400 _compute_target_values / _compute_y_and_taus /
// _compute_loss; pfrl/action_value.py QuantileDiscreteActionValue.greedy_actions and
// evaluate_actions_as_quantiles).
//
// Launch shape: ONE workgroup of 16 waves, one 64-lane wave per sample at a time (a wave
// loops over b = wave, wave + 16, ...), as k_c51_loss.  A sample is at most 64 x 64 pairs:
// lane = prediction i, the N' targets sit in LDS and are read as a broadcast, the two sums
// over j run in registers in increasing j.  The scalar loss is a sum over ALL samples that
// must be bit-identical from run to run in a single launch: inside one workgroup that is a
// barrier and a fixed-order fold of per-sample partials in LDS; spread over several
// workgroups it would need float atomics (arrival order), a second launch, or a workspace
// with an arrival counter that the entry point does not have.  At the agent's B = 32 the 16
// waves take two samples each, about 64 iterations of a dozen vector instructions per sample:
// the launch is latency, not throughput, and sits between two network passes that fill
// the chip.  Packing rows over many workgroups would pay only from a few hundred rows on.
//
// No float atomics; every sum has a fixed order (k, then j, then the butterfly over i, then
// b), so the same inputs give the same bits on every run.
#include "common.h"
#include "row_reduce.h"

namespace {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxBatch = 4096;
constexpr int kMaxQ = 64;       // N, N', K and A: one lane each

__global__ __launch_bounds__(kThreads) void k_iqn_loss(
    const float *__restrict__ quantiles, const int64_t *__restrict__ action,
    const float *__restrict__ taus, const float *__restrict__ next_quantiles,
    const float *__restrict__ next_select, const float *__restrict__ reward,
    const float *__restrict__ discount, const float *__restrict__ terminal,
    const float *__restrict__ weights, int B, int N, int Np, int K, int A, int mean,
    float *__restrict__ out_loss, float *__restrict__ out_grad, float *__restrict__ out_delta,
    float *__restrict__ out_t) {
    __shared__ float s_t[kWaves][kMaxQ];
    __shared__ float s_part[kMaxBatch];
    const int lane = threadIdx.x & 63;
    // (in an SGPR: the loop over this wave's samples and their scalar operands become uniform)
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const float inv_b = 1.0f / (float)B;
    const float f_np = (float)Np, f_k = (float)K, f_pairs = (float)(N * Np);
    for (int b = wave; b < B; b += kWaves) {
        const int64_t act = action[b];
        const float rew = reward[b], term = terminal[b], disc = discount[b];
        // lane = prediction i: y[i] and its threshold, requested before the selection loop
        const int il = min(lane, N - 1);
        const float y = quantiles[((int64_t)b * N + il) * A + act];
        const float tau = taus[(int64_t)b * N + il];
        // greedy next action, lane = action a: sum over k in increasing k, divided by K; eight
        // clamped loads in one basic block at a time (in flight together)
        const float *sel = next_select + (int64_t)b * K * A;
        const int al = min(lane, A - 1);
        float qsum = 0.0f;
        for (int k0 = 0; k0 < K; k0 += 8) {
            float sv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) sv[u] = sel[min(k0 + u, K - 1) * A + al];
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (k0 + u < K) qsum = __fadd_rn(qsum, sv[u]);
        }
        // first maximum, like torch.argmax: (value, index) butterfly, the lower index wins a
        // tie; `>` never ranks a NaN as the maximum; lanes past A hold -inf and their own index
        float bv = lane < A ? __fdiv_rn(qsum, f_k) : -INFINITY;
        int bi = lane;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float ov = __shfl_xor(bv, off, 64);
            const int oi = __shfl_xor(bi, off, 64);
            if (ov > bv || (ov == bv && oi < bi)) {
                bv = ov;
                bi = oi;
            }
        }
        const int g = min(__builtin_amdgcn_readfirstlane(bi), A - 1);
        // Bellman target, lane = target quantile j
        const int jl = min(lane, Np - 1);
        const float nq = next_quantiles[((int64_t)b * Np + jl) * A + g];
        const float t = __fadd_rn(rew, __fmul_rn(__fmul_rn(disc, __fsub_rn(1.0f, term)), nq));
        s_t[wave][lane] = t;
        if (out_t != nullptr && lane < Np) out_t[(int64_t)b * Np + lane] = t;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        // the pairs: lane = i, j increasing
        float el_sum = 0.0f, g_sum = 0.0f;
        for (int j = 0; j < Np; ++j) {
            const float tj = s_t[wave][j];
            const float u = __fsub_rn(y, tj);
            const float au = fabsf(u);
            const float huber = au < 1.0f ? __fmul_rn(__fmul_rn(0.5f, u), u) : __fsub_rn(au, 0.5f);
            const float w = fabsf(__fsub_rn(tau, tj < y ? 1.0f : 0.0f));
            el_sum = __fadd_rn(el_sum, __fmul_rn(w, huber));
            g_sum = __fadd_rn(g_sum, __fmul_rn(w, fminf(fmaxf(u, -1.0f), 1.0f)));
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const bool on = lane < N;
        float coef = weights != nullptr ? weights[b] : 1.0f;
        if (mean) coef = __fmul_rn(coef, inv_b);
        const float d = wave_sum_f32(on ? el_sum : 0.0f);
        const float row = wave_sum_f32(on ? __fdiv_rn(el_sum, f_np) : 0.0f);
        const float gy = __fmul_rn(__fdiv_rn(g_sum, f_np), coef);
        // the whole [N][A] slice of the gradient: the taken action's column, +0.0 elsewhere
        float *grow = out_grad + (int64_t)b * N * A;
        const int na = N * A;
        for (int base = 0; base < na; base += 64) {
            const int idx = base + lane;
            const int i = idx / A;
            const float gi = __shfl(gy, i & 63, 64);
            if (idx < na) grow[idx] = (idx - i * A) == act ? gi : 0.0f;
        }
        if (lane == 0) {
            out_delta[b] = __fdiv_rn(d, f_pairs);
            s_part[b] = __fmul_rn(row, coef);
        }
    }
    __syncthreads();
    if (wave == 0) {
        float acc = 0.0f;
        for (int b = lane; b < B; b += 64) acc += s_part[b];
        acc = wave_sum_f32(acc);
        if (lane == 0) out_loss[0] = acc;
    }
}

}  // namespace

extern "C" int pfrl_iqn_loss(const float *quantiles, const int64_t *action, const float *taus,
                             const float *next_quantiles, const float *next_select,
                             const float *reward, const float *discount, const float *terminal,
                             const float *weights, int32_t B, int32_t N, int32_t Np, int32_t K,
                             int32_t A, int32_t mean, float *out_loss, float *out_grad,
                             float *out_delta, float *out_t, void *stream) {
    PFRL_CHECK_ARG(B >= 1 && B <= kMaxBatch, "pfrl_iqn_loss: batch size must be in [1, 4096]");
    PFRL_CHECK_ARG(N >= 1 && N <= kMaxQ && Np >= 1 && Np <= kMaxQ && K >= 1 && K <= kMaxQ,
                   "pfrl_iqn_loss: N, N' and K must be in [1, 64]");
    PFRL_CHECK_ARG(A >= 1 && A <= kMaxQ, "pfrl_iqn_loss: the number of actions must be in [1, 64]");
    PFRL_CHECK_ARG(quantiles != nullptr && action != nullptr && taus != nullptr &&
                       next_quantiles != nullptr && next_select != nullptr && reward != nullptr &&
                       discount != nullptr && terminal != nullptr && out_loss != nullptr &&
                       out_grad != nullptr && out_delta != nullptr,
                   "pfrl_iqn_loss: only weights and out_t may be NULL");
    hipLaunchKernelGGL(k_iqn_loss, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, quantiles,
                       action, taus, next_quantiles, next_select, reward, discount, terminal,
                       weights, (int)B, (int)N, (int)Np, (int)K, (int)A, (int)mean, out_loss,
                       out_grad, out_delta, out_t);
    PFRL_LAUNCH_CHECK();
}
