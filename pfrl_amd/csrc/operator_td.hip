// Fused target-and-loss launch of the DQN variants whose Bellman target is an OPERATOR on the
// target network's action values at s and at s': advantage learning (AL, PAL, DoublePAL) and
// dynamic policy programming (DPP, DPPL, DPPGreedy).  Replaces, with ONE launch, the gather /
// argmax / softmax / logsumexp / elementwise / reduce / scatter chain PyTorch launches for
//     pfrl/agents/al.py, pal.py, double_pal.py  _compute_y_and_t
//     pfrl/agents/dpp.py:19-83,99-127           _l_operator, _compute_target_values, _compute_y_and_t
//     pfrl/agents/dqn.py                        compute_value_loss / compute_weighted_value_loss
//     pfrl/action_value.py:60-79                evaluate_actions, compute_advantage, compute_expectation
// and for the loss's backward pass (the gradient w.r.t. Q(s) is analytic, one entry per row).
//
// Launch shape: ONE workgroup of 16 waves, one 64-lane wave per row at a time (a wave loops over
// b = wave, wave + 16, ...), lane = action (A <= 64), the shape of k_iqn_loss / k_c51_loss.  All
// of a row's operands -- the three or four [A] rows and the replay columns -- are requested
// unconditionally at the top of the iteration (optional operands through a pointer that is
// always valid, lanes past A through a clamped index), one coalesced load each.  Maxima are
// butterflies (max is exact, so the order does not matter; the argmax carries its index and the
// lower index wins a tie); the sums of the Boltzmann operators run over INCREASING a, every
// lane reading lane a's term out of the vector register (v_readlane, a is wave-uniform), so no
// LDS and no barrier inside a row.  The replay agents run B = 8 ... 256: the launch is a latency
// chain, not throughput.  The scalar loss must be bit-identical from run to run in a single
// launch: every wave adds its own rows' terms in increasing b, the 16 partials are folded in
// wave order behind one barrier.  No float atomics.
#include <math.h>

#include "common.h"

namespace {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;

enum { OP_AL = 0, OP_PAL = 1, OP_DOUBLE_PAL = 2, OP_DPP = 3, OP_DPPL = 4, OP_DPP_GREEDY = 5 };

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}

// lane l's value in every lane; l is wave-uniform
__device__ __forceinline__ float lane_value(float v, int l) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}

// The operator L of DPP (softmax(eta x) . x) or DPPL (logsumexp(eta x) / eta) on the row a
// wave holds one element per lane of (x, lanes past A hold anything finite), mx = max_a x.
// Max-subtracted; both sums over increasing a.
template <int OP>
__device__ __forceinline__ void boltzmann_pair(float xc, float mxc, float xn, float mxn, int A,
                                               float eta, float &Lc, float &Ln) {
    // (rounding is monotone and eta > 0: max_a fl(eta x_a) == fl(eta max_a x_a))
    const float mzc = __fmul_rn(eta, mxc), mzn = __fmul_rn(eta, mxn);
    const float ec = expf(__fsub_rn(__fmul_rn(eta, xc), mzc));
    const float en = expf(__fsub_rn(__fmul_rn(eta, xn), mzn));
    float sc = 0.0f, sn = 0.0f;
    for (int a = 0; a < A; ++a) {
        sc = __fadd_rn(sc, lane_value(ec, a));
        sn = __fadd_rn(sn, lane_value(en, a));
    }
    if (OP == OP_DPPL) {
        Lc = __fdiv_rn(__fadd_rn(mzc, logf(sc)), eta);
        Ln = __fdiv_rn(__fadd_rn(mzn, logf(sn)), eta);
        return;
    }
    const float tc = __fmul_rn(__fdiv_rn(ec, sc), xc), tn = __fmul_rn(__fdiv_rn(en, sn), xn);
    float lc = 0.0f, ln = 0.0f;
    for (int a = 0; a < A; ++a) {
        lc = __fadd_rn(lc, lane_value(tc, a));
        ln = __fadd_rn(ln, lane_value(tn, a));
    }
    Lc = lc;
    Ln = ln;
}

template <int OP>
__global__ __launch_bounds__(kThreads) void k_dqn_operator_td_loss(
    const float *__restrict__ q, const float *__restrict__ target_cur,
    const float *__restrict__ target_next, const float *__restrict__ next_online,
    const int64_t *__restrict__ action, const float *__restrict__ reward,
    const float *__restrict__ discount, const float *__restrict__ terminal,
    const float *__restrict__ weights, int64_t B, int A, float param, int clip_delta, int mean,
    float *__restrict__ out_loss, float *__restrict__ out_grad_q, float *__restrict__ out_y,
    float *__restrict__ out_abs_delta, float *__restrict__ out_t) {
    __shared__ float s_part[kWaves];
    const int lane = threadIdx.x & 63;
    // (in an SGPR: the loop over this wave's rows and their scalar operands become uniform)
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const float scale = mean ? 1.0f / (float)B : 1.0f;
    // (optional inputs are read through a pointer that is always valid: no branch at a load)
    const float *__restrict__ sel_src = OP == OP_DOUBLE_PAL ? next_online : target_next;
    const float *__restrict__ wt_src = weights ? weights : reward;
    const int al = min(lane, A - 1);
    const bool on = lane < A;
    float local = 0.0f;
    for (int64_t b = wave; b < B; b += kWaves) {
        const int64_t at = b * A + al;
        const float qv = q[at], tcv = target_cur[at], tnv = target_next[at], sv = sel_src[at];
        const int act = __builtin_amdgcn_readfirstlane((int)action[b]);
        const float rew = reward[b], disc = discount[b], term = terminal[b];
        const float wt_raw = wt_src[b];
        const float wt = weights ? wt_raw : 1.0f;
        const float y = lane_value(qv, act);
        const float tca = lane_value(tcv, act);
        const float mc = wave_max(on ? tcv : -INFINITY), mn = wave_max(on ? tnv : -INFINITY);
        const float coef = __fmul_rn(disc, __fsub_rn(1.0f, term));
        float t;
        if (OP == OP_AL || OP == OP_PAL || OP == OP_DOUBLE_PAL) {
            float next = mn;
            if (OP == OP_DOUBLE_PAL) {
                // first maximum of the online network's values at s', like torch.argmax:
                // (value, index) butterfly, strict > and the lower index wins a tie
                float bv = on ? sv : -INFINITY;
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
                next = lane_value(tnv, min(__builtin_amdgcn_readfirstlane(bi), A - 1));
            }
            const float tq = __fadd_rn(rew, __fmul_rn(coef, next));
            float gap = __fsub_rn(tca, mc);
            if (OP != OP_AL) gap = fmaxf(gap, __fsub_rn(lane_value(tnv, act), mn));
            t = __fadd_rn(tq, __fmul_rn(param, gap));
        } else {
            float Lc = mc, Ln = mn;
            if (OP != OP_DPP_GREEDY) boltzmann_pair<OP>(tcv, mc, tnv, mn, A, param, Lc, Ln);
            const float ahead = __fadd_rn(rew, __fmul_rn(coef, Ln));
            t = __fsub_rn(__fadd_rn(tca, ahead), Lc);
        }
        // loss and gradient: k_dqn_td_loss's
        const float d = __fsub_rn(y, t);
        const float ad = fabsf(d);
        float l, g;
        if (clip_delta) {
            l = ad < 1.0f ? __fmul_rn(__fmul_rn(0.5f, ad), ad) : __fsub_rn(ad, 0.5f);
            g = ad < 1.0f ? d : (d > 0.0f ? 1.0f : -1.0f);
        } else {
            l = __fmul_rn(0.5f, __fmul_rn(d, d));
            g = d;
        }
        local += l * wt;
        const float gq = g * wt * scale;
        if (on) out_grad_q[b * A + lane] = (lane == act) ? gq : 0.0f;
        if (lane == 0) {
            out_y[b] = y;
            out_abs_delta[b] = ad;
            if (out_t != nullptr) out_t[b] = t;
        }
    }
    if (lane == 0) s_part[wave] = local;
    __syncthreads();
    if (threadIdx.x == 0) {
        float tot = 0.0f;
        for (int k = 0; k < kWaves; ++k) tot += s_part[k];
        out_loss[0] = tot * scale;
    }
}

}  // namespace

extern "C" int pfrl_dqn_operator_td_loss(
    const float *q, const float *target_cur, const float *target_next, const float *next_online,
    const int64_t *action, const float *reward, const float *discount, const float *terminal,
    const float *weights, int64_t B, int32_t A, int32_t op, float param, int clip_delta, int mean,
    float *out_loss, float *out_grad_q, float *out_y, float *out_abs_delta, float *out_t,
    void *stream) {
    PFRL_CHECK_ARG(B >= 1 && A >= 1 && A <= 64,
                   "pfrl_dqn_operator_td_loss: B >= 1 and 1 <= A <= 64");
    PFRL_CHECK_ARG(op >= OP_AL && op <= OP_DPP_GREEDY, "pfrl_dqn_operator_td_loss: op must be in 0..5");
    PFRL_CHECK_ARG((next_online != nullptr) == (op == OP_DOUBLE_PAL),
                   "pfrl_dqn_operator_td_loss: next_online is DoublePAL's (op 2) and only its");
    PFRL_CHECK_ARG(isfinite(param) && ((op != OP_DPP && op != OP_DPPL) || param > 0.0f),
                   "pfrl_dqn_operator_td_loss: alpha must be finite, eta finite and positive");
    PFRL_CHECK_ARG(q != nullptr && target_cur != nullptr && target_next != nullptr &&
                       action != nullptr && reward != nullptr && discount != nullptr &&
                       terminal != nullptr && out_loss != nullptr && out_grad_q != nullptr &&
                       out_y != nullptr && out_abs_delta != nullptr,
                   "pfrl_dqn_operator_td_loss: only next_online, weights and out_t may be NULL");
#define CALL_OP(OP)                                                                              \
    hipLaunchKernelGGL((k_dqn_operator_td_loss<OP>), dim3(1), dim3(kThreads), 0,                 \
                       (hipStream_t)stream, q, target_cur, target_next, next_online, action,     \
                       reward, discount, terminal, weights, B, (int)A, param, clip_delta, mean,  \
                       out_loss, out_grad_q, out_y, out_abs_delta, out_t)
    switch (op) {
        case OP_AL: CALL_OP(OP_AL); break;
        case OP_PAL: CALL_OP(OP_PAL); break;
        case OP_DOUBLE_PAL: CALL_OP(OP_DOUBLE_PAL); break;
        case OP_DPP: CALL_OP(OP_DPP); break;
        case OP_DPPL: CALL_OP(OP_DPPL); break;
        default: CALL_OP(OP_DPP_GREEDY); break;
    }
#undef CALL_OP
    PFRL_LAUNCH_CHECK();
}
