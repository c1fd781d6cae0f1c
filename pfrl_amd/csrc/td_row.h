// The per-row lines of the one-step TD losses (pfrl/agents/dqn.py:44-104, 388-470), shared by the
// DQN launches of tdloss.hip and the NAF launch of naf.hip: the target, the Huber / squared term
// and its derivative.  Every step is one rounded f32 operation in the reference's association.
#pragma once
#include <hip/hip_runtime.h>

namespace {

// t = r + (disc * (1 - term)) * next
__device__ __forceinline__ float td_target(float reward, float discount, float terminal, float next) {
    const float coef = __fmul_rn(discount, __fsub_rn(1.0f, terminal));
    return __fadd_rn(reward, __fmul_rn(coef, next));
}

// l = Huber(1)(d) or d^2 / 2, g = dl/dd; ad = |d|
__device__ __forceinline__ void td_loss_term(float d, float ad, int clip_delta, float &l, float &g) {
    if (clip_delta) {
        l = ad < 1.0f ? __fmul_rn(__fmul_rn(0.5f, ad), ad) : __fsub_rn(ad, 0.5f);
        g = ad < 1.0f ? d : (d > 0.0f ? 1.0f : -1.0f);
    } else {
        l = __fmul_rn(0.5f, __fmul_rn(d, d));
        g = d;
    }
}

}  // namespace
