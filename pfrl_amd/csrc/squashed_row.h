// The example squashed-Gaussian policy head on ONE element (examples/mujoco/reproduction/
// soft_actor_critic/train_soft_actor_critic.py:128-141), shared by k_squashed_head_fwd / _bwd
// (actor.hip) and k_squashed_head_act (actor_act.hip): the launches produce the same scale, the same
// pre-squash sample and the same action bit for bit from the same (mean, log_scale, eps).  Every line
// is one rounded IEEE operation in the order of the torch code it replaces (the files are built with
// -ffp-contract=off): clamp, (mul,) exp(, sqrt), then `torch.normal(loc, scale)`'s eps * scale + loc
// as a multiply and an add, then tanh.
#pragma once
#include <hip/hip_runtime.h>

namespace {

// scale = sqrt(exp(2 clamp(log_scale, lo, hi))) (MODE 0) or exp(clamp(log_scale, lo, hi)) (MODE 1);
// v: the value of the exp, which the backward formulas reuse
template <int MODE>
__device__ __forceinline__ float head_scale(float ls, float lo, float hi, float &v) {
    float c = ls < lo ? lo : ls;          // torch.clamp: min(max(x, lo), hi), NaN passes through
    c = c > hi ? hi : c;
    if (MODE == 0) {
        v = expf(c * 2.f);
        return sqrtf(v);
    }
    v = expf(c);
    return v;
}

// action = tanh(u), u = mean + eps * scale (`sample`) or the distribution's mode u = mean;
// s: the scale, u: the pre-squash value (what the log-probability is evaluated at)
template <int MODE>
__device__ __forceinline__ float squashed_head_action(float mean, float ls, float lo, float hi, bool sample,
                                                      float eps, float &s, float &u) {
    float v;
    s = head_scale<MODE>(ls, lo, hi, v);
    u = sample ? mean + eps * s : mean;
    return tanhf(u);
}

}  // namespace
