// Row arithmetic of PPO._lossfun (pfrl/agents/ppo.py:634-671) that does not depend on the policy's
// distribution: the clipped surrogate as a function of log pi(a|s), and the (clipped) value loss.
// Shared by the categorical kernels (rollout.hip) and the Gaussian ones (ppo_gaussian.hip), so that
// both treat clip bounds and ties the way torch's min / max / clamp backward do.
#pragma once
#include <hip/hip_runtime.h>

// surr = min(ratio adv, clamp(ratio, 1 - eps, 1 + eps) adv) with ratio = exp(lpa - lpo);
// g_lpa = d(-surr / M) / d lpa
__device__ __forceinline__ void ppo_surrogate_row(float lpa, float lpo, float ad, float inv_m,
                                                  float clip_eps, float &surr, float &g_lpa) {
    const float ratio = expf(lpa - lpo);
    const float lo = 1.0f - clip_eps, hi = 1.0f + clip_eps;
    const float rc = fminf(fmaxf(ratio, lo), hi);
    const float s1 = ratio * ad, s2 = rc * ad;
    surr = fminf(s1, s2);
    // d surr / d ratio: both operands of min carry it inside the clip range (a tie: half
    // each, summing to adv); outside only the unclipped product does, if it is the minimum
    const bool inside = ratio >= lo && ratio <= hi;
    float ds = 0.f;
    if (inside) ds = ad;
    else if (s1 < s2) ds = ad;
    else if (s1 == s2) ds = 0.5f * ad;
    g_lpa = -inv_m * ds * ratio;
}

// loss = loss_policy + value_func_coef loss_value + entropy_coef loss_entropy on the three float32
// means, loss_entropy = -mean H, added left to right as ppo.py:665-669 adds them
__device__ __forceinline__ float ppo_total_loss(float pol, float val, float ent, float vf_coef,
                                                float ent_coef) {
    return (pol + vf_coef * val) + ent_coef * (-ent);
}

// lv = (v - vt)^2, or max((v - vt)^2, (clip(v, vo -+ eps_vf) - vt)^2) when clip_eps_vf >= 0;
// gv = d lv / d v
__device__ __forceinline__ void ppo_value_row(float v, float vo, float vt, float clip_eps_vf,
                                              float &lv, float &gv) {
    const float d1 = v - vt;
    lv = d1 * d1;
    gv = 2.f * d1;
    if (clip_eps_vf >= 0.f) {
        const float vlo = vo - clip_eps_vf, vhi = vo + clip_eps_vf;
        const float vc = fminf(fmaxf(v, vlo), vhi);
        const float d2 = vc - vt;
        const float l2 = d2 * d2;
        // d vc / d v: torch.min(torch.max(v, lo), hi) -- 1 strictly inside, 1/2 at a bound
        // (max / min split ties), 0 outside; the two factors multiply, so clip_eps_vf == 0 with
        // v == v_old (lo == hi == v) is halved twice: 1/4
        const float dmax = v > vlo ? 1.f : (v == vlo ? 0.5f : 0.f);
        const float vm = fmaxf(v, vlo);
        const float dmin = vm < vhi ? 1.f : (vm == vhi ? 0.5f : 0.f);
        const float dvc = dmax * dmin;
        if (l2 > lv) {
            lv = l2;
            gv = 2.f * d2 * dvc;
        } else if (l2 == lv) {
            gv = 0.5f * (2.f * d1) + 0.5f * (2.f * d2 * dvc);
        }
    }
}
