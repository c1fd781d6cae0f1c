// NAF (normalized advantage function) TD loss of DQN / DoubleDQN with a quadratic Q-function, and its
// gradients with respect to the four raw head outputs, in ONE launch.  Replaces, per update,
//     pfrl/q_functions/state_q_functions.py FCQuadraticStateQFunction.forward behind its Linear layers
//         (tanh and scale, exp, lower_triangular_matrix, L L^T)
//     pfrl/action_value.py QuadraticActionValue (greedy_actions, max, evaluate_actions)
//     pfrl/agents/dqn.py _compute_y_and_t, _compute_target_values, compute_value_loss,
//         compute_weighted_value_loss; pfrl/agents/double_dqn.py
// for the online and the target network and their backward passes: a few dozen stock launches of
// 4-5 us each around 32 x n numbers.
//
//   mu = tanh(m) half_width + centre (or m),  L_ii = exp(e_i),  L_ij = c_k (k = i (i - 1) / 2 + j, i > j)
//   d = a - mu,  w = L^T d,  y = v - 1/2 |w|^2            (P = L L^T is never formed)
//   a* = min(high, max(low, mu*)), mu* = the target's mu' (DQN) or the online mu'' at s' (DoubleDQN)
//   next = v' - 1/2 |L'^T (a* - mu')|^2, or v' itself with no bounds and no Double (the maximiser is mu')
//   (all of the above in f64 on the f32 inputs; y and next are rounded to f32 once)
//   t, delta = y - t, Huber / squared term, weights: td_row.h, as k_dqn_td_loss; the terms are added
//   in f64 (rows in a fixed order) and the mean or sum is rounded to f32 once
//   g = dloss/dy:  dv = g,  dL_ij = -g d_i w_j,  dc_k = dL_ij,  de_i = dL_ii L_ii,
//                  dmu = g (L w),  dm = dmu half_width (1 - tanh^2 m) (or dmu)
//
// ONE WAVE OWNS ONE ROW, lane j column j of L and -- loaded a second time, from cache -- row j, so
// that L^T d and L w are both sums inside a lane; d_i and w_j reach the other lanes as lane reads
// with a constant index.  NB (4, 8, 16 or 32 >= n) bounds the unrolled loops: every load of a row is
// unconditional (an index outside the triangle reads element 0 of the row, an absent input reads
// through a pointer that is valid) and issued before the first use.  One workgroup of W waves (16
// up to n = 4, then 8 up to n = 16, then 4: the register arrays grow with NB) walks the rows (wave w: rows w,
// w + W, ...) and adds its loss terms in that order; the W wave sums are added in wave order.  No
// float atomics: the same inputs give the same bits on every launch.  B is 32 in practice, so the
// launch is latency-bound and one workgroup is enough.
#include "common.h"
#include "row_reduce.h"
#include "td_row.h"

namespace {

constexpr int kMaxWaves = 16;
constexpr int kMaxN = 32;

// NaN-propagating, as torch.max / torch.min
__device__ __forceinline__ double torch_max(double a, double b) { return (a > b || a != a) ? a : b; }
__device__ __forceinline__ double torch_min(double a, double b) { return (a < b || a != a) ? a : b; }

struct NafArgs {
    const float *v, *m, *e, *c;         // online network at s
    const float *tv, *tm, *te, *tc;     // target network at s'
    const float *m2;                    // online mu at s' (DoubleDQN) or null
    const float *action, *reward, *discount, *terminal, *weights;
    const float *half_width, *centre, *low, *high;
    float *loss, *y, *abs_delta, *dv, *dm, *de, *dc;
};

// WAVES: 16 up to n = 4, 8 up to n = 16, 4 beyond (three register arrays of NB floats per lane)
template <int NB, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void k_naf_td_loss(NafArgs a, int B, int n, int clip_delta,
                                                            int mean) {
    __shared__ double s_part[kMaxWaves];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nc = n * (n - 1) / 2;
    const bool on = lane < n;
    const int l = on ? lane : 0;                    // (lanes past n read column 0 and write nothing)
    const bool scale_mu = a.half_width != nullptr;
    const bool next_quad = a.m2 != nullptr || a.low != nullptr || a.high != nullptr;
    // optional inputs through pointers that are always valid: no branch at a load
    const float *__restrict__ c_src = nc ? a.c : a.e;
    const float *__restrict__ tc_src = nc ? a.tc : a.te;
    const float *__restrict__ m2_src = a.m2 ? a.m2 : a.tm;
    const float *__restrict__ wt_src = a.weights ? a.weights : a.reward;
    const float *__restrict__ hw_src = scale_mu ? a.half_width : a.e;
    const float *__restrict__ ce_src = scale_mu ? a.centre : a.e;
    const float *__restrict__ lo_src = a.low ? a.low : a.e;
    const float *__restrict__ hi_src = a.high ? a.high : a.e;
    const float hw_raw = hw_src[l], ce_raw = ce_src[l], lo_raw = lo_src[l], hi_raw = hi_src[l];
    const float scale = mean ? 1.0f / (float)B : 1.0f;
    const int row_off = l * (l - 1) / 2;            // row l of the triangle: c[row_off + j], j < l
    double local = 0.0;                             // (the loss sum in f64: B terms of any size)
    for (int b = wave; b < B; b += WAVES) {
        const size_t bn = (size_t)b * n;
        // (wave-uniform row pointers, 32-bit lane offsets)
        const float *__restrict__ crow = c_src + (size_t)b * nc;
        const float *__restrict__ tcrow = tc_src + (size_t)b * nc;
        float *__restrict__ dcrow = a.dc + (size_t)b * nc;
        float col[NB], trow[NB], tcol[NB];
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            // column l: L_il, l < i < n;  row l: L_lj, j = i < l
            const unsigned kc = (i > l && i < n && on) ? i * (i - 1) / 2 + l : 0;
            const unsigned kr = (i < l && on) ? row_off + i : 0;
            col[i] = crow[kc];
            trow[i] = crow[kr];
            tcol[i] = tcrow[kc];
        }
        const float v = a.v[b], tv = a.tv[b];
        const float m = a.m[bn + l], e = a.e[bn + l], tm = a.tm[bn + l], te = a.te[bn + l];
        const float m2 = m2_src[bn + l], act = a.action[bn + l];
        const float rew = a.reward[b], disc = a.discount[b], term = a.terminal[b];
        const float wt = a.weights ? wt_src[b] : 1.0f;

        // online network at s.  The row arithmetic is f64 on the f32 inputs, rounded to f32 once per
        // output: a handful of operations per lane, and y, next and the gradients then carry no
        // rounding of their own beyond that of the TD error they share with the reference.
        const double hw = (double)hw_raw, ce = (double)ce_raw;
        const double th = tanh((double)m);
        const double mu = scale_mu ? th * hw + ce : (double)m;
        const double diag = exp((double)e);
        const double d = on ? (double)act - mu : 0.0;
        double w = diag * d;
#pragma unroll
        for (int i = 1; i < NB; ++i) {
            const double di = __shfl(d, i, 64);
            w = fma((i > l && i < n) ? (double)col[i] : 0.0, di, w);
        }
        w = on ? w : 0.0;
        const float y = (float)((double)v - 0.5 * wave_sum_f64(w * w));

        // target network at s'
        float next = tv;
        if (next_quad) {                            // (uniform over the launch)
            const double tmu = scale_mu ? tanh((double)tm) * hw + ce : (double)tm;
            double star = tmu;
            if (a.m2 != nullptr) star = scale_mu ? tanh((double)m2) * hw + ce : (double)m2;
            if (a.low != nullptr) star = torch_max((double)lo_raw, star);
            if (a.high != nullptr) star = torch_min((double)hi_raw, star);
            const double td = on ? star - tmu : 0.0;
            double tw = exp((double)te) * td;
#pragma unroll
            for (int i = 1; i < NB; ++i) {
                const double di = __shfl(td, i, 64);
                tw = fma((i > l && i < n) ? (double)tcol[i] : 0.0, di, tw);
            }
            tw = on ? tw : 0.0;
            next = (float)((double)tv - 0.5 * wave_sum_f64(tw * tw));
        }

        const float t = td_target(rew, disc, term, next);
        const float delta = __fsub_rn(y, t);
        const float ad = fabsf(delta);
        float lt, g;
        td_loss_term(delta, ad, clip_delta, lt, g);
        local += (double)(lt * wt);
        const float gq = g * wt * scale;

        // gradients: dL_il = -gq d_i w_l down column l, dmu_l = gq (L w)_l along row l
        const double ngw = -((double)gq * w);
        double lw = diag * w;
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const double di = __shfl(d, i, 64), wi = __shfl(w, i, 64);
            if (i > l && i < n && on) dcrow[(unsigned)(i * (i - 1) / 2 + l)] = (float)(ngw * di);
            lw = fma((i < l) ? (double)trow[i] : 0.0, wi, lw);
        }
        if (on) {
            const double dmu = (double)gq * lw;
            a.de[bn + l] = (float)((ngw * d) * diag);
            a.dm[bn + l] = (float)(scale_mu ? (dmu * hw) * (1.0 - th * th) : dmu);
        }
        if (lane == 0) {
            a.dv[b] = gq;
            a.y[b] = y;
            a.abs_delta[b] = ad;
        }
    }
    // every lane of a wave holds the same `local`
    if (lane == 0) s_part[wave] = local;
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = 0.0;
        for (int k = 0; k < WAVES; ++k) tot += s_part[k];
        a.loss[0] = (float)(mean ? tot / (double)B : tot);
    }
}

}  // namespace

extern "C" int pfrl_naf_td_loss(const float *v, const float *m, const float *e, const float *c,
                                const float *tv, const float *tm, const float *te, const float *tc,
                                const float *m2, const float *action, const float *reward,
                                const float *discount, const float *terminal, const float *weights,
                                const float *half_width, const float *centre, const float *low,
                                const float *high, int32_t B, int32_t n, int clip_delta, int mean,
                                float *out_loss, float *out_y, float *out_abs_delta, float *dv, float *dm,
                                float *de, float *dc, void *stream) {
    PFRL_CHECK_ARG(B >= 1 && n >= 1 && n <= kMaxN, "pfrl_naf_td_loss: B >= 1, 1 <= n <= 32");
    PFRL_CHECK_ARG(v && m && e && tv && tm && te && action && reward && discount && terminal &&
                       out_loss && out_y && out_abs_delta && dv && dm && de,
                   "pfrl_naf_td_loss: null pointer");
    PFRL_CHECK_ARG(n == 1 || (c && tc && dc), "pfrl_naf_td_loss: n > 1 needs c, tc and dc");
    PFRL_CHECK_ARG((half_width == nullptr) == (centre == nullptr),
                   "pfrl_naf_td_loss: half_width and centre go together");
    NafArgs a{v,      m,        e,        c,       tv,         tm,     te,  tc,   m2,
              action, reward,   discount, terminal, weights,   half_width, centre, low, high,
              out_loss, out_y,  out_abs_delta, dv, dm,         de,     dc};
#define CALL_NAF(NB, WAVES)                                                                        \
    hipLaunchKernelGGL((k_naf_td_loss<NB, WAVES>), dim3(1), dim3(64 * WAVES), 0, (hipStream_t)stream, \
                       a, (int)B, (int)n, clip_delta, mean)
    if (n <= 4)
        CALL_NAF(4, 16);
    else if (n <= 8)
        CALL_NAF(8, 8);
    else if (n <= 16)
        CALL_NAF(16, 8);
    else
        CALL_NAF(32, 4);
#undef CALL_NAF
    PFRL_LAUNCH_CHECK();
}
