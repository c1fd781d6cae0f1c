// The recurrence of a whole packed GRU sequence, forward and backward, as one launch per time step
// (the update path of recurrent PPO and of the other recurrent agents; csrc/gru.hip is the acting
// step).  torch.nn.GRU, one layer, gate order (r, z, n), f32.  The rows are a PackedSequence's:
// time-major, n_0 >= n_1 >= ... >= n_{T-1} >= 1 rows per step, step t starting at row off_t.  The
// caller does what can be batched as library GEMMs: P = X W_ih^T + b_ih + [b_hr, b_hz, 0] over all
// rows, and the weight and input gradients.  b_hn cannot go into P, because the reset gate scales
// it: it comes here as its own [H] vector.  What is here is the part that cannot be batched:
//     forward  t = 0 .. T-1:  s = h_{t-1} W_hh^T;  r = sig(P_r + s_r), z = sig(P_z + s_z),
//                             q = s_n + b_hn, n = tanh(P_n + r q), h_t = (1 - z) n + z h_{t-1}
//     backward s = T .. 0:    dh_{s-1} = dY_{s-1} + dQ_s W_hh + dh_s z_s, then the pointwise gradient
// The stream orders the launches: no grid-wide barrier, no persistent workgroups.
//
// Forward step (k_gru_seq_step_fwd).  A workgroup owns 4 hidden units and the 12 gate columns
// c = 4 gate + unit of one 16x16x4 MFMA N-tile; columns 12 .. 15 are idle, their lanes load nothing
// and feed zeros.  5 units would fill 15 columns, but: the launch is one trip of loads long, not
// MFMA-bound, so the idle quarter of the matrix unit costs no time; the idle lanes fetch nothing, so
// it costs no bytes; 4 divides H = 512 into 128 equal workgroups (5 gives 103, the last one with 2
// units, and 25 % more bytes per workgroup on the critical path of each); and (row, unit) stays a
// shift and a mask.  No timing of the 5-unit form was taken.  The reduction is h_{t-1} W_hh^T only:
// ceil(H / 16) blocks, 32 at H = 512, over 8 waves = ONE trip of 4 blocks each, W_hh (3 MB at
// H = 512, resident in L2 / MALL across the T launches) straight into the B operand, 16 bytes per
// lane where H % 4 == 0 and the bases are aligned.  Partial tiles fold through LDS in wave order and
// the folding thread runs the gate arithmetic: y, for training the four saved values (r, z, n, q:
// 4H floats a row, what the backward needs and no more), and hn for rows that end at this step.
// With h0 == NULL the first step has no reduction at all.
//
// Backward step (k_gru_seq_step_bwd).  A workgroup owns 16 hidden units j, one N-tile of dh.  (a)
// red[n][j] = sum_k dQ_s[n][k] W_hh[k][j] over K = 3H (96 blocks at H = 512: 16 waves, 6 blocks
// each, two trips of 3, so kUnrBwd = 3 where the LSTM's 4H wanted 4), W_hh read column-wise, four
// dword loads per lane whose 16 lanes of a k read 64 contiguous bytes; no transposed copy of the
// weights exists.  The reduction runs on the f64 16x16x4 MFMA, operands widened at the MFMA,
// partial tiles and fold in f64, ONE rounding to f32 per element: dh feeds every earlier step, as in
// csrc/lstm_seq.hip, where f32 accumulation missed the accuracy rule.  (b) the thread that folded
// (row, unit) goes on, in the same launch, to the pointwise gradient of step s - 1:
//     dh = dY + (red + carry  |  dhn for a row that ends here),   carry' = dh z
//     da_n = dh (1 - z)(1 - n^2),  da_z = dh (h_prev - n) z (1 - z),  da_r = da_n q r (1 - r)
// The direct term dh z has no LSTM counterpart in dh (there it is the cell's): it travels in a
// [n_0, H] carry buffer and ends, with the last reduction, as dh0.
// Two gradient arrays are written, dP = [da_r, da_z, da_n] and dQ = [da_r, da_z, da_n r], both
// [R, 3H] in full.  Storing r and z once (dQ plus a bare da_n block) would save two dword stores per
// element here and cost the caller a second GEMM launch for each of dX and dW_ih plus a
// concatenation for db_ih: not free, so not done.
//
// Load form, tails and fold order are csrc/recurrent_mfma.h's: no atomics, one fixed order of every
// sum, the same inputs give the same bits on every launch.
#include "recurrent_mfma.h"

namespace {

constexpr int kFwdUnits = 4;        // hidden units of a forward workgroup (12 of 16 columns)
constexpr int kFwdWaves = 8;
constexpr int kUnrFwd = 4;          // blocks of 16 k per load trip
constexpr int kBwdUnits = 16;       // hidden units of a backward workgroup (16 columns of dh)
constexpr int kBwdWaves = 16;
constexpr int kUnrBwd = 3;

struct SeqFwdArgs {
    const float *p, *hprev, *w_hh, *b_hn;      // p: rows of this step; hprev: of the step before (or h0, or NULL)
    float *y, *saved, *hn;                     // y [.][H], saved [.][4H] (r, z, n, q) or NULL; hn [n_0][H]
    int n, n_next, H;                          // rows of this step and of the next (0 after the last)
};

struct SeqBwdArgs {
    const float *dq_s, *w_hh;                  // dQ rows of step s (NULL at s = T)
    const float *dy, *dhn, *saved, *hprev;     // dy, saved: rows of step s - 1; hprev: y rows of s - 2, h0 or NULL
    float *dp_prev, *dq_prev, *carry, *dh0;    // rows of step s - 1; [n_0][H]; written at s = 0
    int n_s, n_prev, H;                        // rows of step s (0 at s = T) and s - 1 (0 at s = 0)
};

template <int MT, bool VEC>
__global__ __launch_bounds__(kFwdWaves * 64) PFRL_NO_PACKED_FP32 void k_gru_seq_step_fwd(SeqFwdArgs a) {
    __shared__ float part[kFwdWaves][MT * 16][kPad];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int c16 = lane & 15, kq = lane >> 4, gate = c16 >> 2;
    const int N = a.n, H = a.H;
    const int j0 = blockIdx.x * kFwdUnits, row0 = blockIdx.y * kRowsPerWg;
    const unsigned grow = (unsigned)(min(gate, 2) * H + min(j0 + (c16 & 3), H - 1));   // this lane's gate row
    unsigned arow[MT];                                                                // ... and its h rows
    clamp_rows(arow, row0, c16, N - 1);

    const int nb = a.hprev != nullptr ? (H + 15) >> 4 : 0;      // no carried state: no reduction at all
    const int b_begin = share_begin<kFwdWaves>(wave, nb), b_end = share_begin<kFwdWaves>(wave + 1, nb);
    f32x4 acc[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int b = b_begin; b < b_end; b += kUnrFwd) {
        float4 w[kUnrFwd], v[kUnrFwd][MT];
        int left[kUnrFwd];
#pragma unroll
        for (int j = 0; j < kUnrFwd; ++j) {
            const int k = 16 * min(b + j, b_end - 1) + 4 * kq;   // (a short last trip repeats, as zeros)
            left[j] = b + j < b_end ? H - k : 0;
            w[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (gate < 3) w[j] = load4<VEC>(a.w_hh + (size_t)grow * H, k, H);     // (columns 12 .. 15: idle)
#pragma unroll
            for (int t = 0; t < MT; ++t) v[j][t] = load4<VEC>(a.hprev + (size_t)arow[t] * H, k, H);
        }
        mfma_trip(acc, w, v, left);
    }
#pragma unroll
    for (int t = 0; t < MT; ++t) store_partial(part, wave, t, acc[t], c16, kq);
    __syncthreads();

    // one thread per (row, unit): the three hidden-side sums folded in wave order, then the gate arithmetic
    const int e = threadIdx.x;
    if (e >= MT * 16 * kFwdUnits) return;
    const int r = e >> 2, u = e & 3;
    const int n = row0 + r, j = j0 + u;
    if (n >= N || j >= H) return;
    float s[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) s[q] = fold_waves(part, r, 4 * q + u);
    const float *__restrict__ pr = a.p + (size_t)n * 3 * H + j;
    const size_t o = (size_t)n * H + j;
    const float gr = sigmoidf(pr[0] + s[0]), gz = sigmoidf(pr[H] + s[1]);
    const float q = a.b_hn != nullptr ? s[2] + a.b_hn[j] : s[2];
    const float gn = tanhf(pr[2 * H] + gr * q);
    const float h1 = a.hprev != nullptr ? (1.f - gz) * gn + gz * a.hprev[o] : (1.f - gz) * gn;
    a.y[o] = h1;
    if (a.saved != nullptr) {             // training: what the backward step reads
        float *__restrict__ sr = a.saved + (size_t)n * 4 * H + j;
        sr[0] = gr, sr[H] = gz, sr[2 * H] = gn, sr[3 * H] = q;
    }
    if (n >= a.n_next) a.hn[o] = h1;      // this row's sequence ends here
}

template <int MT, bool VEC>
__global__ __launch_bounds__(kBwdWaves * 64) PFRL_NO_PACKED_FP32 void k_gru_seq_step_bwd(SeqBwdArgs a) {
    __shared__ double part[kBwdWaves][MT * 16][kPad];
    constexpr int UNR = MT == 4 && !VEC ? 2 : kUnrBwd;         // (64 rows of scalar loads: 3 blocks in flight would spill)
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int c16 = lane & 15, kq = lane >> 4;
    const int Ns = a.n_s, Np = a.n_prev, H = a.H, K = 3 * a.H;
    const int j0 = blockIdx.x * kBwdUnits, row0 = blockIdx.y * kRowsPerWg;
    const int bcol = min(j0 + c16, H - 1);                      // this lane's column of W_hh
    unsigned arow[MT];                                          // ... and its dQ rows
    clamp_rows(arow, row0, c16, max(Ns - 1, 0));                // (s = T has no rows and no reduction)

    // (a) red = dQ_s W_hh: K = 3H over the waves, accumulated in f64 (see the head of the file)
    const int nb = Ns > 0 ? (K + 15) >> 4 : 0;
    const int b_begin = share_begin<kBwdWaves>(wave, nb), b_end = share_begin<kBwdWaves>(wave + 1, nb);
    f64x4 acc[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[t] = f64x4{0., 0., 0., 0.};
    for (int b = b_begin; b < b_end; b += UNR) {
        float4 w[UNR], v[UNR][MT];
        int left[UNR];
#pragma unroll
        for (int j = 0; j < UNR; ++j) {
            const int k = 16 * min(b + j, b_end - 1) + 4 * kq;
            left[j] = b + j < b_end ? K - k : 0;
            const float *__restrict__ wc = a.w_hh + bcol;
            w[j] = make_float4(wc[(size_t)min(k, K - 1) * H], wc[(size_t)min(k + 1, K - 1) * H],
                               wc[(size_t)min(k + 2, K - 1) * H], wc[(size_t)min(k + 3, K - 1) * H]);
#pragma unroll
            for (int t = 0; t < MT; ++t) v[j][t] = load4<VEC>(a.dq_s + (size_t)arow[t] * K, k, K);
        }
        mfma_trip(acc, w, v, left);
    }
#pragma unroll
    for (int t = 0; t < MT; ++t) store_partial(part, wave, t, acc[t], c16, kq);
    __syncthreads();

    // one thread per (row, unit): red folded in wave order and rounded once, then (b) the gradient of step s - 1
    const int e = threadIdx.x;
    const int r = e >> 4, u = e & 15;
    if (r >= MT * 16) return;
    const int n = row0 + r, j = j0 + u;
    if (j >= H) return;
    const float red = (float)fold_waves(part, r, u);
    const size_t o = (size_t)n * H + j;
    if (Np == 0) {                        // s = 0: the reduction plus the direct term is the initial state's gradient
        if (n < Ns) a.dh0[o] = red + a.carry[o];
        return;
    }
    if (n >= Np) return;
    // a row whose sequence goes on at step s takes what step s sent back, one that ends here dhn
    const float dh = a.dy[o] + (n < Ns ? red + a.carry[o] : a.dhn != nullptr ? a.dhn[o] : 0.f);
    const float *__restrict__ sr = a.saved + (size_t)n * 4 * H + j;
    const float gr = sr[0], gz = sr[H], gn = sr[2 * H], q = sr[3 * H];
    const float hp = a.hprev != nullptr ? a.hprev[o] : 0.f;
    const float da_n = dh * (1.f - gz) * (1.f - gn * gn);
    const float da_z = dh * (hp - gn) * (gz * (1.f - gz));
    const float da_r = da_n * q * (gr * (1.f - gr));
    float *__restrict__ dp = a.dp_prev + (size_t)n * 3 * H + j, *__restrict__ dq = a.dq_prev + (size_t)n * 3 * H + j;
    dp[0] = da_r, dp[H] = da_z, dp[2 * H] = da_n;
    dq[0] = da_r, dq[H] = da_z, dq[2 * H] = da_n * gr;
    a.carry[o] = dh * gz;
}

const char *const kTooLarge = "2^31 saved or weight elements or more";

}  // namespace

extern "C" int pfrl_gru_seq_fwd(const float *p, const float *h0, const float *w_hh, const float *b_hn,
                                float *y, float *saved, float *hn, const int32_t *batch_sizes, int32_t T,
                                int32_t H, void *stream) {
    PFRL_CHECK_ARG(p && w_hh && y && hn, "pfrl_gru_seq_fwd: null pointer");
    std::vector<int64_t> off;
    const char *bad = check_sizes(batch_sizes, T, H, 3, kTooLarge, off);
    PFRL_CHECK_ARG(bad == nullptr, bad);
    hipStream_t st = (hipStream_t)stream;
    for (int t = 0; t < T; ++t) {
        const int n = batch_sizes[t];
        const float *hprev = t > 0 ? y + off[t - 1] * H : h0;
        const SeqFwdArgs a{p + off[t] * 3 * H, hprev, w_hh, b_hn, y + off[t] * H,
                           saved != nullptr ? saved + off[t] * 4 * H : nullptr, hn,
                           n, t + 1 < T ? batch_sizes[t + 1] : 0, H};
        const bool vec = H % 4 == 0 && aligned16(w_hh) && aligned16(hprev);
        const dim3 grid((H + kFwdUnits - 1) / kFwdUnits, (n + kRowsPerWg - 1) / kRowsPerWg);
        with_tiles(n, vec, [&](auto mt, auto v) {
            hipLaunchKernelGGL((k_gru_seq_step_fwd<decltype(mt)::value, decltype(v)::value>), grid,
                               dim3(kFwdWaves * 64), 0, st, a);
        });
    }
    PFRL_LAUNCH_CHECK();
}

extern "C" int pfrl_gru_seq_bwd(const float *dy, const float *dhn, const float *w_hh, const float *saved,
                                const float *y, const float *h0, float *dp, float *dq, float *dh0,
                                float *carry, const int32_t *batch_sizes, int32_t T, int32_t H,
                                void *stream) {
    PFRL_CHECK_ARG(dy && w_hh && saved && y && dp && dq && carry, "pfrl_gru_seq_bwd: null pointer");
    std::vector<int64_t> off;
    const char *bad = check_sizes(batch_sizes, T, H, 3, kTooLarge, off);
    PFRL_CHECK_ARG(bad == nullptr, bad);
    hipStream_t st = (hipStream_t)stream;
    const bool vec = H % 4 == 0 && aligned16(dq);               // (then every dQ row of 3H floats starts on 16 bytes)
    for (int s = T; s >= (dh0 != nullptr ? 0 : 1); --s) {
        const int n_s = s < T ? batch_sizes[s] : 0, n_prev = s > 0 ? batch_sizes[s - 1] : 0;
        const int64_t op = s > 0 ? off[s - 1] : 0;             // first row of step s - 1
        const SeqBwdArgs a{s < T ? dq + off[s] * 3 * H : nullptr, w_hh, dy + op * H, dhn, saved + op * 4 * H,
                           s > 1 ? y + off[s - 2] * H : h0, dp + op * 3 * H, dq + op * 3 * H, carry, dh0,
                           n_s, n_prev, H};
        const int rows = s > 0 ? n_prev : n_s;
        const dim3 grid((H + kBwdUnits - 1) / kBwdUnits, (rows + kRowsPerWg - 1) / kRowsPerWg);
        with_tiles(rows, vec, [&](auto mt, auto v) {
            hipLaunchKernelGGL((k_gru_seq_step_bwd<decltype(mt)::value, decltype(v)::value>), grid,
                               dim3(kBwdWaves * 64), 0, st, a);
        });
    }
    PFRL_LAUNCH_CHECK();
}
