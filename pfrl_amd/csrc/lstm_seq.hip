// The recurrence of a whole packed LSTM sequence, forward and backward, as one launch per time step
// (the update path of the recurrent agents; csrc/lstm.hip is the acting step).  torch.nn.LSTM, one
// layer, gate order (i, f, g, o), f32.  The rows are a PackedSequence's: time-major, n_0 >= n_1 >=
// ... >= n_{T-1} >= 1 rows per step, step t starting at row off_t = n_0 + ... + n_{t-1}.  The input
// projection P = X W_ih^T + b_ih + b_hh over all rows is one library GEMM done by the caller; what
// is here is the part that cannot be batched:
//     forward  t = 0 .. T-1:  a_t = P_t + h_{t-1} W_hh^T,  c_t = f c_{t-1} + i g,  h_t = o tanh(c_t)
//     backward s = T .. 0:    dh_{s-1} = dY_{s-1} + dA_s W_hh,  then the pointwise gradient dA_{s-1}
// Every step depends on the one before it, and the stream orders the launches: no grid-wide barrier,
// no persistent workgroups.
//
// Forward step (k_lstm_seq_step_fwd).  The cell kernel's ownership: a workgroup owns 4 hidden units,
// the 16 gate columns c = 4 gate + unit, one 16x16x4 MFMA N-tile, so the cell update is its epilogue
// and the pre-activations never reach memory.  The reduction is only h_{t-1} W_hh^T: ceil(H / 16)
// blocks of 16 k, 32 at H = 512.  8 waves take 4 blocks each there, which is ONE trip of 4 blocks:
// all loads of a wave are in flight before its first MFMA.  16 waves (the cell kernel's, sized for
// I + H = 3648 columns) would hold 2 blocks each, the same single trip with twice the partial tiles
// to write and fold; 4 waves would need 8 blocks in flight, 160 load registers at 64 rows.  W_hh
// goes from global memory (4 MB at H = 512, resident in L2 / MALL across the T launches) straight
// into the B operand, 16 bytes per lane where H % 4 == 0 and the bases are aligned, clamped scalar
// loads otherwise.  Partial tiles fold through LDS in wave order (8 x MT x 16 x 17 floats: 8.5 / 17
// / 34 KB for MT = 1 / 2 / 4).
//
// Backward step (k_lstm_seq_step_bwd).  A workgroup owns 16 hidden units j, one N-tile of dh.  (a)
// dh_prev[n][j] = sum_r dA_s[n][r] W_hh[r][j] over K = 4H (128 blocks at H = 512: 16 waves, 8 blocks
// each, two trips of 4), folded in LDS in wave order.  This reduction runs on the f64 16x16x4 MFMA, operands widened at
// the MFMA, partial tiles and fold in f64 (16 x MT x 16 x 17 doubles: 34 / 68 / 136 KB), ONE rounding to f32 per
// element: dh_prev feeds all four gate gradients of every earlier step, and with f32 accumulation dh0 erred up to
// 2.9 times what a sequential f32 sum does at H = 4.  Price: 12.5 -> 17.0 us per launch at H = 512, 32 rows.
// (b) the thread that folded (row, unit) goes on, in the same launch, to the pointwise gradient of
// step s - 1 for its element: everything it needs is per unit, and the next launch reads the
// finished dA rows as its A operand.  B operand: W_hh is read column-wise here, lane (c, kq) takes
// W_hh[(k0 + 4 kq + i) H + j0 + c], i = 0 .. 3, as four dword loads; the 16 lanes of a k read 64
// contiguous bytes, so every fetched sector is used in full, and every element is used by exactly
// one workgroup once.  A transpose through LDS would add a store, a barrier and a load per element
// for no reuse, so the loads stay direct.  No transposed copy of the weights exists anywhere.
//
// Load form, tails and fold order are csrc/recurrent_mfma.h's: no atomics, one fixed order of every
// sum, the same inputs give the same bits on every launch.
#include "recurrent_mfma.h"

namespace {

constexpr int kFwdUnits = 4;        // hidden units of a forward workgroup (16 gate columns)
constexpr int kFwdWaves = 8;
constexpr int kBwdUnits = 16;       // hidden units of a backward workgroup (16 columns of dh)
constexpr int kBwdWaves = 16;
constexpr int kUnr = 4;             // blocks of 16 k per load trip

struct SeqFwdArgs {
    const float *p, *hprev, *cprev, *w_hh;     // p, hprev, cprev: rows of this step / the step before
    float *y, *c, *g, *hn, *cn;                // y, c, g: rows of this step; hn, cn: [n_0][H]
    int n, n_next, H;                          // rows of this step and of the next (0 after the last)
};

struct SeqBwdArgs {
    const float *da_s, *w_hh;                  // dA rows of step s (NULL at s = T)
    const float *dy, *dhn, *dcn, *g, *c, *cprev;   // dy, g, c: rows of step s - 1; cprev: of s - 2
    float *da_prev, *dc_carry, *dh0;           // dA rows of step s - 1; [n_0][H]; written at s = 0
    int n_s, n_prev, H;                        // rows of step s (0 at s = T) and s - 1 (0 at s = 0)
};

template <int MT, bool VEC>
__global__ __launch_bounds__(kFwdWaves * 64) PFRL_NO_PACKED_FP32 void k_lstm_seq_step_fwd(SeqFwdArgs a) {
    __shared__ float part[kFwdWaves][MT * 16][kPad];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int c16 = lane & 15, kq = lane >> 4;
    const int N = a.n, H = a.H;
    const int j0 = blockIdx.x * kFwdUnits, row0 = blockIdx.y * kRowsPerWg;
    const unsigned grow = (unsigned)((c16 >> 2) * H + min(j0 + (c16 & 3), H - 1));   // this lane's gate row
    unsigned arow[MT];                                                              // ... and its h rows
    clamp_rows(arow, row0, c16, N - 1);

    const int nb = a.hprev != nullptr ? (H + 15) >> 4 : 0;      // no carried state: no reduction at all
    const int b_begin = share_begin<kFwdWaves>(wave, nb), b_end = share_begin<kFwdWaves>(wave + 1, nb);
    f32x4 acc[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int b = b_begin; b < b_end; b += kUnr) {
        float4 w[kUnr], v[kUnr][MT];
        int left[kUnr];
#pragma unroll
        for (int j = 0; j < kUnr; ++j) {
            const int k = 16 * min(b + j, b_end - 1) + 4 * kq;   // (a short last trip repeats, as zeros)
            left[j] = b + j < b_end ? H - k : 0;
            w[j] = load4<VEC>(a.w_hh + (size_t)grow * H, k, H);
#pragma unroll
            for (int t = 0; t < MT; ++t) v[j][t] = load4<VEC>(a.hprev + (size_t)arow[t] * H, k, H);
        }
        mfma_trip(acc, w, v, left);
    }
#pragma unroll
    for (int t = 0; t < MT; ++t) store_partial(part, wave, t, acc[t], c16, kq);
    __syncthreads();

    // one thread per (row, unit): the four gates folded in wave order, then the cell update
    const int e = threadIdx.x;
    if (e >= MT * 16 * kFwdUnits) return;
    const int r = e >> 2, u = e & 3;
    const int n = row0 + r, j = j0 + u;
    if (n >= N || j >= H) return;
    float g[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) g[q] = fold_waves(part, r, 4 * q + u) + a.p[(size_t)n * 4 * H + q * H + j];
    const size_t o = (size_t)n * H + j;
    const float gi = sigmoidf(g[0]), gf = sigmoidf(g[1]), gg = tanhf(g[2]), go = sigmoidf(g[3]);
    const float c1 = a.cprev != nullptr ? gf * a.cprev[o] + gi * gg : gi * gg;
    const float h1 = go * tanhf(c1);
    a.y[o] = h1;
    a.c[o] = c1;
    if (a.g != nullptr) {                 // training: the ACTIVATED gates, what the backward step reads
        float *__restrict__ gr = a.g + (size_t)n * 4 * H + j;
        gr[0] = gi, gr[H] = gf, gr[2 * H] = gg, gr[3 * H] = go;
    }
    if (n >= a.n_next) a.hn[o] = h1, a.cn[o] = c1;      // this row's sequence ends here
}

template <int MT>
__global__ __launch_bounds__(kBwdWaves * 64) PFRL_NO_PACKED_FP32 void k_lstm_seq_step_bwd(SeqBwdArgs a) {
    __shared__ double part[kBwdWaves][MT * 16][kPad];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int c16 = lane & 15, kq = lane >> 4;
    const int Ns = a.n_s, Np = a.n_prev, H = a.H, K = 4 * a.H;
    const int j0 = blockIdx.x * kBwdUnits, row0 = blockIdx.y * kRowsPerWg;
    const int bcol = min(j0 + c16, H - 1);                      // this lane's column of W_hh
    unsigned arow[MT];                                          // ... and its dA rows
    clamp_rows(arow, row0, c16, max(Ns - 1, 0));                // (s = T has no rows and no reduction)

    // (a) dh_prev = dA_s W_hh: K = 4H over the waves, accumulated in f64 (see the head of the file)
    const int nb = Ns > 0 ? (K + 15) >> 4 : 0;
    const int b_begin = share_begin<kBwdWaves>(wave, nb), b_end = share_begin<kBwdWaves>(wave + 1, nb);
    f64x4 acc[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[t] = f64x4{0., 0., 0., 0.};
    for (int b = b_begin; b < b_end; b += kUnr) {
        float4 w[kUnr], v[kUnr][MT];
        int left[kUnr];
#pragma unroll
        for (int j = 0; j < kUnr; ++j) {
            const int k = 16 * min(b + j, b_end - 1) + 4 * kq;
            left[j] = b + j < b_end ? K - k : 0;
            const float *__restrict__ wc = a.w_hh + bcol;
            w[j] = make_float4(wc[(size_t)min(k, K - 1) * H], wc[(size_t)min(k + 1, K - 1) * H],
                               wc[(size_t)min(k + 2, K - 1) * H], wc[(size_t)min(k + 3, K - 1) * H]);
#pragma unroll
            for (int t = 0; t < MT; ++t) v[j][t] = load4<true>(a.da_s + (size_t)arow[t] * K, k, K);   // (K = 4H: always 16-byte rows)
        }
        mfma_trip(acc, w, v, left);
    }
#pragma unroll
    for (int t = 0; t < MT; ++t) store_partial(part, wave, t, acc[t], c16, kq);
    __syncthreads();

    // one thread per (row, unit): dh_prev folded in wave order and rounded once, then (b) the gradient of step s - 1
    const int e = threadIdx.x;
    const int r = e >> 4, u = e & 15;
    if (r >= MT * 16) return;
    const int n = row0 + r, j = j0 + u;
    if (j >= H) return;
    const float dhp = (float)fold_waves(part, r, u);
    const size_t o = (size_t)n * H + j;
    if (Np == 0) {                        // s = 0: what is carried is the gradient of the initial state
        if (n < Ns) a.dh0[o] = dhp;       // (dc0 is dc_carry itself)
        return;
    }
    if (n >= Np) return;
    const bool carried = n < Ns;          // the row's sequence goes on at step s
    const float dh = a.dy[o] + (carried ? dhp : a.dhn != nullptr ? a.dhn[o] : 0.f);
    const float *__restrict__ gr = a.g + (size_t)n * 4 * H + j;
    const float gi = gr[0], gf = gr[H], gg = gr[2 * H], go = gr[3 * H];
    const float tc = tanhf(a.c[o]);
    const float dc = dh * go * (1.f - tc * tc) + (carried ? a.dc_carry[o] : a.dcn != nullptr ? a.dcn[o] : 0.f);
    const float cp = a.cprev != nullptr ? a.cprev[o] : 0.f;
    float *__restrict__ dr = a.da_prev + (size_t)n * 4 * H + j;
    dr[0] = dc * gg * (gi * (1.f - gi));
    dr[H] = dc * cp * (gf * (1.f - gf));
    dr[2 * H] = dc * gi * (1.f - gg * gg);
    dr[3 * H] = dh * tc * (go * (1.f - go));
    a.dc_carry[o] = dc * gf;
}

const char *const kTooLarge = "2^31 gate elements or more";

}  // namespace

extern "C" int pfrl_lstm_seq_fwd(const float *p, const float *h0, const float *c0, const float *w_hh,
                                 float *y, float *c, float *gates, float *hn, float *cn,
                                 const int32_t *batch_sizes, int32_t T, int32_t H, void *stream) {
    PFRL_CHECK_ARG(p && w_hh && y && c && hn && cn, "pfrl_lstm_seq_fwd: null pointer");
    std::vector<int64_t> off;
    const char *bad = check_sizes(batch_sizes, T, H, 4, kTooLarge, off);
    PFRL_CHECK_ARG(bad == nullptr, bad);
    hipStream_t st = (hipStream_t)stream;
    for (int t = 0; t < T; ++t) {
        const int n = batch_sizes[t];
        const float *hprev = t > 0 ? y + off[t - 1] * H : h0, *cprev = t > 0 ? c + off[t - 1] * H : c0;
        const SeqFwdArgs a{p + off[t] * 4 * H, hprev, cprev, w_hh, y + off[t] * H, c + off[t] * H,
                           gates != nullptr ? gates + off[t] * 4 * H : nullptr, hn, cn,
                           n, t + 1 < T ? batch_sizes[t + 1] : 0, H};
        const bool vec = H % 4 == 0 && aligned16(w_hh) && aligned16(hprev);
        const dim3 grid((H + kFwdUnits - 1) / kFwdUnits, (n + kRowsPerWg - 1) / kRowsPerWg);
        with_tiles(n, vec, [&](auto mt, auto v) {
            hipLaunchKernelGGL((k_lstm_seq_step_fwd<decltype(mt)::value, decltype(v)::value>), grid,
                               dim3(kFwdWaves * 64), 0, st, a);
        });
    }
    PFRL_LAUNCH_CHECK();
}

extern "C" int pfrl_lstm_seq_bwd(const float *dy, const float *dhn, const float *dcn, const float *w_hh,
                                 const float *gates, const float *c, const float *c0, float *da,
                                 float *dh0, float *dc0, const int32_t *batch_sizes, int32_t T,
                                 int32_t H, void *stream) {
    PFRL_CHECK_ARG(dy && w_hh && gates && c && da && dc0, "pfrl_lstm_seq_bwd: null pointer");
    std::vector<int64_t> off;
    const char *bad = check_sizes(batch_sizes, T, H, 4, kTooLarge, off);
    PFRL_CHECK_ARG(bad == nullptr, bad);
    hipStream_t st = (hipStream_t)stream;
    PFRL_CHECK_ARG(aligned16(da), "pfrl_lstm_seq_bwd: da must start on 16 bytes");   // (then every row of 4H floats does)
    for (int s = T; s >= (dh0 != nullptr ? 0 : 1); --s) {
        const int n_s = s < T ? batch_sizes[s] : 0, n_prev = s > 0 ? batch_sizes[s - 1] : 0;
        const int64_t op = s > 0 ? off[s - 1] : 0;             // first row of step s - 1
        const SeqBwdArgs a{s < T ? da + off[s] * 4 * H : nullptr, w_hh, dy + op * H, dhn, dcn,
                           gates + op * 4 * H, c + op * H, s > 1 ? c + off[s - 2] * H : c0,
                           da + op * 4 * H, dc0, dh0, n_s, n_prev, H};
        const int rows = s > 0 ? n_prev : n_s;
        const dim3 grid((H + kBwdUnits - 1) / kBwdUnits, (rows + kRowsPerWg - 1) / kRowsPerWg);
        with_tiles(rows, true, [&](auto mt, auto) {          // (dA rows are 4H floats: always 16-byte loads)
            hipLaunchKernelGGL((k_lstm_seq_step_bwd<decltype(mt)::value>), grid, dim3(kBwdWaves * 64), 0, st, a);
        });
    }
    PFRL_LAUNCH_CHECK();
}
