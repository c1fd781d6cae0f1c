// One GRU time step as ONE launch (the acting path of recurrent PPO and of every agent whose
// RecurrentSequential holds an nn.GRU): for N rows, in torch.nn.GRU's gate order (r, z, n),
//     r = sigmoid(W_ir x + b_ir + W_hr h + b_hr)        x [N, I], h [N, H], W_ih [3H, I], W_hh [3H, H]
//     z = sigmoid(W_iz x + b_iz + W_hz h + b_hz)
//     q = W_hn h + b_hn,   n = tanh(W_in x + b_in + r q),   h' = (1 - z) n + z h
// At the reference example's shape (I = H = 512, 8 to 32 rows) this is 6.3 MB of weights against a
// few thousand pointwise operations: memory-bound, and so short that one trip of loads is the whole
// launch.  The design is about fetching every weight byte exactly once, all of them in flight
// before the first MFMA.
//
// Why this is not the LSTM cell with three gates.  The reset gate multiplies the HIDDEN side of the
// candidate only, so W_in x and W_hn h cannot be summed in one accumulator column as the LSTM's
// x W_ih^T + h W_hh^T are: they have to arrive at the epilogue apart, and b_hn belongs to the second.
//
// Split.  A workgroup owns U = 4 hidden units and 16 accumulator columns c = 4 kind + unit, one
// 16x16x4 MFMA N-tile, with kind in {r, z, n_x, n_h}: the three gates fill the tile exactly because
// the candidate needs two columns.  The reduction range is the concatenation of the I columns of x
// and the H columns of h, in blocks of 16 k, shared by 16 waves: wave w takes blocks
// [w nb / 16, (w + 1) nb / 16), 4 each at I = H = 512, ONE trip.  Columns r and z reduce over the
// whole range (W_ih row, then W_hh row).  Column n_x reduces over the x blocks only and n_h over the
// h blocks only: in the other part their lanes issue NO load (the load is predicated on the lane's
// kind) and feed zeros to the MFMA, so the 3H (I + H) weights are fetched once each and nothing else
// is: a fourth "gate" of padding would cost a third more traffic on a kernel that is all traffic.
// Each wave keeps the accumulators of all MT (1, 2 or 4) M-tiles of 16 rows that the workgroup
// serves; rows beyond 64 go to blockIdx.y (the weights then come from L2 / MALL).
//
// Data movement.  A weight element is used by one workgroup once, so it goes from global memory
// straight into the MFMA B operand, the lane's gate row in the load form of csrc/recurrent_mfma.h.
// x / h rows go the same way into the A operand; every workgroup re-reads them (32 KB at 8 rows),
// which stays in L2.
// LDS holds only the partial tiles, [16 waves][16 MT rows][17] floats, folded in wave order by the
// thread that then runs the gate arithmetic of its (row, unit) and stores h' (twice where the caller
// wants the step's output next to the carried state): no gates tensor in HBM, no atomics, no
// scratch, no second launch, the same bits on every launch.  A wave that holds only h blocks adds
// exact zeros to n_x and the other way round, so the fold needs no case distinction.
//
// Tails are the kernel's, by the rules of csrc/recurrent_mfma.h (columns beyond I / H, rows beyond
// N, units beyond H); h0 == NULL drops the h blocks from the range altogether (n_h is then b_hn
// alone).
#include "recurrent_mfma.h"

namespace {

constexpr int kUnits = 4;           // hidden units of a workgroup (16 columns: r, z, n_x, n_h of each)
constexpr int kWaves = 16;          // waves of a workgroup, each a share of the reduction
enum { kR = 0, kZ = 1, kNx = 2, kNh = 3 };

struct GruArgs {
    const float *x, *h0, *w_ih, *w_hh, *b_ih, *b_hh;
    float *h1, *y;
    int N, I, H;
};

template <int MT, int UNR, bool VEC>
__global__ __launch_bounds__(kWaves * 64) PFRL_NO_PACKED_FP32 void k_gru_cell_fwd(GruArgs a) {
    __shared__ float part[kWaves][MT * 16][kPad];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int c16 = lane & 15, kq = lane >> 4, kind = c16 >> 2;
    const int N = a.N, I = a.I, H = a.H;
    const int j0 = blockIdx.x * kUnits, row0 = blockIdx.y * kRowsPerWg;
    // element offsets fit 32 bits (the entry checks 3 H max(I, H) and N max(I, H) against 2^31);
    // n_x and n_h are both gate 2, one in W_ih and one in W_hh
    const unsigned grow = (unsigned)(min(kind, 2) * H + min(j0 + (c16 & 3), H - 1));
    unsigned arow[MT];                                     // this lane's x / h0 rows
    clamp_rows(arow, row0, c16, N - 1);

    f32x4 acc[MT];
    // the candidate's two columns each own one part of the range: nothing is loaded in the other
    reduce_concat<kWaves, UNR, VEC>(acc, a.x, a.h0, a.w_ih, a.w_hh, I, H, grow, arow, wave, kq,
                                    [kind](bool hh) { return kind != (hh ? kNx : kNh); });
#pragma unroll
    for (int t = 0; t < MT; ++t) store_partial(part, wave, t, acc[t], c16, kq);
    __syncthreads();

    // one thread per (row, unit): the four columns folded in wave order, then the gate arithmetic
    const int e = threadIdx.x;
    if (e >= MT * 16 * kUnits) return;
    const int r = e >> 2, u = e & 3;
    const int n = row0 + r, j = j0 + u;
    if (n >= N || j >= H) return;
    float g[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        float s = fold_waves(part, r, 4 * q + u);
        // r and z take both biases, n_x only b_in, n_h only b_hn
        if (a.b_ih != nullptr && q != kNh) s += a.b_ih[q * H + j];
        if (a.b_hh != nullptr && q != kNx) s += a.b_hh[min(q, 2) * H + j];
        g[q] = s;
    }
    const size_t o = (size_t)n * H + j;
    const float gr = sigmoidf(g[kR]), gz = sigmoidf(g[kZ]), gn = tanhf(g[kNx] + gr * g[kNh]);
    const float h1 = a.h0 != nullptr ? (1.f - gz) * gn + gz * a.h0[o] : (1.f - gz) * gn;
    a.h1[o] = h1;
    if (a.y != nullptr) a.y[o] = h1;      // the step's output next to the carried state: two buffers, as nn.GRU's
}

}  // namespace

extern "C" int pfrl_gru_cell_fwd(const float *x, const float *h0, const float *w_ih, const float *w_hh,
                                 const float *b_ih, const float *b_hh, float *h1, float *y, int32_t N,
                                 int32_t I, int32_t H, void *stream) {
    PFRL_CHECK_ARG(x && w_ih && w_hh && h1, "pfrl_gru_cell_fwd: null pointer");
    PFRL_CHECK_ARG(N >= 1 && N <= kMaxRows && I >= 1 && H >= 1,
                   "pfrl_gru_cell_fwd: 1 <= N <= 256 rows, at least one input and one hidden unit");
    const int64_t kmax = I > H ? I : H;
    PFRL_CHECK_ARG(3 * (int64_t)H * kmax < ((int64_t)1 << 31) && kMaxRows * kmax < ((int64_t)1 << 31),
                   "pfrl_gru_cell_fwd: a weight matrix of 2^31 elements or more");
    const GruArgs a{x, h0, w_ih, w_hh, b_ih, b_hh, h1, y, N, I, H};
    // 16-byte loads need every row of every operand to start on 16 bytes
    const bool vec = I % 4 == 0 && H % 4 == 0 && aligned16(x) && aligned16(w_ih) && aligned16(w_hh) &&
                     (h0 == nullptr || aligned16(h0));
    const dim3 grid((H + kUnits - 1) / kUnits, (N + kRowsPerWg - 1) / kRowsPerWg);
    hipStream_t st = (hipStream_t)stream;
    with_tiles(N, vec, [&](auto mt, auto v) {
        constexpr int MT = decltype(mt)::value, UNR = MT == 4 ? 2 : 4;     // blocks per load trip
        hipLaunchKernelGGL((k_gru_cell_fwd<MT, UNR, decltype(v)::value>), grid, dim3(kWaves * 64), 0, st, a);
    });
    PFRL_LAUNCH_CHECK();
}
