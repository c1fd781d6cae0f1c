// One LSTM time step as ONE launch (the acting path of the recurrent agents): for N rows, in
// torch.nn.LSTM's gate order (i, f, g, o),
//     gates = x W_ih^T + h0 W_hh^T + b_ih + b_hh        x [N, I], h0 / c0 [N, H], W_ih [4H, I], W_hh [4H, H]
//     c1 = sigmoid(f) c0 + sigmoid(i) tanh(g),   h1 = sigmoid(o) tanh(c1)
// At the DRQN shape (I = 3136, H = 512, N = 32) this is a skinny GEMM over 29.9 MB of weights
// followed by a few thousand pointwise operations: memory-bound, so the design is about streaming
// the weights once and keeping many bytes in flight.
//
// Split.  A workgroup owns U = 4 hidden units and the 16 gate rows (4 gates x 4 units) that belong
// to them: exactly one MFMA N-tile, column c = 4 * gate + unit.  Its 16 waves share ONE reduction,
// the I columns of x against W_ih followed by the H columns of h0 against W_hh, in blocks of 16 k;
// wave w takes blocks [w nb / 16, (w + 1) nb / 16).  Each wave keeps the accumulators of all MT
// (1, 2 or 4) M-tiles of 16 rows that the workgroup serves; rows beyond 64 go to blockIdx.y, whose
// workgroups read the same weights again (from L2 / MALL when they run together).
//
// Data movement.  Every weight element is used by one workgroup only, so it goes from global
// memory straight into the MFMA B operand, gate row c of lane (c, kq), in the load form of
// csrc/recurrent_mfma.h; x / h0 rows are loaded the same way into the A operand; every workgroup
// re-reads them (467 KB at N = 32), which stays in L2.  LDS holds only the partial tiles:
// [16 waves][16 MT rows][17] floats, folded in wave order by the thread that then runs the cell
// update of its (row, unit): no atomics, no second launch, no gates tensor in HBM, the same bits on
// every launch.
//
// Tails are the kernel's, by the rules of csrc/recurrent_mfma.h (columns beyond I / H, rows beyond
// N, units beyond H).
#include "recurrent_mfma.h"

namespace {

constexpr int kUnits = 4;           // hidden units of a workgroup (16 gate columns)
constexpr int kWaves = 16;          // waves of a workgroup, each a share of the reduction

struct LstmArgs {
    const float *x, *h0, *c0, *w_ih, *w_hh, *b_ih, *b_hh;
    float *h1, *c1, *y;
    int N, I, H;
};

template <int MT, int UNR, bool VEC>
__global__ __launch_bounds__(kWaves * 64) PFRL_NO_PACKED_FP32 void k_lstm_cell_fwd(LstmArgs a) {
    __shared__ float part[kWaves][MT * 16][kPad];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int c16 = lane & 15, kq = lane >> 4;
    const int N = a.N, I = a.I, H = a.H;
    const int j0 = blockIdx.x * kUnits, row0 = blockIdx.y * kRowsPerWg;
    // element offsets fit 32 bits (the entry checks 4 H max(I, H) and N max(I, H) against 2^31)
    const unsigned grow = (unsigned)((c16 >> 2) * H + min(j0 + (c16 & 3), H - 1));   // this lane's gate row
    unsigned arow[MT];                                                              // ... and its x / h0 rows
    clamp_rows(arow, row0, c16, N - 1);

    f32x4 acc[MT];
    reduce_concat<kWaves, UNR, VEC>(acc, a.x, a.h0, a.w_ih, a.w_hh, I, H, grow, arow, wave, kq,
                                    [](bool) { return true; });
#pragma unroll
    for (int t = 0; t < MT; ++t) store_partial(part, wave, t, acc[t], c16, kq);
    __syncthreads();

    // one thread per (row, unit): the four gates folded in wave order, then the cell update
    const int e = threadIdx.x;
    if (e >= MT * 16 * kUnits) return;
    const int r = e >> 2, u = e & 3;
    const int n = row0 + r, j = j0 + u;
    if (n >= N || j >= H) return;
    float g[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        float s = fold_waves(part, r, 4 * q + u);
        if (a.b_ih != nullptr) s += a.b_ih[q * H + j];
        if (a.b_hh != nullptr) s += a.b_hh[q * H + j];
        g[q] = s;
    }
    const size_t o = (size_t)n * H + j;
    const float ig = sigmoidf(g[0]) * tanhf(g[2]);
    const float c1 = a.c0 != nullptr ? sigmoidf(g[1]) * a.c0[o] + ig : ig;
    a.c1[o] = c1;
    const float h1 = sigmoidf(g[3]) * tanhf(c1);
    a.h1[o] = h1;
    if (a.y != nullptr) a.y[o] = h1;      // the step's output next to the carried state: two buffers, as nn.LSTM's
}

}  // namespace

extern "C" int pfrl_lstm_cell_fwd(const float *x, const float *h0, const float *c0, const float *w_ih,
                                  const float *w_hh, const float *b_ih, const float *b_hh, float *h1,
                                  float *c1, float *y, int32_t N, int32_t I, int32_t H, void *stream) {
    PFRL_CHECK_ARG(x && w_ih && w_hh && h1 && c1, "pfrl_lstm_cell_fwd: null pointer");
    PFRL_CHECK_ARG(N >= 1 && N <= kMaxRows && I >= 1 && H >= 1,
                   "pfrl_lstm_cell_fwd: 1 <= N <= 256 rows, at least one input and one hidden unit");
    const int64_t kmax = I > H ? I : H;
    PFRL_CHECK_ARG(4 * (int64_t)H * kmax < ((int64_t)1 << 31) && kMaxRows * kmax < ((int64_t)1 << 31),
                   "pfrl_lstm_cell_fwd: a weight matrix of 2^31 elements or more");
    const LstmArgs a{x, h0, c0, w_ih, w_hh, b_ih, b_hh, h1, c1, y, N, I, H};
    // 16-byte loads need every row of every operand to start on 16 bytes
    const bool vec = I % 4 == 0 && H % 4 == 0 && aligned16(x) && aligned16(w_ih) && aligned16(w_hh) &&
                     (h0 == nullptr || aligned16(h0));
    const dim3 grid((H + kUnits - 1) / kUnits, (N + kRowsPerWg - 1) / kRowsPerWg);
    hipStream_t st = (hipStream_t)stream;
    with_tiles(N, vec, [&](auto mt, auto v) {
        constexpr int MT = decltype(mt)::value, UNR = MT == 4 ? 2 : 4;     // blocks per load trip
        hipLaunchKernelGGL((k_lstm_cell_fwd<MT, UNR, decltype(v)::value>), grid, dim3(kWaves * 64), 0, st, a);
    });
    PFRL_LAUNCH_CHECK();
}
