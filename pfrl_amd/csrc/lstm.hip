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
// memory straight into the MFMA B operand: lane (c = lane & 15, kq = lane >> 4) loads the four
// floats k0 + 4 kq .. + 3 of gate row c as ONE 16-byte load, and MFMA step i of the block takes
// element i of every lane's four for BOTH operands (any bijection of k serves a reduction).  x / h0
// rows are loaded the same way into the A operand; every workgroup re-reads them (467 KB at
// N = 32), which stays in L2.  All loads of UNR blocks are issued before the first MFMA of the trip.
// LDS holds only the partial tiles: [16 waves][16 MT rows][17] floats, folded in wave order by the
// thread that then runs the cell update of its (row, unit): no atomics, no second launch, no gates
// tensor in HBM, the same bits on every launch.
//
// Tails are the kernel's: columns beyond I / H enter as zeros (clamped address, masked value), rows
// beyond N and units beyond H repeat the last valid one and are not stored.
#include "common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// Packed fp32 arithmetic (two floats per VALU op) is switched off for this kernel, in the source so
// that every build path agrees: the compiler emits none here today, and the fixed-order sums below
// are not to change form with a compiler that would.
#if defined(__HIP_DEVICE_COMPILE__)
#define PFRL_NO_PACKED_FP32 __attribute__((target("no-packed-fp32-ops")))
#else
#define PFRL_NO_PACKED_FP32
#endif

constexpr int kUnits = 4;           // hidden units of a workgroup (16 gate columns)
constexpr int kWaves = 16;          // waves of a workgroup, each a share of the reduction
constexpr int kRowsPerWg = 64;      // 4 M-tiles
constexpr int kMaxRows = 256;       // blockIdx.y <= 4: the admitted envelope
constexpr int kPad = 17;            // LDS row stride of a partial tile

struct LstmArgs {
    const float *x, *h0, *c0, *w_ih, *w_hh, *b_ih, *b_hh;
    float *h1, *c1, *y;
    int N, I, H;
};

// Four consecutive floats k .. k + 3 of a matrix row of K columns; addresses beyond the row are
// clamped into it and the caller zeroes those elements when it uses them (a select next to the load
// would wait for it).  VEC: K % 4 == 0 and the row starts on 16 bytes (k is always a multiple of 4),
// so the four are in or out together.
template <bool VEC>
__device__ __forceinline__ float4 load4(const float *__restrict__ row, int k, int K) {
    if (VEC) return *reinterpret_cast<const float4 *>(row + min(k, K - 4));
    return make_float4(row[min(k, K - 1)], row[min(k + 1, K - 1)], row[min(k + 2, K - 1)],
                       row[min(k + 3, K - 1)]);
}

__device__ __forceinline__ float sigmoidf(float v) { return 1.f / (1.f + expf(-v)); }

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
#pragma unroll
    for (int t = 0; t < MT; ++t) arow[t] = (unsigned)min(row0 + 16 * t + c16, N - 1);

    const int nb0 = (I + 15) >> 4, nb = nb0 + (a.h0 != nullptr ? (H + 15) >> 4 : 0);
    const int b_begin = wave * nb / kWaves, b_end = (wave + 1) * nb / kWaves;
    f32x4 acc[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int b = b_begin; b < b_end; b += UNR) {
        float4 w[UNR], v[UNR][MT];
        int left[UNR];                                     // columns of the row from this lane's k on
#pragma unroll
        for (int j = 0; j < UNR; ++j) {
            const int bb = min(b + j, b_end - 1);          // (clamped: a short last trip repeats, as zeros)
            const bool hh = bb >= nb0;                     // (uniform) which part of the concatenated range
            const int K = hh ? H : I, k = 16 * (bb - (hh ? nb0 : 0)) + 4 * kq;
            const float *__restrict__ wm = hh ? a.w_hh : a.w_ih;
            const float *__restrict__ am = hh ? a.h0 : a.x;
            left[j] = b + j < b_end ? K - k : 0;
            w[j] = load4<VEC>(wm + (size_t)grow * K, k, K);
#pragma unroll
            for (int t = 0; t < MT; ++t) v[j][t] = load4<VEC>(am + (size_t)arow[t] * K, k, K);
        }
#pragma unroll
        for (int j = 0; j < UNR; ++j) {
            // (no branch round a block: the loads of a block behind one would sink into it)
            const float wv[4] = {left[j] > 0 ? w[j].x : 0.f, left[j] > 1 ? w[j].y : 0.f,
                                 left[j] > 2 ? w[j].z : 0.f, left[j] > 3 ? w[j].w : 0.f};
#pragma unroll
            for (int t = 0; t < MT; ++t) {
                const float av[4] = {left[j] > 0 ? v[j][t].x : 0.f, left[j] > 1 ? v[j][t].y : 0.f,
                                     left[j] > 2 ? v[j][t].z : 0.f, left[j] > 3 ? v[j][t].w : 0.f};
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], wv[i], acc[t], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i)       // accumulator layout: row = 4 (lane >> 4) + i, column = lane & 15
            part[wave][16 * t + 4 * kq + i][c16] = acc[t][i];
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
        float s = part[0][r][4 * q + u];
#pragma unroll
        for (int wv = 1; wv < kWaves; ++wv) s += part[wv][r][4 * q + u];
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

template <int MT, int UNR>
void launch(const LstmArgs &a, bool vec, dim3 grid, hipStream_t st) {
    if (vec)
        hipLaunchKernelGGL((k_lstm_cell_fwd<MT, UNR, true>), grid, dim3(kWaves * 64), 0, st, a);
    else
        hipLaunchKernelGGL((k_lstm_cell_fwd<MT, UNR, false>), grid, dim3(kWaves * 64), 0, st, a);
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

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
    if (N <= 16)
        launch<1, 4>(a, vec, grid, st);
    else if (N <= 32)
        launch<2, 4>(a, vec, grid, st);
    else
        launch<4, 2>(a, vec, grid, st);
    PFRL_LAUNCH_CHECK();
}
