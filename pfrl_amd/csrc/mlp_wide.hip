// Whole wide MLPs as one launch for gfx950: Linear(K, <= 512), act, Linear(<= 512, <= 512), act,
// Linear(<= 512, <= 64) of the replay actor-critic agents (pfrl's MuJoCo reproductions of SAC, TD3 and
// DDPG: 256-256 and 400-300 ReLU networks for the policy and the twin critics at B = 256), where a kernel
// per layer costs a launch floor each whatever it computes.  mlp.hip keeps every hidden layer's weights
// whole in LDS; a 256 x 256 f32 layer is 256 KB, so here the ACTIVATIONS are resident and the WEIGHTS
// stream.  Forward of one network, or of two of equal shapes on the same input, in one launch; the
// frozen-parameter backward (input gradient only, summed over the networks) in one launch.  Pointers
// travel by value, as in mlp.hip, so launches capture.  All products run on v_mfma_f32_16x16x4_f32.
//
// Forward (k_mlp_wide_fwd, 512 threads = 8 waves).  A workgroup owns a tile of 16 rows of one network
// (blockIdx.y picks the network).  The tile's activations for the whole width are in LDS (sA, 16 rows of
// 516 floats: 16-byte aligned rows, and 516 r + k maps the 16 lanes of a ds_read_b128 phase to different
// banks) as the A operand of the next layer: lane (c, kq) reads the four floats k0 + 4 kq .. + 3 of row c
// per block of 16 k and MFMA step i takes element i of both operands (recurrent_mfma.h's rule).  Weights
// are never resident: lane (c, kq) loads the same four k of weight row 16 ct + c straight from global
// memory / L2 into registers, as ONE 16-byte load where fan_in % 4 == 0 and the matrix starts on 16 bytes
// and as four clamped dword loads otherwise (393-float rows), for every column tile ct of its wave (tile
// ct goes to wave ct % 8: two tiles a wave at 256 wide, four at 512).  Two blocks are in flight: the loads
// of blocks b + 2 and b + 3 are issued behind the MFMAs of b and b + 1, before anything waits.  The first
// layer's x (one or two column blocks x1 | x2, rows of any alignment) goes through a double-buffered LDS
// stage in chunks of 128 k, the next chunk's global loads issued before the current chunk's MFMAs, so
// LDS use does not grow with K.  Widths that are no multiple of 16 and k tails are zeros in LDS (the A
// operand); weight addresses beyond a row or beyond the last row are clamped into the matrix and meet
// those zeros or land in columns that are not stored.  Every global load is bounds-checked or clamped.
// Once every accumulator of a layer is in registers (a barrier), bias and activation are applied in
// registers and written over sA in place; hidden activations reach HBM only through `save`.
// LDS: 33 024 (sA) + 16 896 (x stage) = 49 920 bytes, static.
// Every output element is ONE accumulator chain over k in ascending blocks of 16, elements 0 .. 3 of a
// block in order, with the same zero padding, in the one tile program there is: the bits of an output row
// depend on that row and the parameters only -- not on M, the row's position or n_nets.
//
// Input gradient (k_mlp_wide_dx, 256 threads = 4 waves).  A workgroup owns 16 rows and walks the networks
// in order.  d_l (16 rows, LDS, same layout as sA) is the A operand; the reduction of d_{l-1} = d_l W_l
// runs over W_l's ROWS n, so the weight operand is read in the other orientation, and the loads stay 16
// bytes wide by dealing the output columns instead: per block of 16 n, lane (c, q) takes rows n0 + 4 q + s
// (s = 0 .. 3, pairing with element s of its ds_read_b128 of d_l) and loads the four floats 64 g + 4 c ..
// + 3 of each; element e of those loads is the B operand of accumulator e, which therefore holds the 16
// output columns 64 g + 4 c' + e.  Four accumulators cover a group of 64 columns; group g goes to wave
// g % 4 (one group a wave at 256 wide, two at 512).  act'(a_{l-1}) comes from the saved activations, loaded
// before the MFMA loop, and d_{l-1} replaces d_l in LDS behind a barrier.  The last step, d_0 against
// W_0[:, col0 : col0 + ncol] (rows of any alignment, ncol <= 64), takes one 16-column tile per wave with
// dword loads, and its accumulators run on over the networks: network 0's terms first, no atomics, one
// order of every sum.  LDS: 33 024 bytes, static.
#include "mlp_common.h"

namespace {

constexpr int kRows = 16;              // rows of a workgroup's tile
constexpr int kMaxHidden = 512;
constexpr int kMaxLast = 64;
constexpr int kMaxK = 1024;            // K1 + K2
constexpr int kMaxM = 65536;
constexpr int kLdA = kMaxHidden + 4;   // LDS row stride of the activations
constexpr int kFwdThreads = 512, kFwdWaves = 8;
constexpr int kXChunk = 128;           // k columns of x per LDS trip (8 blocks)
constexpr int kLdX = kXChunk + 4;
constexpr int kDxThreads = 256, kDxWaves = 4;

struct WideFwdNet {
    const float *w[3], *b[3];
    float *save[2], *y;
};
struct WideFwdArgs {
    WideFwdNet net[2];
    int n[3];
};

struct WideDxNet {
    const float *w[3], *a[2], *dy;
};
struct WideDxArgs {
    WideDxNet net[2];
    int n[3];
};

// (uniform) rows of K floats from p on all start on 16 bytes: the 16-byte load form applies
__device__ __forceinline__ bool rows16(const float *p, int K) { return (K & 3) == 0 && ((uintptr_t)p & 15) == 0; }

// acc[j] += the block's four k: element i of the A fragment against element i of tile j's B fragment
template <int NT>
__device__ __forceinline__ void mma_block(f32x4 (&acc)[NT], const float4 &a, const float4 (&w)[NT]) {
    const float av[4] = {a.x, a.y, a.z, a.w};
    float wv[NT][4];
#pragma unroll
    for (int j = 0; j < NT; ++j) wv[j][0] = w[j].x, wv[j][1] = w[j].y, wv[j][2] = w[j].z, wv[j][3] = w[j].w;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) mfma_16x16x4(acc[j], av[i], wv[j][i]);
}

// The forward's B fragments of block b: the four floats 16 b + 4 kq .. + 3 of weight row wrow[j] (K columns)
template <int NT, bool VEC>
__device__ __forceinline__ void load_w(float4 (&w)[NT], const float *__restrict__ W, const unsigned (&wrow)[NT], int K,
                                       int b, int kq) {
#pragma unroll
    for (int j = 0; j < NT; ++j) w[j] = load4<VEC>(W + (size_t)wrow[j] * K, 16 * b + 4 * kq, K);
}

// Blocks [b_begin, b_end) of a layer of nb blocks: `a` is the lane's A fragment of block b_begin in LDS; wa / wb
// hold the B fragments of blocks b_begin and b_begin + 1 on entry and of b_end and b_end + 1 (clamped to the last
// block) on return.  b_end - b_begin is even except at the layer's end.
template <int NT, bool VEC>
__device__ __forceinline__ void run_blocks(f32x4 (&acc)[NT], float4 (&wa)[NT], float4 (&wb)[NT], const float *a,
                                           const float *__restrict__ W, const unsigned (&wrow)[NT], int K, int b_begin,
                                           int b_end, int nb, int kq) {
    for (int b = b_begin; b < b_end; b += 2, a += 32) {
        mma_block(acc, *reinterpret_cast<const float4 *>(a), wa);
        load_w<NT, VEC>(wa, W, wrow, K, min(b + 2, nb - 1), kq);
        if (b + 1 < b_end) mma_block(acc, *reinterpret_cast<const float4 *>(a + 16), wb);
        load_w<NT, VEC>(wb, W, wrow, K, min(b + 3, nb - 1), kq);
    }
}

// This thread's four elements of chunk c of the input tile ([16][128] of x1 | x2, zeros beyond M and K1 + K2)
__device__ __forceinline__ void load_x(float (&v)[4], const float *__restrict__ x1, const float *__restrict__ x2, int K1,
                                       int K2, int row0, int M, int c, int tid) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int idx = tid + kFwdThreads * t, r = idx >> 7, gc = kXChunk * c + (idx & 127);
        v[t] = gc < K1 ? stage_elem(x1, row0 + r, M, gc, K1, K1) : stage_elem(x2, row0 + r, M, gc - K1, K2, K2);
    }
}

__device__ __forceinline__ void store_x(float (*dst)[kLdX], const float (&v)[4], int tid) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int idx = tid + kFwdThreads * t;
        dst[idx >> 7][idx & 127] = v[t];
    }
}

// One layer of the forward: N outputs from K inputs (FIRST: x through the LDS stage; otherwise sA), bias and
// activation in registers, the result over sA in place (not for the last layer) and to `out` when given.
template <int NT, bool VEC, bool FIRST>
__device__ __forceinline__ void fwd_layer(float (*sA)[kLdA], float (*sX)[kRows][kLdX], const float *__restrict__ x1,
                                          const float *__restrict__ x2, int K1, int K2, const float *__restrict__ W,
                                          const float *__restrict__ bias, float *__restrict__ out, bool last, int act,
                                          int K, int N, int row0, int M, int tid) {
    const int lane = tid & 63, wave = tid >> 6, c16 = lane & 15, kq = lane >> 4;
    const int ntiles = (N + 15) >> 4, nb = (K + 15) >> 4;
    unsigned wrow[NT];
    float bv[NT];
    f32x4 acc[NT];
    float4 wa[NT], wb[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) wrow[j] = (unsigned)min(16 * (wave + kFwdWaves * j) + c16, N - 1);
    load_w<NT, VEC>(wa, W, wrow, K, 0, kq);
    load_w<NT, VEC>(wb, W, wrow, K, min(1, nb - 1), kq);
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        bv[j] = bias[wrow[j]];
        acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if (FIRST) {
        const int nch = (K + kXChunk - 1) / kXChunk;
        float xv[4];
        load_x(xv, x1, x2, K1, K2, row0, M, 0, tid);
        store_x(sX[0], xv, tid);
        __syncthreads();
        for (int c = 0; c < nch; ++c) {
            if (c + 1 < nch) load_x(xv, x1, x2, K1, K2, row0, M, c + 1, tid);
            run_blocks<NT, VEC>(acc, wa, wb, &sX[c & 1][c16][4 * kq], W, wrow, K, 8 * c, min(8 * c + 8, nb), nb, kq);
            if (c + 1 < nch) store_x(sX[(c + 1) & 1], xv, tid);
            __syncthreads();                                 // (chunk c has been read, chunk c + 1 is written)
        }
    } else {
        run_blocks<NT, VEC>(acc, wa, wb, &sA[c16][4 * kq], W, wrow, K, 0, nb, nb, kq);
        __syncthreads();                                     // (every wave has read the layer's input)
    }
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int ct = wave + kFwdWaves * j;
        if (ct >= ntiles) continue;
        const int col = 16 * ct + c16;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = 4 * kq + i;
            float v = acc[j][i] + bv[j];
            if (!last) {
                v = col < N ? activate(v, act) : 0.f;
                sA[r][col] = v;
            }
            if (out != nullptr && col < N && row0 + r < M) out[(size_t)(row0 + r) * N + col] = v;
        }
    }
    if (!last) __syncthreads();
}

template <bool FIRST>
__device__ __forceinline__ void fwd_dispatch(float (*sA)[kLdA], float (*sX)[kRows][kLdX], const float *x1, const float *x2,
                                             int K1, int K2, const float *W, const float *bias, float *out, bool last,
                                             int act, int K, int N, int row0, int M, int tid) {
    const int nt = (((N + 15) >> 4) + kFwdWaves - 1) / kFwdWaves;         // column tiles of the busiest wave
    const bool vec = rows16(W, K);
#define PFRL_WIDE_FWD(NT_)                                                                                             \
    if (vec)                                                                                                           \
        fwd_layer<NT_, true, FIRST>(sA, sX, x1, x2, K1, K2, W, bias, out, last, act, K, N, row0, M, tid);              \
    else                                                                                                               \
        fwd_layer<NT_, false, FIRST>(sA, sX, x1, x2, K1, K2, W, bias, out, last, act, K, N, row0, M, tid);
    if (nt == 1) {
        PFRL_WIDE_FWD(1)
    } else if (nt == 2) {
        PFRL_WIDE_FWD(2)
    } else if (nt == 3) {
        PFRL_WIDE_FWD(3)
    } else {
        PFRL_WIDE_FWD(4)
    }
#undef PFRL_WIDE_FWD
}

__global__ __launch_bounds__(kFwdThreads) PFRL_NO_PACKED_FP32 void k_mlp_wide_fwd(const float *__restrict__ x1,
                                                                                 const float *__restrict__ x2,
                                                                                 WideFwdArgs args, int M, int K1, int K2,
                                                                                 int L, int act) {
    __shared__ __attribute__((aligned(16))) float sA[kRows][kLdA];
    __shared__ __attribute__((aligned(16))) float sX[2][kRows][kLdX];
    const WideFwdNet &net = args.net[blockIdx.y];
    const int tid = threadIdx.x, row0 = blockIdx.x * kRows;
    fwd_dispatch<true>(sA, sX, x1, x2, K1, K2, net.w[0], net.b[0], net.save[0], false, act, K1 + K2, args.n[0], row0, M,
                       tid);
    for (int l = 1; l < L; ++l)
        fwd_dispatch<false>(sA, sX, x1, x2, K1, K2, net.w[l], net.b[l], l == L - 1 ? net.y : net.save[l], l == L - 1, act,
                            args.n[l - 1], args.n[l], row0, M, tid);
}

// The input gradient's B fragments of block b for NG column groups: row 16 b + 4 q + s of W (N rows of K floats),
// the four floats kcol[j] .. + 3
template <int NG, bool VEC>
__device__ __forceinline__ void load_wt(float4 (&w)[NG][4], const float *__restrict__ W, const int (&kcol)[NG], int N,
                                        int K, int b, int q) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const float *__restrict__ row = W + (size_t)min(16 * b + 4 * q + s, N - 1) * K;
#pragma unroll
        for (int j = 0; j < NG; ++j) w[j][s] = load4<VEC>(row, kcol[j], K);
    }
}

template <int NG>
__device__ __forceinline__ void mma_block_t(f32x4 (&acc)[NG][4], const float4 &a, const float4 (&w)[NG][4], bool second) {
    const float av[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int j = 0; j < NG; ++j) {
            if (j > 0 && !second) continue;                  // (uniform: a wave without a second group)
            mfma_16x16x4(acc[j][0], av[s], w[j][s].x);
            mfma_16x16x4(acc[j][1], av[s], w[j][s].y);
            mfma_16x16x4(acc[j][2], av[s], w[j][s].z);
            mfma_16x16x4(acc[j][3], av[s], w[j][s].w);
        }
}

// d_{l-1} = (d_l W) act'(a) over sD in place: N = d_l's width (the reduction), K = d_{l-1}'s; a is [M][K].
template <int NG, bool VEC>
__device__ __forceinline__ void dx_layer(float (*sD)[kLdA], const float *__restrict__ W, const float *__restrict__ a,
                                         int act, int N, int K, int row0, int M, int tid) {
    const int lane = tid & 63, wave = tid >> 6, c16 = lane & 15, q = lane >> 4;
    const int nb = (N + 15) >> 4, kpad = ((K + 15) >> 4) << 4;
    int kcol[NG];
    f32x4 acc[NG][4];
    float4 wa[NG][4], wb[NG][4], av[NG][4];
#pragma unroll
    for (int j = 0; j < NG; ++j) kcol[j] = 64 * (wave + kDxWaves * j) + 4 * c16;
    const bool second = NG > 1 && 64 * (wave + kDxWaves) < K;
    load_wt<NG, VEC>(wa, W, kcol, N, K, 0, q);
    load_wt<NG, VEC>(wb, W, kcol, N, K, min(1, nb - 1), q);
#pragma unroll
    for (int j = 0; j < NG; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            av[j][i] = load4<VEC>(a + (size_t)min(row0 + 4 * q + i, M - 1) * K, kcol[j], K);
            acc[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    const float *d = &sD[c16][4 * q];
    for (int b = 0; b < nb; b += 2, d += 32) {
        mma_block_t(acc, *reinterpret_cast<const float4 *>(d), wa, second);
        load_wt<NG, VEC>(wa, W, kcol, N, K, min(b + 2, nb - 1), q);
        if (b + 1 < nb) mma_block_t(acc, *reinterpret_cast<const float4 *>(d + 16), wb, second);
        load_wt<NG, VEC>(wb, W, kcol, N, K, min(b + 3, nb - 1), q);
    }
    __syncthreads();                                         // (every wave has read d_l)
#pragma unroll
    for (int j = 0; j < NG; ++j) {
        if (kcol[j] >= kpad) continue;                       // (kpad is a multiple of 4: a lane's four together)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float am[4] = {av[j][i].x, av[j][i].y, av[j][i].z, av[j][i].w};
            float4 v;
            v.x = kcol[j] + 0 < K ? act_grad(acc[j][0][i], am[0], act) : 0.f;
            v.y = kcol[j] + 1 < K ? act_grad(acc[j][1][i], am[1], act) : 0.f;
            v.z = kcol[j] + 2 < K ? act_grad(acc[j][2][i], am[2], act) : 0.f;
            v.w = kcol[j] + 3 < K ? act_grad(acc[j][3][i], am[3], act) : 0.f;
            *reinterpret_cast<float4 *>(&sD[4 * q + i][kcol[j]]) = v;
        }
    }
    __syncthreads();
}

__device__ __forceinline__ void dx_dispatch(float (*sD)[kLdA], const float *W, const float *a, int act, int N, int K,
                                            int row0, int M, int tid) {
    const bool vec = rows16(W, K) && rows16(a, K);
    if (K <= 64 * kDxWaves) {
        if (vec)
            dx_layer<1, true>(sD, W, a, act, N, K, row0, M, tid);
        else
            dx_layer<1, false>(sD, W, a, act, N, K, row0, M, tid);
    } else {
        if (vec)
            dx_layer<2, true>(sD, W, a, act, N, K, row0, M, tid);
        else
            dx_layer<2, false>(sD, W, a, act, N, K, row0, M, tid);
    }
}

// acc += d_0 W_0[:, col0 + 16 wave + c16] (N rows of K floats; the wave's 16-column tile), one block of dword
// loads ahead
__device__ __forceinline__ void dx_final(f32x4 &acc, const float (*sD)[kLdA], const float *__restrict__ W, int N, int K,
                                         int col, int c16, int q) {
    const int nb = (N + 15) >> 4;
    float wn[4], wc[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) wn[s] = W[(size_t)min(4 * q + s, N - 1) * K + col];
    const float *d = &sD[c16][4 * q];
    for (int b = 0; b < nb; ++b, d += 16) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            wc[s] = wn[s];
            wn[s] = W[(size_t)min(16 * (b + 1) + 4 * q + s, N - 1) * K + col];
        }
        const float4 a = *reinterpret_cast<const float4 *>(d);
        mfma_16x16x4(acc, a.x, wc[0]);
        mfma_16x16x4(acc, a.y, wc[1]);
        mfma_16x16x4(acc, a.z, wc[2]);
        mfma_16x16x4(acc, a.w, wc[3]);
    }
}

__global__ __launch_bounds__(kDxThreads) PFRL_NO_PACKED_FP32 void k_mlp_wide_dx(WideDxArgs args, float *__restrict__ dx,
                                                                               int M, int K, int L, int n_nets, int act,
                                                                               int col0, int ncol) {
    __shared__ __attribute__((aligned(16))) float sD[kRows][kLdA];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c16 = lane & 15, q = lane >> 4;
    const int row0 = blockIdx.x * kRows;
    const int last = args.n[L - 1];
    const bool tile = 16 * wave < ncol;                      // (uniform) this wave has a tile of dx
    const int col = col0 + min(16 * wave + c16, ncol - 1);
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < n_nets; ++k) {
        const WideDxNet &net = args.net[k];
        __syncthreads();                                     // (the previous network's d_0 has been read)
        stage<kDxThreads>(sD, net.dy, kRows, row0, M, 0, last, last, tid);
        __syncthreads();
        for (int l = L - 1; l >= 1; --l) dx_dispatch(sD, net.w[l], net.a[l - 1], act, args.n[l], args.n[l - 1], row0, M, tid);
        if (tile) dx_final(acc, sD, net.w[0], args.n[0], K, col, c16, q);
    }
    if (tile && 16 * wave + c16 < ncol) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = row0 + 4 * q + i;
            if (r < M) dx[(size_t)r * ncol + 16 * wave + c16] = acc[i];
        }
    }
}

// the envelope both entry points share
const char *check_wide(int32_t M, int32_t K, int32_t L, int32_t n_nets, const float *const *w, const int32_t *widths,
                       int32_t act) {
    if (M < 1 || M > kMaxM) return "1 <= M <= 65536";
    if (K < 1 || K > kMaxK) return "1 <= K1 + K2 <= 1024";
    if (L < 2 || L > 3) return "2 or 3 layers";
    if (n_nets < 1 || n_nets > 2) return "one or two networks";
    if (w == nullptr || widths == nullptr) return "null pointer";
    if (act != PFRL_MLP_TANH && act != PFRL_MLP_RELU) return "activation: tanh or ReLU";
    for (int l = 0; l < L; ++l) {
        const int lim = l == L - 1 ? kMaxLast : kMaxHidden;
        if (widths[l] < 1 || widths[l] > lim) return "hidden widths 1 .. 512, last width 1 .. 64";
        for (int k = 0; k < n_nets; ++k) {
            if (w[3 * k + l] == nullptr) return "null pointer";
            if (!aligned4(w[3 * k + l])) return "misaligned pointer";
        }
    }
    return nullptr;
}

}  // namespace

extern "C" int pfrl_mlp_wide_fwd(const float *x1, const float *x2, int32_t M, int32_t K1, int32_t K2, int32_t n_layers,
                                 int32_t n_nets, const float *const *w, const float *const *b, const int32_t *widths,
                                 int32_t act, float *const *save, float *const *y, void *stream) {
    if (n_nets == 0) return 0;
    PFRL_CHECK_ARG(K1 >= 1 && K2 >= 0, "pfrl_mlp_wide_fwd: K1 >= 1, K2 >= 0");
    const char *err = check_wide(M, K1 + K2, n_layers, n_nets, w, widths, act);
    PFRL_CHECK_ARG(err == nullptr, err);
    PFRL_CHECK_ARG(x1 != nullptr && aligned4(x1) && (K2 == 0 || (x2 != nullptr && aligned4(x2))),
                   "pfrl_mlp_wide_fwd: null or misaligned input");
    PFRL_CHECK_ARG(b != nullptr && y != nullptr, "pfrl_mlp_wide_fwd: null pointer");
    WideFwdArgs a{};
    for (int l = 0; l < n_layers; ++l) a.n[l] = widths[l];
    for (int k = 0; k < n_nets; ++k) {
        WideFwdNet &n = a.net[k];
        for (int l = 0; l < n_layers; ++l) {
            n.w[l] = w[3 * k + l];
            n.b[l] = b[3 * k + l];
            PFRL_CHECK_ARG(n.b[l] != nullptr && aligned4(n.b[l]), "pfrl_mlp_wide_fwd: null or misaligned bias");
        }
        for (int l = 0; l + 1 < n_layers; ++l) {
            n.save[l] = save != nullptr ? save[2 * k + l] : nullptr;
            PFRL_CHECK_ARG(aligned4(n.save[l]), "pfrl_mlp_wide_fwd: misaligned pointer");
        }
        n.y = y[k];
        PFRL_CHECK_ARG(n.y != nullptr && aligned4(n.y), "pfrl_mlp_wide_fwd: null or misaligned output");
    }
    hipLaunchKernelGGL(k_mlp_wide_fwd, dim3((M + kRows - 1) / kRows, n_nets), dim3(kFwdThreads), 0, (hipStream_t)stream,
                       x1, x2, a, (int)M, (int)K1, (int)K2, (int)n_layers, (int)act);
    PFRL_LAUNCH_CHECK();
}

extern "C" int pfrl_mlp_wide_dx(int32_t M, int32_t K, int32_t n_layers, int32_t n_nets, const float *const *w,
                                const int32_t *widths, int32_t act, const float *const *saved, const float *const *dy,
                                float *dx, int32_t col0, int32_t ncol, void *stream) {
    if (n_nets == 0) return 0;
    const char *err = check_wide(M, K, n_layers, n_nets, w, widths, act);
    PFRL_CHECK_ARG(err == nullptr, err);
    PFRL_CHECK_ARG(ncol >= 1 && ncol <= kMaxLast && col0 >= 0 && col0 <= K - ncol,
                   "pfrl_mlp_wide_dx: 1 <= ncol <= 64, col0 + ncol <= K");
    PFRL_CHECK_ARG(saved != nullptr && dy != nullptr && dx != nullptr && aligned4(dx),
                   "pfrl_mlp_wide_dx: null or misaligned pointer");
    WideDxArgs a{};
    for (int l = 0; l < n_layers; ++l) a.n[l] = widths[l];
    for (int k = 0; k < n_nets; ++k) {
        WideDxNet &n = a.net[k];
        for (int l = 0; l < n_layers; ++l) n.w[l] = w[3 * k + l];
        for (int l = 0; l + 1 < n_layers; ++l) {
            n.a[l] = saved[2 * k + l];
            PFRL_CHECK_ARG(n.a[l] != nullptr && aligned4(n.a[l]), "pfrl_mlp_wide_dx: null or misaligned activations");
        }
        n.dy = dy[k];
        PFRL_CHECK_ARG(n.dy != nullptr && aligned4(n.dy), "pfrl_mlp_wide_dx: null or misaligned dy");
    }
    hipLaunchKernelGGL(k_mlp_wide_dx, dim3((M + kRows - 1) / kRows), dim3(kDxThreads), 0, (hipStream_t)stream, a, dx,
                       (int)M, (int)K, (int)n_layers, (int)n_nets, (int)act, (int)col0, (int)ncol);
    PFRL_LAUNCH_CHECK();
}
