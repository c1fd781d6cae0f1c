// Whole small MLPs as one launch for gfx950: Linear(obs, <= 64), act, Linear(<= 64, <= 64), act,
// Linear(<= 64, A or 1) of the on-policy continuous-control agents (pfrl's MuJoCo reproductions of PPO,
// TRPO, A2C and REINFORCE: 64-64 tanh networks for the policy and the value function).  At these widths
// every layer is ONE 64 x 64 tile, so a per-layer launch is all launch; here the forward of the whole
// network is one launch and so is its backward, for one network or for two that share the input
// (blockIdx.y picks the network; pointers travel by value, as CriticArgs of td3.hip, so launches capture).
//
// All products run on v_mfma_f32_16x16x4_f32 with both operands read from LDS as [row][k] matrices of
// row stride kLd = 68 floats (16-byte aligned rows; 68 r + k maps the 64 lanes of an operand read to 64
// different banks).  For a block of 16 k, lane (c = lane & 15, kq = lane >> 4) reads the four floats
// k0 + 4 kq .. + 3 of its row as one ds_read_b128 and MFMA step i takes element i of both operands (any
// bijection of k serves a reduction; recurrent_mfma.h states the rule).
//
// Forward.  A workgroup owns a tile of rows.  The first layer's x and W stream through LDS in chunks of
// 64 k (LDS use does not grow with in_features); a hidden layer's weights are in LDS whole, the next
// layer's being loaded while the current one multiplies.  Widths that are no multiple of 16 and k tails
// are zeros in LDS (every global load is bounds-checked; nothing is read beyond a matrix).  Accumulators
// get bias and activation in registers and go back to the LDS row tile as the next layer's A operand;
// hidden activations reach HBM only through the `save` pointers (for the backward pass: tanh' = 1 - a^2
// and ReLU' = a > 0 are both functions of the output).
//   16-row program: the four waves split the (up to four) column tiles       (small M: more workgroups)
//   64-row program: the four waves split the rows, each holds four column tiles
// Every output element is ONE accumulator chain over k in ascending blocks of 16 in both programs, with
// the same zero padding: the bits of an output row depend on that row and the parameters only -- not on
// M, the row's position, the program or n_nets.
//
// Backward.  A workgroup walks its 64-row tiles in ascending order.  Per tile, from the last layer down:
// d_l (LDS) against a_{l-1} (LDS) gives the tile's dW_l with rows as the reduction axis, and db_l as one
// more MFMA against a B operand of ones; d_l against W_l (LDS) gives d_{l-1}, times act'(a_{l-1}), back
// into LDS.  The first layer's x, W and dW go in chunks of 64 columns; dx is optional (observations
// need none).  dW / db stay in registers over all of the workgroup's tiles (up to 8 x 4 + 2 x 4 + 3
// accumulator tiles a wave, in f64: v_mfma_f64_16x16x4_f64 on the widened operands; with f32 chains the
// gradients were three times further from float64 than the per-layer route's) and are rounded and
// written once, as the workgroup's slab of a packed gradient vector
// ([W_0 | b_0 | W_1 | ...], every segment padded to 4 floats).  One workgroup: the slab IS the gradient.
// More: at most kMaxSlabs slabs in a workspace, added in slab order in f64 by k_mlp_fold behind the same
// entry point (the f32 adds of pfrl_splitk_reduce missed the accuracy rule of the tests for bias
// gradients).  No atomics; one order of every sum.
//
// Normalised input (the NORM instantiations behind pfrl_mlp_fwd_norm / pfrl_mlp_bwd_norm: an observation normaliser
// in front of the first layer).  x is the raw batch; the one place where each kernel stages the first layer's x
// chunk (the forward's product, the backward's dW_0 operand) normalises on the way into LDS (stage_x), so y, the
// hidden saves and the packed gradient have the bits of the plain launches on the normalised batch and the
// row-bits rule above holds with "the statistics" added.  No dx with a normaliser; the tangent pass takes none.
//
// Tangent pass (k_mlp_jvp: J v of the last layer's output with respect to the parameters, the forward-mode
// half of a Gauss-Newton / Fisher-vector product whose other half, J^T, is the backward above).  With the
// direction V_l, c_l shaped like W_l, b_l and the hidden activations a_l that the forward saved:
//   t_z = W_l t_{l-1} + V_l a_{l-1} + c_l  (t_{-1} = 0, a_{-1} = x),   t_l = act'(a_l) t_z,   ty = t_z of the last
// layer, times an optional per-column factor.  The forward's tile programs: layer 0 is V_0 x + c_0 with x and
// V_0 streamed in 64-k chunks (V_0 in W_0's place, no W_0 product); a hidden layer has W_l, V_l, the a_{l-1}
// tile and the t_{l-1} tile in LDS and runs both products as ONE accumulator chain, W t first, then V a, over
// ascending k blocks: a row of ty has the same bits at any M, any position and in either program.  The
// direction is read with scalar bounds-checked loads (`stage`): its pointers are 4-byte aligned only, they
// point into a flat vector whose segments are not padded.  LDS, under the 64 KB that a static allocation
// may take:
//   16-row program: a and t tiles 2 x 4 352 B + THREE weight buffers 3 x 17 408 B = 60 928 B.  W_1 and V_1
//                   travel while layer 0 multiplies, W_2 while layer 1 does, V_2 as soon as W_1 has been read.
//   64-row program: a and t tiles 2 x 17 408 B + ONE weight buffer = 52 224 B (W, V and both tiles at once
//                   would be 69 632 B): W_l and V_l pass through the one buffer in turn, the chain unchanged.
#include "mlp_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxW = 64;          // hidden and output widths
constexpr int kMaxIn = 512;
constexpr int kMaxM = 65536;
constexpr int kChunk = 64;         // k columns of the first layer per LDS trip
constexpr int kMaxChunks = kMaxIn / kChunk;
constexpr int kLd = 68;            // LDS row stride
constexpr int kSmallM = 512;       // default: up to this many rows take the 16-row program
constexpr int kBwdRows = 64;
constexpr int kMaxSlabs = 32;

typedef float Tile[kLd];

struct FwdNet {
    const float *w[3], *b[3];
    float *save[2], *y;
    int n[3], act;
};
struct FwdArgs {
    FwdNet net[2];
};

struct JvpArgs {
    const float *w[3], *a[2], *vw[3], *vb[3], *col_scale;
    float *ty;
    int n[3], act;
};

struct BwdNet {
    const float *w[3], *a[2], *dy;
    float *dx, *grads;
    int n[3], act;
};
struct BwdArgs {
    BwdNet net[2];
};

// The observation normaliser in front of the first layer (pfrl_mlp_fwd_norm / pfrl_mlp_bwd_norm): the running
// mean and variance [K0], read in place; clip <= 0: none.
struct NormArgs {
    const float *mean, *var;
    float eps, clip;
};

// The first layer's x chunk into LDS.  NORM: every element as clamp((x - mean[k]) * scale[k], +-clip) with
// scale = (float)(1 / sqrt((double)(var + eps))), the f32 sum widened: on this device the bits of torch's
// (var + eps) ** -0.5 (rsqrtf, 1.f / sqrtf, powf and v_rsq_f32 itself all differ from it in 11 to 26 % of a million
// values; tests/test_mlp_norm.py holds the expression to torch's).  Then a subtract, a multiply and two compares
// (no contraction: the build has it off): the bits of the module's own expression.  A thread's column is the same
// in every trip of the staging loop (kThreads is a multiple of 64), so the column's mean and scale live in two
// registers, loaded once per chunk beside the first x loads: no LDS array, no barrier between the statistics and
// the tile.  Rows beyond M and columns beyond K0 stay zeros; mean and var are never read beyond K0.
template <bool NORM>
__device__ __forceinline__ void stage_x(Tile *dst, const float *__restrict__ x, int rows, int r0, int M, int c0, int K0,
                                        const NormArgs &nm, int tid) {
    if constexpr (!NORM) {
        stage<kThreads>(dst, x, rows, r0, M, c0, K0, K0, tid);
    } else {
        static_assert(kThreads % 64 == 0, "a thread keeps one column");
        const int c = tid & 63, gc = c0 + c;
        const bool in = gc < K0;
        const float mu = in ? nm.mean[gc] : 0.f;
        const float sc = in ? (float)(1.0 / sqrt((double)(nm.var[gc] + nm.eps))) : 0.f;
        const float clip = nm.clip;
        for (int r = tid >> 6; r < rows; r += kThreads / 64) {
            float v = 0.f;
            if (in && r0 + r < M) {
                v = (x[(size_t)(r0 + r) * K0 + gc] - mu) * sc;
                if (clip > 0.f) v = v < -clip ? -clip : (v > clip ? clip : v);
            }
            dst[r][c] = v;
        }
    }
}

// acc[j] += A[arow + c16][0 .. kpad) . W[16 ct(j) + c16][0 .. kpad): NT column tiles against one row tile
template <int RT>
__device__ __forceinline__ void fwd_mma(f32x4 (&acc)[RT / 16], const Tile *sA, const Tile *sW, int kpad, int ntiles,
                                        int wave, int c16, int kq) {
    constexpr int NT = RT / 16;
    const int arow = (RT == 64 ? 16 * wave : 0) + c16;
    for (int k0 = 0; k0 < kpad; k0 += 16) {
        const float4 a = *reinterpret_cast<const float4 *>(&sA[arow][k0 + 4 * kq]);
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int ct = RT == 64 ? j : wave;
            if (ct < ntiles) {
                const float4 w = *reinterpret_cast<const float4 *>(&sW[16 * ct + c16][k0 + 4 * kq]);
                mfma_16x16x4(acc[j], a.x, w.x);
                mfma_16x16x4(acc[j], a.y, w.y);
                mfma_16x16x4(acc[j], a.z, w.z);
                mfma_16x16x4(acc[j], a.w, w.w);
            }
        }
    }
}

// bias and activation in registers; the hidden tile back into sA (columns beyond N as zeros), saved and
// final values to global memory
template <int RT>
__device__ __forceinline__ void fwd_epilogue(const f32x4 (&acc)[RT / 16], Tile *sA, const float *__restrict__ bias,
                                             float *__restrict__ out, bool last, int act, int N, int ntiles, int row0,
                                             int M, int wave, int c16, int kq) {
    constexpr int NT = RT / 16;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int ct = RT == 64 ? j : wave;
        if (ct >= ntiles) continue;
        const int col = 16 * ct + c16;
        const float bv = col < N ? bias[col] : 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = (RT == 64 ? 16 * wave : 0) + 4 * kq + i;
            float v = acc[j][i] + bv;
            if (!last) {
                v = col < N ? activate(v, act) : 0.f;
                sA[r][col] = v;
            }
            if (out != nullptr && col < N && row0 + r < M) out[(size_t)(row0 + r) * N + col] = v;
        }
    }
}

template <int RT, bool NORM>
__global__ __launch_bounds__(kThreads) PFRL_NO_PACKED_FP32 void k_mlp_fwd(const float *__restrict__ x, FwdArgs args,
                                                                         int M, int K0, int L, NormArgs nm) {
    __shared__ __attribute__((aligned(16))) float sA[RT][kLd];
    __shared__ __attribute__((aligned(16))) float sW[2][kMaxW][kLd];
    const FwdNet &net = args.net[blockIdx.y];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c16 = lane & 15, kq = lane >> 4;
    const int row0 = blockIdx.x * RT;
    const int act = net.act;
    constexpr int NT = RT / 16;
    f32x4 acc[NT];

    // the second layer's weights travel while the first layer multiplies
    if (L > 1) stage<kThreads>(sW[1], net.w[1], 16 * ((net.n[1] + 15) >> 4), 0, net.n[1], 0, net.n[0], net.n[0], tid);

    // layer 0: x and W_0 in chunks of 64 k
    {
        const int N = net.n[0], nt = (N + 15) >> 4;
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int c0 = 0; c0 < K0; c0 += kChunk) {
            __syncthreads();                                  // (the previous chunk has been read)
            stage_x<NORM>(sA, x, RT, row0, M, c0, K0, nm, tid);
            stage<kThreads>(sW[0], net.w[0], 16 * nt, 0, N, c0, K0, K0, tid);
            __syncthreads();
            fwd_mma<RT>(acc, sA, sW[0], (min(kChunk, K0 - c0) + 15) & ~15, nt, wave, c16, kq);
        }
        __syncthreads();
        fwd_epilogue<RT>(acc, sA, net.b[0], L == 1 ? net.y : net.save[0], L == 1, act, N, nt, row0, M, wave, c16, kq);
    }
    if (L == 1) return;
    if (L > 2) stage<kThreads>(sW[0], net.w[2], 16 * ((net.n[2] + 15) >> 4), 0, net.n[2], 0, net.n[1], net.n[1], tid);
    __syncthreads();
    {
        const int N = net.n[1], nt = (N + 15) >> 4;
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        fwd_mma<RT>(acc, sA, sW[1], ((net.n[0] + 15) >> 4) << 4, nt, wave, c16, kq);
        __syncthreads();
        fwd_epilogue<RT>(acc, sA, net.b[1], L == 2 ? net.y : net.save[1], L == 2, act, N, nt, row0, M, wave, c16, kq);
    }
    if (L == 2) return;
    __syncthreads();
    {
        const int N = net.n[2], nt = (N + 15) >> 4;
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        fwd_mma<RT>(acc, sA, sW[0], ((net.n[1] + 15) >> 4) << 4, nt, wave, c16, kq);
        fwd_epilogue<RT>(acc, sA, net.b[2], net.y, true, act, N, nt, row0, M, wave, c16, kq);
    }
}

// The tangent of a layer from its accumulators: t_z = acc + c; a hidden layer's t = act'(a) t_z goes into sT
// (a: the layer's saved output, staged in sA; columns beyond N as zeros), the last layer's t_z, times the
// column factor, to global memory.
template <int RT>
__device__ __forceinline__ void jvp_epilogue(const f32x4 (&acc)[RT / 16], const Tile *sA, Tile *sT,
                                             const float *__restrict__ vb, const float *__restrict__ col_scale,
                                             float *__restrict__ ty, bool last, int act, int N, int ntiles, int row0,
                                             int M, int wave, int c16, int kq) {
    constexpr int NT = RT / 16;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int ct = RT == 64 ? j : wave;
        if (ct >= ntiles) continue;
        const int col = 16 * ct + c16;
        const float cv = col < N ? vb[col] : 0.f;
        const float cs = last && col_scale != nullptr && col < N ? col_scale[col] : 1.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = (RT == 64 ? 16 * wave : 0) + 4 * kq + i;
            const float v = acc[j][i] + cv;
            if (!last)
                sT[r][col] = col < N ? act_grad(v, sA[r][col], act) : 0.f;
            else if (col < N && row0 + r < M)
                ty[(size_t)(row0 + r) * N + col] = col_scale != nullptr ? v * cs : v;
        }
    }
}

// a whole [N][K] matrix (weights or direction), rows padded to the tile
__device__ __forceinline__ void stage_mat(Tile *dst, const float *__restrict__ src, int N, int K, int tid) {
    stage<kThreads>(dst, src, 16 * ((N + 15) >> 4), 0, N, 0, K, K, tid);
}

template <int RT>
__global__ __launch_bounds__(kThreads) PFRL_NO_PACKED_FP32 void k_mlp_jvp(const float *__restrict__ x, JvpArgs g, int M,
                                                                         int K0, int L) {
    constexpr int NB = RT == 16 ? 3 : 1, NT = RT / 16;
    __shared__ __attribute__((aligned(16))) float sA[RT][kLd];
    __shared__ __attribute__((aligned(16))) float sT[RT][kLd];
    __shared__ __attribute__((aligned(16))) float sW[NB][kMaxW][kLd];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c16 = lane & 15, kq = lane >> 4;
    const int row0 = blockIdx.x * RT;
    const int act = g.act;
    f32x4 acc[NT];

    if constexpr (NB == 3) {
        if (L > 1) {
            stage_mat(sW[1], g.w[1], g.n[1], g.n[0], tid);
            stage_mat(sW[2], g.vw[1], g.n[1], g.n[0], tid);
        }
    }
    // layer 0: V_0 x in chunks of 64 k
    {
        const int N = g.n[0], nt = (N + 15) >> 4;
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int c0 = 0; c0 < K0; c0 += kChunk) {
            __syncthreads();                                  // (the previous chunk has been read)
            stage<kThreads>(sA, x, RT, row0, M, c0, K0, K0, tid);
            stage<kThreads>(sW[0], g.vw[0], 16 * nt, 0, N, c0, K0, K0, tid);
            __syncthreads();
            fwd_mma<RT>(acc, sA, sW[0], (min(kChunk, K0 - c0) + 15) & ~15, nt, wave, c16, kq);
        }
    }
#pragma unroll
    for (int l = 0; l < 3; ++l) {
        if (l >= L) continue;
        const int N = g.n[l], nt = (N + 15) >> 4;
        const bool last = l == L - 1;
        if (l > 0) {
            // (behind the previous epilogue's barrier: sA = a_{l-1}, sT = t_{l-1}, every buffer read)
            const int kpad = ((g.n[l - 1] + 15) >> 4) << 4;
#pragma unroll
            for (int j = 0; j < NT; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
            if constexpr (NB == 3) {
                if (l == 1 && L > 2) stage_mat(sW[0], g.w[2], g.n[2], g.n[1], tid);
                fwd_mma<RT>(acc, sT, l == 1 ? sW[1] : sW[0], kpad, nt, wave, c16, kq);
                fwd_mma<RT>(acc, sA, l == 1 ? sW[2] : sW[1], kpad, nt, wave, c16, kq);
            } else {
                stage_mat(sW[0], g.w[l], N, g.n[l - 1], tid);
                __syncthreads();
                fwd_mma<RT>(acc, sT, sW[0], kpad, nt, wave, c16, kq);
                __syncthreads();
                stage_mat(sW[0], g.vw[l], N, g.n[l - 1], tid);
                __syncthreads();
                fwd_mma<RT>(acc, sA, sW[0], kpad, nt, wave, c16, kq);
            }
        }
        if (!last) {
            __syncthreads();                                  // (both tiles and this layer's matrices have been read)
            stage<kThreads>(sA, g.a[l], RT, row0, M, 0, N, N, tid);
            if constexpr (NB == 3) {
                if (l == 1) stage_mat(sW[1], g.vw[2], g.n[2], g.n[1], tid);
            }
            __syncthreads();
        }
        jvp_epilogue<RT>(acc, sA, sT, g.vb[l], g.col_scale, g.ty, last, act, N, nt, row0, M, wave, c16, kq);
        if (!last) __syncthreads();
    }
}

// The tile's weight gradient (f64 accumulators: row 16 wave + kq + 4 i): acc[j][i] += sum over the 64 rows r of D[r][.] *
// A[r][16 j + c16] for the ktiles column tiles of A; accb (when given) the same against ones: the column
// sums of D, in every lane column -- in f64 (four more MFMAs per 16 rows): a bias gradient is a plain sum
// of up to 65 536 terms, and its only roundings are the slab's and the fold's.
__device__ __forceinline__ void bwd_wgrad(f64x4 (&acc)[4], f64x4 *accb, const Tile *sD, const Tile *sA, int ktiles,
                                          int wave, int c16, int kq) {
    for (int r0 = 0; r0 < kBwdRows; r0 += 16) {
        float dv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) dv[i] = sD[r0 + 4 * kq + i][16 * wave + c16];
        if (accb != nullptr) {
#pragma unroll
            for (int i = 0; i < 4; ++i) mfma_16x16x4(*accb, dv[i], 1.f);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j < ktiles) {
#pragma unroll
                for (int i = 0; i < 4; ++i) mfma_16x16x4(acc[j], dv[i], sA[r0 + 4 * kq + i][16 * j + c16]);
            }
        }
    }
}

// d[j][i] = sum over n < npad of D[16 wave + 4 kq + i][n] * W[n][16 j + c16]
__device__ __forceinline__ void bwd_dgrad(f32x4 (&d)[4], const Tile *sD, const Tile *sW, int npad, int ktiles, int wave,
                                          int c16, int kq) {
#pragma unroll
    for (int j = 0; j < 4; ++j) d[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int n0 = 0; n0 < npad; n0 += 16) {
        const float4 a = *reinterpret_cast<const float4 *>(&sD[16 * wave + c16][n0 + 4 * kq]);
        const float av[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j < ktiles) {
#pragma unroll
                for (int i = 0; i < 4; ++i) mfma_16x16x4(d[j], av[i], sW[n0 + 4 * kq + i][16 * j + c16]);
            }
        }
    }
}

__device__ __forceinline__ int pad4(int n) { return (n + 3) & ~3; }

// acc[j][i] = element (16 wave + kq + 4 i, k0 + 16 j + c16) of an N x K matrix at dst, rounded once
__device__ __forceinline__ void store_wtile(float *__restrict__ dst, const f64x4 (&acc)[4], int N, int K, int k0, int wave,
                                            int c16, int kq) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int k = k0 + 16 * j + c16;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int n = 16 * wave + kq + 4 * i;
            if (n < N && k < K) dst[(size_t)n * K + k] = (float)acc[j][i];
        }
    }
}

template <bool NORM>
__global__ __launch_bounds__(kThreads) PFRL_NO_PACKED_FP32 void k_mlp_bwd(const float *__restrict__ x, BwdArgs args,
                                                                         int M, int K0, int L, int tiles_per_wg,
                                                                         long long slab_stride, NormArgs nm) {
    __shared__ __attribute__((aligned(16))) float sD[kBwdRows][kLd];
    __shared__ __attribute__((aligned(16))) float sA[kBwdRows][kLd];
    __shared__ __attribute__((aligned(16))) float sW[kMaxW][kLd];
    const BwdNet &net = args.net[blockIdx.y];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c16 = lane & 15, kq = lane >> 4;
    const int act = net.act;
    const int ntiles = (M + kBwdRows - 1) / kBwdRows;
    const int t_begin = blockIdx.x * tiles_per_wg, t_end = min(t_begin + tiles_per_wg, ntiles);
    const int nch = (K0 + kChunk - 1) / kChunk;

    f64x4 gw0[kMaxChunks][4], gw[2][4], gb[3];
#pragma unroll
    for (int c = 0; c < kMaxChunks; ++c)
#pragma unroll
        for (int j = 0; j < 4; ++j) gw0[c][j] = f64x4{0., 0., 0., 0.};
#pragma unroll
    for (int l = 0; l < 2; ++l)
#pragma unroll
        for (int j = 0; j < 4; ++j) gw[l][j] = f64x4{0., 0., 0., 0.};
#pragma unroll
    for (int l = 0; l < 3; ++l) gb[l] = f64x4{0., 0., 0., 0.};

    for (int t = t_begin; t < t_end; ++t) {
        const int row0 = t * kBwdRows;
#pragma unroll
        for (int l = 2; l >= 1; --l) {
            if (l >= L) continue;
            const int N = net.n[l], K = net.n[l - 1], ntn = (N + 15) >> 4, ntk = (K + 15) >> 4;
            __syncthreads();                                  // (sD is written, sA and sW have been read)
            if (l == L - 1) stage<kThreads>(sD, net.dy, kBwdRows, row0, M, 0, N, N, tid);
            stage<kThreads>(sA, net.a[l - 1], kBwdRows, row0, M, 0, K, K, tid);
            stage<kThreads>(sW, net.w[l], 16 * ntn, 0, N, 0, K, K, tid);
            __syncthreads();
            if (wave < ntn) bwd_wgrad(gw[l - 1], &gb[l], sD, sA, ntk, wave, c16, kq);
            f32x4 d[4];
            bwd_dgrad(d, sD, sW, 16 * ntn, ntk, wave, c16, kq);
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int i = 0; i < 4; ++i) d[j][i] = act_grad(d[j][i], sA[16 * wave + 4 * kq + i][16 * j + c16], act);
            __syncthreads();                                  // (every wave has read d_l)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (j < ntk) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) sD[16 * wave + 4 * kq + i][16 * j + c16] = d[j][i];
                }
            }
        }
        // layer 0: x, W_0 and dx in chunks of 64 columns
        const int N = net.n[0], ntn = (N + 15) >> 4;
#pragma unroll
        for (int c = 0; c < kMaxChunks; ++c) {
            if (c >= nch) continue;
            const int c0 = c * kChunk, ntk = min(4, (K0 - c0 + 15) >> 4);
            __syncthreads();
            if (c == 0 && L == 1) stage<kThreads>(sD, net.dy, kBwdRows, row0, M, 0, N, N, tid);
            stage_x<NORM>(sA, x, kBwdRows, row0, M, c0, K0, nm, tid);
            if (net.dx != nullptr) stage<kThreads>(sW, net.w[0], 16 * ntn, 0, N, c0, K0, K0, tid);
            __syncthreads();
            if (wave < ntn) bwd_wgrad(gw0[c], c == 0 ? &gb[0] : nullptr, sD, sA, ntk, wave, c16, kq);
            if (net.dx != nullptr) {
                f32x4 d[4];
                bwd_dgrad(d, sD, sW, 16 * ntn, ntk, wave, c16, kq);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int k = c0 + 16 * j + c16;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int r = row0 + 16 * wave + 4 * kq + i;
                        if (j < ntk && k < K0 && r < M) net.dx[(size_t)r * K0 + k] = d[j][i];
                    }
                }
            }
        }
    }

    // the workgroup's slab: [W_0 | b_0 | W_1 | b_1 | ...], segments padded to 4 floats
    float *__restrict__ out = net.grads + (size_t)blockIdx.x * slab_stride;
#pragma unroll
    for (int l = 0; l < 3; ++l) {
        if (l >= L) continue;
        const int N = net.n[l], K = l == 0 ? K0 : net.n[l - 1];
        if (l == 0) {
#pragma unroll
            for (int c = 0; c < kMaxChunks; ++c)
                if (c < nch) store_wtile(out, gw0[c], N, K, c * kChunk, wave, c16, kq);
        } else {
            store_wtile(out, gw[l - 1], N, K, 0, wave, c16, kq);
        }
        if (tid < pad4(N * K) - N * K) out[N * K + tid] = 0.f;      // (padding: zeros, so the fold reads none)
        out += pad4(N * K);
        if (c16 == 0) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int n = 16 * wave + kq + 4 * i;      // (the f64 accumulator's row order)
                if (n < N) out[n] = (float)gb[l][i];
            }
        }
        if (tid < pad4(N) - N) out[N + tid] = 0.f;
        out += pad4(N);
    }
}

// The slabs of a network added in slab order in f64 and rounded once: out[e] = sum over g of ws[g stride + e].
// (pfrl_splitk_reduce adds in f32: over the 17 slabs of 2 049 rows a bias gradient was 8.6e-6 from float64
// where torch's cascade sum is 3.1e-6.  Here the only roundings are each slab's and the last.)
struct FoldArgs {
    const float *ws[2];
    float *out[2];
    int n[2];
};

__global__ __launch_bounds__(kThreads) void k_mlp_fold(FoldArgs a, int slabs, long long stride) {
    const int k = blockIdx.y, e = blockIdx.x * kThreads + threadIdx.x;
    if (e >= a.n[k]) return;
    const float *__restrict__ p = a.ws[k] + e;
    double s = 0.;
    for (int g = 0; g < slabs; ++g) s += (double)p[(size_t)g * stride];
    a.out[k][e] = (float)s;
}

// the envelope both entry points share
const char *check_envelope(const float *x, int32_t M, int32_t K0, int32_t L, int32_t n_nets, const float *const *w,
                           const int32_t *widths, const int32_t *act) {
    if (M < 1 || M > kMaxM) return "1 <= M <= 65536";
    if (K0 < 1 || K0 > kMaxIn) return "1 <= in_features <= 512";
    if (L < 1 || L > 3) return "1 to 3 layers";
    if (n_nets < 1 || n_nets > 2) return "one or two networks";
    if (x == nullptr || w == nullptr || widths == nullptr || act == nullptr) return "null pointer";
    if (!aligned4(x)) return "misaligned pointer";
    for (int k = 0; k < n_nets; ++k) {
        if (act[k] != PFRL_MLP_TANH && act[k] != PFRL_MLP_RELU) return "activation: tanh or ReLU";
        for (int l = 0; l < L; ++l) {
            if (widths[3 * k + l] < 1 || widths[3 * k + l] > kMaxW) return "1 <= width <= 64";
            if (w[3 * k + l] == nullptr) return "null pointer";
            if (!aligned4(w[3 * k + l])) return "misaligned pointer";
        }
    }
    return nullptr;
}

// the normaliser's arguments (nm == nullptr: none)
const char *check_norm(const float *mean, const float *var, float eps) {
    if (mean == nullptr || var == nullptr) return "normaliser: null pointer";
    if (!aligned4(mean) || !aligned4(var)) return "normaliser: misaligned pointer";
    if (!(eps >= 0.f)) return "normaliser: eps >= 0";
    return nullptr;
}

int mlp_fwd(const float *x, int32_t M, int32_t in_features, int32_t n_layers, int32_t n_nets, const float *const *w,
            const float *const *b, const int32_t *widths, const int32_t *act, float *const *save, float *const *y,
            int32_t small_m, const NormArgs *norm, void *stream) {
    if (n_nets == 0) return 0;
    const char *err = check_envelope(x, M, in_features, n_layers, n_nets, w, widths, act);
    PFRL_CHECK_ARG(err == nullptr, err);
    PFRL_CHECK_ARG(b != nullptr && y != nullptr, "pfrl_mlp_fwd: null pointer");
    FwdArgs a{};
    for (int k = 0; k < n_nets; ++k) {
        FwdNet &n = a.net[k];
        for (int l = 0; l < n_layers; ++l) {
            n.w[l] = w[3 * k + l];
            n.b[l] = b[3 * k + l];
            n.n[l] = widths[3 * k + l];
            PFRL_CHECK_ARG(n.b[l] != nullptr && aligned4(n.b[l]), "pfrl_mlp_fwd: null or misaligned bias");
        }
        for (int l = 0; l + 1 < n_layers; ++l) {
            n.save[l] = save != nullptr ? save[2 * k + l] : nullptr;
            PFRL_CHECK_ARG(aligned4(n.save[l]), "pfrl_mlp_fwd: misaligned pointer");
        }
        n.y = y[k];
        n.act = act[k];
        PFRL_CHECK_ARG(n.y != nullptr && aligned4(n.y), "pfrl_mlp_fwd: null or misaligned output");
    }
    const int lim = small_m < 0 ? kSmallM : small_m;
    const bool small = M <= lim;
    const dim3 grid((M + (small ? 15 : 63)) / (small ? 16 : 64), n_nets);
    const NormArgs nm = norm != nullptr ? *norm : NormArgs{};
    auto kernel = norm != nullptr ? (small ? k_mlp_fwd<16, true> : k_mlp_fwd<64, true>)
                                  : (small ? k_mlp_fwd<16, false> : k_mlp_fwd<64, false>);
    hipLaunchKernelGGL(kernel, grid, dim3(kThreads), 0, (hipStream_t)stream, x, a, (int)M, (int)in_features,
                       (int)n_layers, nm);
    PFRL_LAUNCH_CHECK();
}

}  // namespace

extern "C" int pfrl_mlp_fwd(const float *x, int32_t M, int32_t in_features, int32_t n_layers, int32_t n_nets,
                            const float *const *w, const float *const *b, const int32_t *widths, const int32_t *act,
                            float *const *save, float *const *y, int32_t small_m, void *stream) {
    return mlp_fwd(x, M, in_features, n_layers, n_nets, w, b, widths, act, save, y, small_m, nullptr, stream);
}

extern "C" int pfrl_mlp_fwd_norm(const float *x, int32_t M, int32_t in_features, int32_t n_layers, int32_t n_nets,
                                 const float *const *w, const float *const *b, const int32_t *widths,
                                 const int32_t *act, float *const *save, float *const *y, int32_t small_m,
                                 const float *mean, const float *var, float eps, float clip, void *stream) {
    if (n_nets == 0) return 0;
    const char *err = check_norm(mean, var, eps);
    PFRL_CHECK_ARG(err == nullptr, err);
    const NormArgs nm{mean, var, eps, clip};
    return mlp_fwd(x, M, in_features, n_layers, n_nets, w, b, widths, act, save, y, small_m, &nm, stream);
}

extern "C" int pfrl_mlp_jvp(const float *x, int32_t M, int32_t in_features, int32_t n_layers, const float *const *w,
                            const int32_t *widths, int32_t act, const float *const *saved, const float *const *vw,
                            const float *const *vb, const float *col_scale, float *ty, int32_t small_m,
                            void *stream) {
    const char *err = check_envelope(x, M, in_features, n_layers, 1, w, widths, &act);
    PFRL_CHECK_ARG(err == nullptr, err);
    PFRL_CHECK_ARG(vw != nullptr && vb != nullptr && ty != nullptr && (n_layers == 1 || saved != nullptr),
                   "pfrl_mlp_jvp: null pointer");
    PFRL_CHECK_ARG(aligned4(ty) && aligned4(col_scale), "pfrl_mlp_jvp: misaligned pointer");
    JvpArgs g{};
    for (int l = 0; l < n_layers; ++l) {
        g.w[l] = w[l];
        g.vw[l] = vw[l];
        g.vb[l] = vb[l];
        g.n[l] = widths[l];
        PFRL_CHECK_ARG(g.vw[l] != nullptr && g.vb[l] != nullptr && aligned4(g.vw[l]) && aligned4(g.vb[l]),
                       "pfrl_mlp_jvp: null or misaligned direction");
    }
    for (int l = 0; l + 1 < n_layers; ++l) {
        g.a[l] = saved[l];
        PFRL_CHECK_ARG(g.a[l] != nullptr && aligned4(g.a[l]), "pfrl_mlp_jvp: null or misaligned activations");
    }
    g.col_scale = col_scale;
    g.ty = ty;
    g.act = act;
    const int lim = small_m < 0 ? kSmallM : small_m;
    if (M <= lim)
        hipLaunchKernelGGL(k_mlp_jvp<16>, dim3((M + 15) / 16), dim3(kThreads), 0, (hipStream_t)stream, x, g, (int)M,
                           (int)in_features, (int)n_layers);
    else
        hipLaunchKernelGGL(k_mlp_jvp<64>, dim3((M + 63) / 64), dim3(kThreads), 0, (hipStream_t)stream, x, g, (int)M,
                           (int)in_features, (int)n_layers);
    PFRL_LAUNCH_CHECK();
}

extern "C" int pfrl_mlp_bwd_slabs(int32_t M) {
    if (M < 1 || M > kMaxM) return 0;
    const int tiles = (M + kBwdRows - 1) / kBwdRows;
    const int per_wg = (tiles + kMaxSlabs - 1) / kMaxSlabs;
    return (tiles + per_wg - 1) / per_wg;
}

namespace {

int mlp_bwd(const float *x, int32_t M, int32_t in_features, int32_t n_layers, int32_t n_nets, const float *const *w,
            const int32_t *widths, const int32_t *act, const float *const *saved, const float *const *dy,
            float *const *dx, float *const *grads, float *const *slab_ws, int64_t slab_stride, const NormArgs *norm,
            void *stream) {
    if (n_nets == 0) return 0;
    const char *err = check_envelope(x, M, in_features, n_layers, n_nets, w, widths, act);
    PFRL_CHECK_ARG(err == nullptr, err);
    PFRL_CHECK_ARG(dy != nullptr && grads != nullptr && (n_layers == 1 || saved != nullptr),
                   "pfrl_mlp_bwd: null pointer");
    const int slabs = pfrl_mlp_bwd_slabs(M);
    PFRL_CHECK_ARG(slabs == 1 || slab_ws != nullptr, "pfrl_mlp_bwd: more than one slab needs the workspace");
    BwdArgs a{};
    FoldArgs f{};
    int max_floats = 0;
    for (int k = 0; k < n_nets; ++k) {
        BwdNet &n = a.net[k];
        int64_t floats = 0;
        for (int l = 0; l < n_layers; ++l) {
            n.w[l] = w[3 * k + l];
            n.n[l] = widths[3 * k + l];
            floats += ((n.n[l] * (l == 0 ? in_features : n.n[l - 1]) + 3) & ~3) + ((n.n[l] + 3) & ~3);
        }
        for (int l = 0; l + 1 < n_layers; ++l) {
            n.a[l] = saved[2 * k + l];
            PFRL_CHECK_ARG(n.a[l] != nullptr && aligned4(n.a[l]), "pfrl_mlp_bwd: null or misaligned activations");
        }
        n.dy = dy[k];
        n.dx = dx != nullptr ? dx[k] : nullptr;
        n.grads = slabs == 1 ? grads[k] : slab_ws[k];
        n.act = act[k];
        f.ws[k] = n.grads;
        f.out[k] = grads[k];
        f.n[k] = (int)floats;
        max_floats = floats > max_floats ? (int)floats : max_floats;
        PFRL_CHECK_ARG(n.dy != nullptr && aligned4(n.dy) && aligned4(n.dx), "pfrl_mlp_bwd: null or misaligned pointer");
        PFRL_CHECK_ARG(grads[k] != nullptr && aligned4(grads[k]) && n.grads != nullptr && aligned4(n.grads),
                       "pfrl_mlp_bwd: null or misaligned gradients or workspace");
        PFRL_CHECK_ARG(slabs == 1 || (slab_stride >= floats && slab_stride % 4 == 0),
                       "pfrl_mlp_bwd: slab stride below the packed gradient's length or no multiple of 4");
    }
    const int tiles = (M + kBwdRows - 1) / kBwdRows;
    const NormArgs nm = norm != nullptr ? *norm : NormArgs{};
    hipLaunchKernelGGL(norm != nullptr ? k_mlp_bwd<true> : k_mlp_bwd<false>, dim3(slabs, n_nets), dim3(kThreads), 0,
                       (hipStream_t)stream, x, a, (int)M, (int)in_features, (int)n_layers, (tiles + slabs - 1) / slabs,
                       (long long)(slabs == 1 ? 0 : slab_stride), nm);
    if (slabs > 1)
        hipLaunchKernelGGL(k_mlp_fold, dim3((max_floats + kThreads - 1) / kThreads, n_nets), dim3(kThreads), 0,
                           (hipStream_t)stream, f, slabs, (long long)slab_stride);
    PFRL_LAUNCH_CHECK();
}

}  // namespace

extern "C" int pfrl_mlp_bwd(const float *x, int32_t M, int32_t in_features, int32_t n_layers, int32_t n_nets,
                            const float *const *w, const int32_t *widths, const int32_t *act,
                            const float *const *saved, const float *const *dy, float *const *dx,
                            float *const *grads, float *const *slab_ws, int64_t slab_stride, void *stream) {
    return mlp_bwd(x, M, in_features, n_layers, n_nets, w, widths, act, saved, dy, dx, grads, slab_ws, slab_stride,
                   nullptr, stream);
}

extern "C" int pfrl_mlp_bwd_norm(const float *x, int32_t M, int32_t in_features, int32_t n_layers, int32_t n_nets,
                                 const float *const *w, const int32_t *widths, const int32_t *act,
                                 const float *const *saved, const float *const *dy, float *const *grads,
                                 float *const *slab_ws, int64_t slab_stride, const float *mean, const float *var,
                                 float eps, float clip, void *stream) {
    if (n_nets == 0) return 0;
    const char *err = check_norm(mean, var, eps);
    PFRL_CHECK_ARG(err == nullptr, err);
    const NormArgs nm{mean, var, eps, clip};
    return mlp_bwd(x, M, in_features, n_layers, n_nets, w, widths, act, saved, dy, nullptr, grads, slab_ws, slab_stride,
                   &nm, stream);
}
