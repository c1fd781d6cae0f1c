// IQN's threshold embedding head (pfrl_amd/agents/iqn.py::_quantile_head), forward and backward:
//     out[r][h] = psi[r / N][h] * relu(b[h] + sum_i cos(taus[r] * i_pi[i]) * W[h][i])     r < M = B N
// f32, 16x16x4 f32 MFMA, no atomics, every sum in one fixed order: equal inputs give equal bits.  The
// pre-activation, its ReLU and (in the forward) the [M][n] embedding live in registers and LDS only;
// the forward writes the cosine tile out once as `emb` when the backward will want it.
//
// One product serves all three kernels (pre_tiles): W is the MFMA's A operand, the cosine tile its
// B operand, so a lane's four accumulator values are four consecutive h of ONE row (qnet.hip's first
// convolution does the same): psi and g are read, out is written 16 bytes at a time where H % 4 == 0
// and the bases are aligned, element by element otherwise.  K = n <= 64 is at most 4 blocks of 16;
// both operands are fetched as four consecutive k per lane, so k runs in a permuted but fixed order.
// n % 16 != 0: the cosine tile holds zeros beyond n and the W values beyond n are masked to zero.
// The backward recomputes `pre` through the same function from the saved cosines: the ReLU mask
// has the forward's bits.
//
// Forward (k_iqn_embed_fwd).  A workgroup of 4 waves owns 64 rows and `per` column blocks of 64.
// It computes its 64 x 64 cosine tile once into LDS (one f32 multiply and a precise cosf per element,
// the argument has the composite's bits), every wave takes the whole tile into registers (16
// float4), and then walks the column blocks: wave w owns columns 16 w .. 16 w + 15 of a block,
// streams its 16 rows of W from L2 straight into the A operand, 64 MFMAs, epilogue, store.
// Strip width: units = ceil(M / 64) ceil(H / 64) tile-blocks exist; per = max(1, units / 512), i.e.
// about two workgroups per CU of a 256-CU part once there is that much work, and one block per
// workgroup below.  At H = 3136: 1 024 rows -> 784 workgroups of one block, 2 048 -> 544 of three,
// 8 192 -> 640 of twelve.  A wider strip amortises the cosine tile, a narrower one fills the part.
//
// dpsi (k_iqn_embed_dpsi), row-parallel.  dpsi[bb][h] = sum_n' g[bb N + n'][h] relu(pre).  A
// workgroup's row tile is floor(64 / N) WHOLE batch rows (N <= 64, so at least one): no segment
// straddles two workgroups, and one thread sums a segment's N values from LDS in row order.  The
// segments do straddle the 16-row MFMA tiles, which is why the sum goes through LDS.
//
// dW / db (k_iqn_embed_dw), column-parallel.  A workgroup owns 64 columns (16 per wave, their W
// rows stay in registers) and a slab of 256 rows, which it walks in tiles of 64 staged in LDS.  Per
// 16 rows a wave recomputes pre, forms dpre = g psi [pre > 0] in registers, transposes that 16 x 16
// tile through LDS and multiplies dpre^T by the staged cosines (four N-tiles of 16 i) and by a column
// of ones (db) on the matrix unit.  dpre never reaches memory.  M <= 256: one slab, written straight
// to dw / db.  M > 256: ceil(M / 256) slabs into the caller's workspace, folded slab 0 first by
// pfrl_splitk_reduce.  Accumulation is f32: the accuracy rule of the tests (4 x the f32 composite's
// error) held without the f64 MFMA that the recurrent kernels need, there being no recurrence to
// compound the rounding.
//
// Tails: rows beyond M and columns beyond H feed zeros or clamped addresses and are not stored.
#include "common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kRows = 64;           // rows of a staged tile (4 MFMA tiles)
constexpr int kCols = 64;           // columns of a block: 16 per wave
constexpr int kThreads = 256;
constexpr int kMaxN = 64;           // thresholds per batch row, and basis functions
constexpr int kEs = 68;             // LDS row stride of the cosine tile (rows stay on 16 bytes)
constexpr int kTargetWgs = 512;     // strip width: see the head of the file
constexpr int kSlabRows = 256;      // rows of one dW / db slab
constexpr int kTs = 20;             // LDS row stride of a transposed dpre tile

struct EmbArgs {
    const float *taus, *i_pi, *emb_in, *w, *b, *psi, *g;
    float *out, *emb_out, *dpsi, *dw, *db;      // dw / db: the gradients themselves or slab 0
    long long slab_stride;                      // 0 with one slab
    int M, N, n, H;
    int per, strips;                            // column blocks per workgroup, workgroups per row tile
    int tile_rows;                              // dpsi: floor(64 / N) N
};

// Four consecutive floats k .. k + 3 of a row of K columns, clamped into the row; the caller zeroes
// what lies beyond it.  VEC: K % 4 == 0 and the row starts on 16 bytes.
template <bool VEC>
__device__ __forceinline__ float4 load4(const float *__restrict__ row, int k, int K) {
    if (VEC) return *reinterpret_cast<const float4 *>(row + min(k, K - 4));
    return make_float4(row[min(k, K - 1)], row[min(k + 1, K - 1)], row[min(k + 2, K - 1)],
                       row[min(k + 3, K - 1)]);
}

// This lane's A operand: W[hrow][16 b + 4 kq + i], zero beyond n.
template <bool VECW>
__device__ __forceinline__ void load_w(const float *__restrict__ wrow, int n, int nb, int kq, float (&wv)[4][4]) {
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const int k = 16 * b + 4 * kq, left = n - k;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (b < nb) v = load4<VECW>(wrow, k, n);
        wv[b][0] = left > 0 ? v.x : 0.f, wv[b][1] = left > 1 ? v.y : 0.f;
        wv[b][2] = left > 2 ? v.z : 0.f, wv[b][3] = left > 3 ? v.w : 0.f;
    }
}

// This lane's B operands of T row tiles from the staged cosine tile: row 16 t + c16, k = 16 b + 4 kq + i.
template <int T>
__device__ __forceinline__ void load_e(const float *tile, int t0, int c16, int kq, float4 (&ev)[T][4]) {
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
        for (int b = 0; b < 4; ++b)
            ev[t][b] = *reinterpret_cast<const float4 *>(tile + (16 * (t0 + t) + c16) * kEs + 16 * b + 4 * kq);
}

// acc[t][v] = sum_k W[h0 + 4 kq + v][k] cos[16 t + c16][k]: ONE order of the sum per accumulator
// (block, then element) in the forward and in both backward kernels.
template <int T>
__device__ __forceinline__ void pre_tiles(const float (&wv)[4][4], const float4 (&ev)[T][4], int nb, f32x4 (&acc)[T]) {
#pragma unroll
    for (int t = 0; t < T; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        if (b >= nb) break;
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const float e[4] = {ev[t][b].x, ev[t][b].y, ev[t][b].z, ev[t][b].w};
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[b][i], e[i], acc[t], 0, 0, 0);
        }
    }
}

// Four consecutive columns h .. h + 3 of a row of H: 16 bytes, or the elements below H (zeros beyond).
template <bool VECH>
__device__ __forceinline__ float4 load_h(const float *__restrict__ row, int h, int H) {
    if (VECH) return *reinterpret_cast<const float4 *>(row + h);
    return make_float4(row[h], h + 1 < H ? row[h + 1] : 0.f, h + 2 < H ? row[h + 2] : 0.f,
                       h + 3 < H ? row[h + 3] : 0.f);
}

template <bool VECH>
__device__ __forceinline__ void store_h(float *__restrict__ row, int h, int H, float4 v) {
    if (VECH) {
        *reinterpret_cast<float4 *>(row + h) = v;
        return;
    }
    row[h] = v.x;
    if (h + 1 < H) row[h + 1] = v.y;
    if (h + 2 < H) row[h + 2] = v.z;
    if (h + 3 < H) row[h + 3] = v.w;
}

__device__ __forceinline__ float relu_pre(float acc, float bias) {
    const float pre = acc + bias;
    return pre > 0.f ? pre : 0.f;
}

template <bool VECW, bool VECH>
__global__ __launch_bounds__(kThreads) void k_iqn_embed_fwd(EmbArgs a) {
    __shared__ __attribute__((aligned(16))) float tile[kRows * kEs];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int c16 = lane & 15, kq = lane >> 4;
    const int M = a.M, n = a.n, H = a.H;
    const int rt = blockIdx.x / a.strips, strip = blockIdx.x - rt * a.strips;
    const int row0 = rt * kRows;

    // the cosine tile, once per workgroup; zeros beyond M and beyond n
    for (int e = threadIdx.x; e < kRows * kMaxN; e += kThreads) {
        const int r = e >> 6, i = e & 63, row = row0 + r;
        float c = 0.f;
        if (row < M && i < n) {
            c = cosf(a.taus[row] * a.i_pi[i]);
            if (a.emb_out != nullptr && strip == 0) a.emb_out[(size_t)row * n + i] = c;
        }
        tile[r * kEs + i] = c;
    }
    __syncthreads();
    float4 ev[4][4];
    load_e<4>(tile, 0, c16, kq, ev);
    const float *prow[4];                   // this lane's four rows: their batch row of psi
#pragma unroll
    for (int t = 0; t < 4; ++t) prow[t] = a.psi + (size_t)(min(row0 + 16 * t + c16, M - 1) / a.N) * H;

    const int nb = (n + 15) >> 4, ncb = (H + kCols - 1) / kCols;
    const int cb_end = min((strip + 1) * a.per, ncb);
    for (int cb = strip * a.per; cb < cb_end; ++cb) {
        const int hb = cb * kCols + 16 * wave;
        if (hb >= H) break;                 // (wave-uniform; no barrier below)
        float wv[4][4];
        load_w<VECW>(a.w + (size_t)min(hb + c16, H - 1) * n, n, nb, kq, wv);
        f32x4 acc[4];
        pre_tiles<4>(wv, ev, nb, acc);
        const int h = hb + 4 * kq;
        if (h >= H) continue;
        const float4 bv = load_h<VECH>(a.b, h, H);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int row = row0 + 16 * t + c16;
            if (row >= M) continue;
            const float4 p = load_h<VECH>(prow[t], h, H);
            store_h<VECH>(a.out + (size_t)row * H, h, H,
                          make_float4(p.x * relu_pre(acc[t][0], bv.x), p.y * relu_pre(acc[t][1], bv.y),
                                      p.z * relu_pre(acc[t][2], bv.z), p.w * relu_pre(acc[t][3], bv.w)));
        }
    }
}

// Rows row0 .. row0 + rows - 1 of the saved cosines into the LDS tile, zeros beyond them and beyond n.
__device__ __forceinline__ void stage_emb(float *tile, const float *__restrict__ emb, int row0, int rows, int n) {
    for (int e = threadIdx.x; e < kRows * kMaxN; e += kThreads) {
        const int r = e >> 6, i = e & 63;
        tile[r * kEs + i] = r < rows && i < n ? emb[(size_t)(row0 + r) * n + i] : 0.f;
    }
}

template <bool VECW, bool VECH>
__global__ __launch_bounds__(kThreads) void k_iqn_embed_dpsi(EmbArgs a) {
    __shared__ __attribute__((aligned(16))) float tile[kRows * kEs];
    __shared__ float red[4][kRows][17];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int c16 = lane & 15, kq = lane >> 4;
    const int M = a.M, N = a.N, n = a.n, H = a.H;
    const int rt = blockIdx.x / a.strips, strip = blockIdx.x - rt * a.strips;
    const int row0 = rt * a.tile_rows, rows = min(a.tile_rows, M - row0);     // whole batch rows
    const int bb0 = row0 / N, nbt = rows / N;

    stage_emb(tile, a.emb_in, row0, rows, n);
    __syncthreads();
    float4 ev[4][4];
    load_e<4>(tile, 0, c16, kq, ev);

    const int nb = (n + 15) >> 4, ncb = (H + kCols - 1) / kCols;
    const int cb_end = min((strip + 1) * a.per, ncb);
    for (int cb = strip * a.per; cb < cb_end; ++cb) {     // (every wave makes every trip: barriers inside)
        const int hb = cb * kCols + 16 * wave;
        float wv[4][4];
        load_w<VECW>(a.w + (size_t)min(hb + c16, H - 1) * n, n, nb, kq, wv);
        f32x4 acc[4];
        pre_tiles<4>(wv, ev, nb, acc);
        const int h = hb + 4 * kq;
        float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
        if (h < H) bv = load_h<VECH>(a.b, h, H);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int r = 16 * t + c16;
            float4 gv = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r < rows && h < H) gv = load_h<VECH>(a.g + (size_t)(row0 + r) * H, h, H);
            red[wave][r][4 * kq + 0] = gv.x * relu_pre(acc[t][0], bv.x);
            red[wave][r][4 * kq + 1] = gv.y * relu_pre(acc[t][1], bv.y);
            red[wave][r][4 * kq + 2] = gv.z * relu_pre(acc[t][2], bv.z);
            red[wave][r][4 * kq + 3] = gv.w * relu_pre(acc[t][3], bv.w);
        }
        __syncthreads();
        // one thread per (batch row, column): the segment's N rows in row order
        if (hb + c16 < H)
            for (int q = kq; q < nbt; q += 4) {
                float s = red[wave][q * N][c16];
                for (int j = 1; j < N; ++j) s += red[wave][q * N + j][c16];
                a.dpsi[(size_t)(bb0 + q) * H + hb + c16] = s;
            }
        __syncthreads();
    }
}

template <bool VECW, bool VECH>
__global__ __launch_bounds__(kThreads) void k_iqn_embed_dw(EmbArgs a) {
    __shared__ __attribute__((aligned(16))) float tile[kRows * kEs];
    __shared__ __attribute__((aligned(16))) float tr[4][2][16 * kTs];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int c16 = lane & 15, kq = lane >> 4;
    const int M = a.M, N = a.N, n = a.n, H = a.H;
    const int slab = blockIdx.x / a.strips, cb = blockIdx.x - slab * a.strips;
    const int rs = slab * kSlabRows, re = min(rs + kSlabRows, M);
    const int hb = cb * kCols + 16 * wave, h = hb + 4 * kq;
    const int nb = (n + 15) >> 4;

    // (a wave whose columns lie beyond H runs along on clamped addresses and stores nothing: the
    // barriers below are the workgroup's)
    float wv[4][4];
    load_w<VECW>(a.w + (size_t)min(hb + c16, H - 1) * n, n, nb, kq, wv);
    float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (h < H) bv = load_h<VECH>(a.b, h, H);
    f32x4 dacc[4], bacc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) dacc[j] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int r0 = rs; r0 < re; r0 += kRows) {
        __syncthreads();                    // the tile's readers of the trip before
        stage_emb(tile, a.emb_in, r0, min(kRows, re - r0), n);
        __syncthreads();
        for (int t = 0; t < 4 && r0 + 16 * t < re; ++t) {
            float4 ev[1][4];
            load_e<1>(tile, t, c16, kq, ev);
            f32x4 acc[1];
            pre_tiles<1>(wv, ev, nb, acc);
            // dpre[row = r0 + 16 t + c16][h .. h + 3], zero outside the slab and beyond H
            const int row = r0 + 16 * t + c16;
            float d[4] = {0.f, 0.f, 0.f, 0.f};
            if (row < re && h < H) {
                const float4 gv = load_h<VECH>(a.g + (size_t)row * H, h, H);
                const float4 p = load_h<VECH>(a.psi + (size_t)(row / N) * H, h, H);
                d[0] = acc[0][0] + bv.x > 0.f ? gv.x * p.x : 0.f;
                d[1] = acc[0][1] + bv.y > 0.f ? gv.y * p.y : 0.f;
                d[2] = acc[0][2] + bv.z > 0.f ? gv.z * p.z : 0.f;
                d[3] = acc[0][3] + bv.w > 0.f ? gv.w * p.w : 0.f;
            }
            // transpose: the A operand of dpre^T cos wants lane (h, rows 4 kq .. 4 kq + 3)
            float *x = tr[wave][t & 1];
#pragma unroll
            for (int v = 0; v < 4; ++v) x[(4 * kq + v) * kTs + c16] = d[v];
            __syncthreads();
            const float4 dv = *reinterpret_cast<const float4 *>(x + c16 * kTs + 4 * kq);
            const float dt[4] = {dv.x, dv.y, dv.z, dv.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float *erow = tile + (16 * t + 4 * kq + i) * kEs + c16;
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j < nb) dacc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(dt[i], erow[16 * j], dacc[j], 0, 0, 0);
                bacc = __builtin_amdgcn_mfma_f32_16x16x4f32(dt[i], 1.f, bacc, 0, 0, 0);
            }
        }
    }
    // dacc[j][v] = dW[h + v][16 j + c16] of this slab; bacc[v] = db[h + v] in every column
    float *dw = a.dw + (size_t)slab * a.slab_stride, *db = a.db + (size_t)slab * a.slab_stride;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        if (h + v >= H) break;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (16 * j + c16 < n) dw[(size_t)(h + v) * n + 16 * j + c16] = dacc[j][v];
        if (c16 == 0) db[h + v] = bacc[v];
    }
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

const char *check_shape(int32_t B, int32_t N, int32_t n, int32_t H) {
    if (B < 1 || H < 1) return "pfrl_iqn_embed: at least one batch row and one hidden unit";
    if (N < 1 || N > kMaxN) return "pfrl_iqn_embed: 1 <= thresholds per row <= 64";
    if (n < 1 || n > kMaxN) return "pfrl_iqn_embed: 1 <= basis functions <= 64";
    if ((int64_t)B * N * H >= ((int64_t)1 << 31) || (int64_t)H * n >= ((int64_t)1 << 31))
        return "pfrl_iqn_embed: 2^31 output or weight elements or more";
    return nullptr;
}

// Column blocks per workgroup for `tiles` row tiles (the head of the file), and the workgroups per tile.
void strip_plan(int64_t tiles, int H, int *per, int *strips) {
    const int ncb = (H + kCols - 1) / kCols;
    const int64_t p = tiles * ncb / kTargetWgs;
    *per = (int)(p < 1 ? 1 : p > ncb ? ncb : p);
    *strips = (ncb + *per - 1) / *per;
}

int64_t r4(int64_t v) { return (v + 3) & ~(int64_t)3; }

#define PFRL_IQN_EMBED_LAUNCH(KERNEL, GRID)                                                             \
    do {                                                                                                \
        if (vecw && vech)                                                                               \
            hipLaunchKernelGGL((KERNEL<true, true>), dim3(GRID), dim3(kThreads), 0, st, a);             \
        else if (vecw)                                                                                  \
            hipLaunchKernelGGL((KERNEL<true, false>), dim3(GRID), dim3(kThreads), 0, st, a);            \
        else if (vech)                                                                                  \
            hipLaunchKernelGGL((KERNEL<false, true>), dim3(GRID), dim3(kThreads), 0, st, a);            \
        else                                                                                            \
            hipLaunchKernelGGL((KERNEL<false, false>), dim3(GRID), dim3(kThreads), 0, st, a);           \
    } while (0)

}  // namespace

extern "C" int pfrl_iqn_embed_fwd(const float *taus, const float *i_pi, const float *w, const float *b,
                                  const float *psi, float *out, float *emb, int32_t B, int32_t N, int32_t n,
                                  int32_t H, void *stream) {
    PFRL_CHECK_ARG(taus && i_pi && w && b && psi && out, "pfrl_iqn_embed_fwd: null pointer");
    const char *bad = check_shape(B, N, n, H);
    PFRL_CHECK_ARG(bad == nullptr, bad);
    EmbArgs a{};
    a.taus = taus, a.i_pi = i_pi, a.w = w, a.b = b, a.psi = psi, a.out = out, a.emb_out = emb;
    a.M = B * N, a.N = N, a.n = n, a.H = H;
    const int64_t tiles = ((int64_t)a.M + kRows - 1) / kRows;
    strip_plan(tiles, H, &a.per, &a.strips);
    const bool vecw = n % 4 == 0 && aligned16(w);
    const bool vech = H % 4 == 0 && aligned16(b) && aligned16(psi) && aligned16(out);
    hipStream_t st = (hipStream_t)stream;
    PFRL_IQN_EMBED_LAUNCH(k_iqn_embed_fwd, (unsigned)(tiles * a.strips));
    PFRL_LAUNCH_CHECK();
}

extern "C" int pfrl_iqn_embed_bwd(const float *g, const float *emb, const float *w, const float *b,
                                  const float *psi, float *dpsi, float *dw, float *db, float *part,
                                  int64_t part_floats, int32_t B, int32_t N, int32_t n, int32_t H,
                                  void *stream) {
    PFRL_CHECK_ARG(g && emb && w && b && psi && dpsi && dw && db, "pfrl_iqn_embed_bwd: null pointer");
    const char *bad = check_shape(B, N, n, H);
    PFRL_CHECK_ARG(bad == nullptr, bad);
    const int M = B * N;
    const int64_t slabs = ((int64_t)M + kSlabRows - 1) / kSlabRows;
    const int64_t db_off = r4((int64_t)H * n), stride = db_off + r4(H);
    if (slabs > 1)
        PFRL_CHECK_ARG(part && part_floats >= slabs * stride && aligned16(part) && aligned16(dw) && aligned16(db),
                       "pfrl_iqn_embed_bwd: more than 256 rows need a 16-byte aligned workspace of "
                       "ceil(M / 256) (r4(H n) + r4(H)) floats and 16-byte aligned dw / db");
    EmbArgs a{};
    a.g = g, a.emb_in = emb, a.w = w, a.b = b, a.psi = psi, a.dpsi = dpsi;
    a.M = M, a.N = N, a.n = n, a.H = H;
    const bool vecw = n % 4 == 0 && aligned16(w);
    const bool vech = H % 4 == 0 && aligned16(b) && aligned16(psi) && aligned16(g);
    hipStream_t st = (hipStream_t)stream;

    a.tile_rows = kRows / N * N;
    const int64_t tiles = ((int64_t)M + a.tile_rows - 1) / a.tile_rows;
    strip_plan(tiles, H, &a.per, &a.strips);
    PFRL_IQN_EMBED_LAUNCH(k_iqn_embed_dpsi, (unsigned)(tiles * a.strips));

    a.per = 1, a.strips = (H + kCols - 1) / kCols;
    a.dw = slabs > 1 ? part : dw, a.db = slabs > 1 ? part + db_off : db;
    a.slab_stride = slabs > 1 ? stride : 0;
    PFRL_IQN_EMBED_LAUNCH(k_iqn_embed_dw, (unsigned)(slabs * a.strips));
    if (slabs > 1) {
        const float *parts[2] = {part, part + db_off};
        float *outs[2] = {dw, db};
        const int64_t strides[2] = {stride, stride};
        const int32_t ns[2] = {H * n, H}, splits[2] = {(int32_t)slabs, (int32_t)slabs};
        return pfrl_splitk_reduce(2, parts, outs, nullptr, strides, ns, splits, nullptr, nullptr, stream);
    }
    PFRL_LAUNCH_CHECK();
}
