// What the recurrent kernels share (lstm.hip, lstm_seq.hip, gru.hip, gru_seq.hip): every one of them
// is a skinny reduction on the 16x16x4 MFMA whose K range is split over the waves of a workgroup,
// folded through LDS, with the cell arithmetic as the epilogue of the folding thread.  One copy of
// the rules that make the same inputs give the same bits on every launch:
//
// Load form.  Lane (c = lane & 15, kq = lane >> 4) loads the four floats k0 + 4 kq .. + 3 of its row
// for a block of 16 k, as ONE 16-byte load where the rows allow it (VEC) and as four clamped dword
// loads otherwise, and MFMA step i of the block takes element i of every lane's four for BOTH
// operands (any bijection of k serves a reduction).  All loads of a trip of UNR blocks stand before
// its first MFMA, with no branch between them, so that they can be in flight together.
// Tails.  k beyond the reduction enters as zeros: clamped address, masked value.  The select sits at
// the MFMA, not at the load (there it would wait for the load), and a short last trip repeats its
// last block as zeros rather than branching round it (the loads of a block behind a branch would
// sink into it).  Rows and units beyond the last valid one repeat it and are not stored.
// Fold.  A wave writes its partial tiles to LDS; one thread per (row, column) adds them starting
// from wave 0's, then wave 1's, 2's, ...: no atomics, one order of every sum.
#pragma once
#include <type_traits>
#include <vector>

#include "common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x4 __attribute__((ext_vector_type(4)));

// Packed fp32 arithmetic (two floats per VALU op) is switched off for these kernels, in the source so
// that every build path agrees: the compiler emits none here today, and the fixed-order sums below
// are not to change form with a compiler that would.
#if defined(__HIP_DEVICE_COMPILE__)
#define PFRL_NO_PACKED_FP32 __attribute__((target("no-packed-fp32-ops")))
#else
#define PFRL_NO_PACKED_FP32
#endif

constexpr int kRowsPerWg = 64;      // 4 M-tiles
constexpr int kMaxRows = 256;       // blockIdx.y <= 4: the admitted envelope
constexpr int kPad = 17;            // LDS row stride of a partial tile

// Four consecutive floats k .. k + 3 of a matrix row of K columns; addresses beyond the row are
// clamped into it and the caller zeroes those elements when it uses them.  VEC: K % 4 == 0 and the
// row starts on 16 bytes (k is always a multiple of 4), so the four are in or out together.
template <bool VEC>
__device__ __forceinline__ float4 load4(const float *__restrict__ row, int k, int K) {
    if (VEC) return *reinterpret_cast<const float4 *>(row + min(k, K - 4));
    return make_float4(row[min(k, K - 1)], row[min(k + 1, K - 1)], row[min(k + 2, K - 1)],
                       row[min(k + 3, K - 1)]);
}

__device__ __forceinline__ float sigmoidf(float v) { return 1.f / (1.f + expf(-v)); }

__device__ __forceinline__ void mfma_16x16x4(f32x4 &acc, float a, float b) {
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
}
__device__ __forceinline__ void mfma_16x16x4(f64x4 &acc, float a, float b) {     // widened at the MFMA
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64((double)a, (double)b, acc, 0, 0, 0);
}

// One load trip's MFMAs into f32 (ACC = f32x4) or f64 (f64x4) accumulators: UNR blocks, MT M-tiles,
// element i of every lane's four for both operands; left[j] = columns of the row from this lane's k
// on in block j, 0 for a block that only repeats.  Order: block, M-tile, element.
template <typename ACC, int MT, int UNR>
__device__ __forceinline__ void mfma_trip(ACC (&acc)[MT], const float4 (&w)[UNR], const float4 (&v)[UNR][MT],
                                          const int (&left)[UNR]) {
#pragma unroll
    for (int j = 0; j < UNR; ++j) {
        const float wv[4] = {left[j] > 0 ? w[j].x : 0.f, left[j] > 1 ? w[j].y : 0.f,
                             left[j] > 2 ? w[j].z : 0.f, left[j] > 3 ? w[j].w : 0.f};
#pragma unroll
        for (int t = 0; t < MT; ++t) {
            const float av[4] = {left[j] > 0 ? v[j][t].x : 0.f, left[j] > 1 ? v[j][t].y : 0.f,
                                 left[j] > 2 ? v[j][t].z : 0.f, left[j] > 3 ? v[j][t].w : 0.f};
#pragma unroll
            for (int i = 0; i < 4; ++i) mfma_16x16x4(acc[t], av[i], wv[i]);
        }
    }
}

// The nb blocks of 16 k over WAVES waves: wave w takes [share_begin(w, nb), share_begin(w + 1, nb)).
template <int WAVES>
__device__ __forceinline__ int share_begin(int wave, int nb) {
    return wave * nb / WAVES;
}

// The A-operand rows of lane column c16, one per M-tile, from the workgroup's row0 on; those beyond
// `last` repeat it.
template <int MT>
__device__ __forceinline__ void clamp_rows(unsigned (&arow)[MT], int row0, int c16, int last) {
#pragma unroll
    for (int t = 0; t < MT; ++t) arow[t] = (unsigned)min(row0 + 16 * t + c16, last);
}

// M-tile t of a wave's partial tiles to its part of LDS, [WAVES][16 MT rows][kPad].
// f32 accumulator layout: row = 4 (lane >> 4) + i, column = lane & 15
template <int WAVES, int ROWS>
__device__ __forceinline__ void store_partial(float (&part)[WAVES][ROWS][kPad], int wave, int t, f32x4 acc, int c16, int kq) {
#pragma unroll
    for (int i = 0; i < 4; ++i) part[wave][16 * t + 4 * kq + i][c16] = acc[i];
}

// f64 accumulator layout: row = (lane >> 4) + 4 i, column = lane & 15
template <int WAVES, int ROWS>
__device__ __forceinline__ void store_partial(double (&part)[WAVES][ROWS][kPad], int wave, int t, f64x4 acc, int c16, int kq) {
#pragma unroll
    for (int i = 0; i < 4; ++i) part[wave][16 * t + kq + 4 * i][c16] = acc[i];
}

// Element (r, c) of the tile, folded in wave order (after the barrier that follows the stores).
template <typename T, int WAVES, int ROWS>
__device__ __forceinline__ T fold_waves(const T (&part)[WAVES][ROWS][kPad], int r, int c) {
    T s = part[0][r][c];
#pragma unroll
    for (int wv = 1; wv < WAVES; ++wv) s += part[wv][r][c];
    return s;
}

// The reduction of the two cell kernels into acc (zeroed here): the I columns of x against W_ih
// followed by the H columns of h0 against W_hh (none when h0 is NULL) as ONE range of blocks shared
// by the WAVES waves.  `grow` is the lane's weight row in both matrices; loads_w(hh) says whether
// this lane's column reduces over the x part (hh false) / the h part (hh true) of the range: where
// not, it loads nothing and feeds zeros.
template <int WAVES, int UNR, bool VEC, int MT, typename LOADS_W>
__device__ __forceinline__ void reduce_concat(f32x4 (&acc)[MT], const float *x, const float *h0, const float *w_ih,
                                              const float *w_hh, int I, int H, unsigned grow,
                                              const unsigned (&arow)[MT], int wave, int kq, LOADS_W loads_w) {
    const int nb0 = (I + 15) >> 4, nb = nb0 + (h0 != nullptr ? (H + 15) >> 4 : 0);
    const int b_begin = share_begin<WAVES>(wave, nb), b_end = share_begin<WAVES>(wave + 1, nb);
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
            const float *__restrict__ wm = hh ? w_hh : w_ih;
            const float *__restrict__ am = hh ? h0 : x;
            left[j] = b + j < b_end ? K - k : 0;
            w[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (loads_w(hh)) w[j] = load4<VEC>(wm + (size_t)grow * K, k, K);
#pragma unroll
            for (int t = 0; t < MT; ++t) v[j][t] = load4<VEC>(am + (size_t)arow[t] * K, k, K);
        }
        mfma_trip(acc, w, v, left);
    }
}

inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// The envelope the sequence entries share; fills off[0 .. T] (first row of every step, and R).  The
// saved rows are 4H floats for both cell types, W_hh is `wgates` x H x H; `too_large` is the caller's
// message for either of them reaching 2^31 elements.
inline const char *check_sizes(const int32_t *bs, int32_t T, int32_t H, int wgates, const char *too_large,
                               std::vector<int64_t> &off) {
    if (bs == nullptr) return "null batch_sizes";
    if (T < 1 || H < 1) return "at least one time step and one hidden unit";
    off.assign((size_t)T + 1, 0);
    for (int t = 0; t < T; ++t) {
        if (bs[t] < 1 || (t > 0 && bs[t] > bs[t - 1])) return "batch sizes must be >= 1 and non-increasing";
        off[t + 1] = off[t] + bs[t];
    }
    if (bs[0] > kMaxRows) return "at most 256 rows per step";
    if (off[T] * 4 * H >= ((int64_t)1 << 31) || wgates * (int64_t)H * H >= ((int64_t)1 << 31)) return too_large;
    return nullptr;
}

// f(MT, VEC) with MT = 1 / 2 / 4 M-tiles for up to 16 / 32 / more rows and VEC = vec, both as
// std::integral_constant: the caller's generic lambda names its kernel instantiation from them.
template <typename F>
void with_tiles(int rows, bool vec, F &&f) {
    auto with_vec = [&](auto mt) {
        if (vec)
            f(mt, std::true_type{});
        else
            f(mt, std::false_type{});
    };
    if (rows <= 16)
        with_vec(std::integral_constant<int, 1>{});
    else if (rows <= 32)
        with_vec(std::integral_constant<int, 2>{});
    else
        with_vec(std::integral_constant<int, 4>{});
}

}  // namespace
