// Fixed-order reductions shared by the "one thread per row" loss launches: a wave butterfly, the
// fold of a workgroup's wave sums into its row of partial[block][cols], and the fold of one column
// of that workspace by the one-wave finish kernels.  Every sum has one order (lanes by butterfly,
// waves in wave order, blocks in block order), so the same operands give the same bits on every
// run and in every kernel that uses these functions.  No float atomics.
#pragma once
#include <hip/hip_runtime.h>

namespace {

// Butterfly over the 64 lanes (offsets 32 .. 1): the sum, in every lane.
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ float wave_sum_f32(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// The sum of a 256-thread workgroup (four waves) in every thread: butterfly per wave, then the four
// wave sums folded pairwise through sh[4].
__device__ __forceinline__ float block_sum(float v, float *sh) {
    v = wave_sum_f32(v);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

__device__ __forceinline__ float torch_min(float a, float b) {   // NaN-propagating, as torch.min
    return (a < b || a != a) ? a : b;
}

// s_red[k][w] holds wave w's sum of quantity k (written by lane 0 of each wave).  Thread k < n adds
// the waves of row k in wave order and writes partial[block][k]; the rows of partial are `cols`
// wide (n when not given: a kernel that fills only the head of its rows passes the full width).
template <int ROWS, int WAVES>
__device__ __forceinline__ void block_fold(double (&s_red)[ROWS][WAVES], int n,
                                           double *__restrict__ partial, int cols = 0) {
    __syncthreads();
    if ((int)threadIdx.x < n) {
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) t += s_red[threadIdx.x][w];
        partial[(size_t)blockIdx.x * (cols ? cols : n) + threadIdx.x] = t;
    }
}

// Column k of partial[nblk][cols] summed by a one-wave workgroup: lane l adds blocks l, l + 64, ...
// in block order, then the butterfly.  The sum, in every lane.
__device__ __forceinline__ double fold_column(const double *__restrict__ partial, int nblk, int cols,
                                              int k) {
    double s = 0.0;
    for (int b = threadIdx.x; b < nblk; b += 64) s += partial[(size_t)b * cols + k];
    return wave_sum_f64(s);
}

}  // namespace
