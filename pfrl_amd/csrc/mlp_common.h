// What the whole-MLP kernels share (mlp.hip: up to 64 wide, weights resident in LDS; mlp_wide.hip: up to
// 512 wide, weights streamed): the activation and its derivative from the activation's output, and the
// bounds-checked staging of a matrix into zero-padded LDS rows.  The MFMA fragment rule (lane (c, kq)
// takes the four floats k0 + 4 kq .. + 3 of its row, step i of a block pairs element i of both operands)
// is recurrent_mfma.h's.
#pragma once
#include "recurrent_mfma.h"

namespace {

__device__ __forceinline__ float activate(float v, int act) {
    return act == PFRL_MLP_TANH ? tanhf(v) : (v < 0.f ? 0.f : v);
}

// d times act'(a), from the activation's output
__device__ __forceinline__ float act_grad(float d, float a, int act) {
    return act == PFRL_MLP_TANH ? d * (1.f - a * a) : (a > 0.f ? d : 0.f);
}

// Element (gr, gc) of a row-major matrix with `ld` columns; zero beyond row nr - 1 and column nc - 1.
__device__ __forceinline__ float stage_elem(const float *__restrict__ src, int gr, int nr, int gc, int nc, int ld) {
    return gr < nr && gc < nc ? src[(size_t)gr * ld + gc] : 0.f;
}

// `rows` x 64 floats of a row-major matrix with `ld` columns, from (r0, c0) on, into dst (rows of LD
// floats); zeros beyond row nr - 1 and column nc - 1.  Consecutive threads take consecutive columns.
template <int THREADS, int LD>
__device__ __forceinline__ void stage(float (*dst)[LD], const float *__restrict__ src, int rows, int r0, int nr, int c0,
                                      int nc, int ld, int tid) {
    for (int idx = tid; idx < rows * 64; idx += THREADS) {
        const int r = idx >> 6, c = idx & 63;
        dst[r][c] = stage_elem(src, r0 + r, nr, c0 + c, nc, ld);
    }
}

inline bool aligned4(const void *p) { return ((uintptr_t)p & 3) == 0; }

}  // namespace
