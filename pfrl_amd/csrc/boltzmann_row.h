// Boltzmann exploration over one row of action values (pfrl/explorers/boltzmann.py:18-26), in the
// registers of ONE lane, shared by k_dqn_act_head_boltzmann (qnet.hip) and k_boltzmann_select
// (frames.hip): the two produce the same probabilities and the same action bit for bit from the
// same action values.  Every line is one rounded IEEE operation, in this order (the files are
// built with -ffp-contract=off), so that a NumPy restatement reproduces the action from the
// probabilities exactly (tests/test_boltzmann_cpu.py).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr int kMaxBoltzmannA = 64;

// row[0 .. A): the action values on entry, the probabilities on return (memory only this lane
// touches).  softmax(q / T) in float32: z = q / T, mx = max z, e = exp(z - mx), s = e_0 + e_1 + ..
// in index order, p = e / s.  Then `np.random.choice(arange(A), p=p)` with the host's draw u
// (numpy/random/mtrand.pyx, choice with replacement: cdf = p.cumsum() in float64, cdf /= cdf[-1],
// cdf.searchsorted(u, side="right")): the number of cdf entries <= u, at most A - 1 because
// cdf[-1] == 1 > u.  Returns -1 when a probability is NaN (choice raises "probabilities contain
// NaN": a NaN or +inf action value, a row of -inf).
__device__ __forceinline__ int64_t boltzmann_row(float *row, const int A, const float T, const double u) {
    float mx = row[0] = __fdiv_rn(row[0], T);
    for (int n = 1; n < A; ++n) {
        const float z = __fdiv_rn(row[n], T);
        row[n] = z;
        mx = fmaxf(mx, z);
    }
    float s = 0.f;
    for (int n = 0; n < A; ++n) {
        const float e = expf(row[n] - mx);
        row[n] = e;
        s += e;
    }
    double total = 0.0;
    bool bad = false;
    for (int n = 0; n < A; ++n) {
        const float p = __fdiv_rn(row[n], s);
        row[n] = p;
        bad |= p != p;
        total += (double)p;
    }
    double c = 0.0;
    int a = 0;
    for (int n = 0; n < A; ++n) {
        c += (double)row[n];
        a += __ddiv_rn(c, total) <= u ? 1 : 0;
    }
    if (bad) return -1;
    return a < A - 1 ? a : A - 1;     // (u >= 1 is no draw of random_sample: never an index past the row)
}

}  // namespace
