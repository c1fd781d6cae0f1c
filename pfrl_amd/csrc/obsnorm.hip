// The running statistics of an observation normaliser (nn/empirical_normalization.py, the reference's
// pfrl/nn/empirical_normalization.py:63-88) learn from a batch in TWO launches behind one entry point, in f64,
// without atomics and with one order of every sum -- where the module runs about ten library launches in f32
// and reads `count >= until` back to the host.
//
// k_obs_partial.  Grid (row slabs) x (groups of 64 columns); the slab count is a function of n alone (at most
// kMaxSlabs, at least 64 rows a slab while n allows).  A workgroup of four waves owns the [rows, 64] block of x:
// wave w takes the slab's rows w, w + 4, ..., lane c the column 64 g + c, so every load of a wave is 64
// consecutive floats of one row.  Each lane keeps (count, mean, M2) of its column in f64 registers (Welford:
// d = x - mean; mean += d / count; M2 += d (x - mean)) -- the mean / M2 form: a column of offset 1 000 and spread
// 0.01 loses nothing, where sum x^2 - (sum x)^2 / n in any precision first forms two numbers of 1e6 n.  The four
// waves' triples meet in LDS (6 KB) and wave 0 merges them in wave order (Chan: d = m_b - m_a;
// mean = m_a + d n_b / n; M2 = M2_a + M2_b + d^2 n_a n_b / n); the slab's (mean, M2) goes to the workspace
// ws[slab][2][D] (every element that the merge reads is written by this launch: no state survives a call).
//
// k_obs_merge.  One workgroup, one thread per column: the slabs in slab order by the same rule (a slab's count
// follows from n), the batch's mean m_x and biased variance v_x = M2 / n, then the module's rule in f64 on the
// widened buffers,
//   r = n / count_new;  d = m_x - mean;  mean += r d;  var += r (v_x - var + d (m_x - mean_new)),
// rounded ONCE to f32 into mean and var, in place, and count += n (int64, on the device).  With until >= 0 a
// call at count >= until writes nothing: the module's own test, made here, so the host never waits for count.
// Every thread reads count before the barrier behind which thread 0 writes it.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxSlabs = 64;
constexpr int kMinSlabRows = 64;
constexpr int kMaxD = 512;
constexpr int kMaxN = 65536;

__host__ __device__ inline int rows_per_slab(int n) {
    const int per = (n + kMaxSlabs - 1) / kMaxSlabs;
    return per < kMinSlabRows ? kMinSlabRows : per;
}
__host__ __device__ inline int slab_count(int n) { return (n + rows_per_slab(n) - 1) / rows_per_slab(n); }

// (n_a, m_a, M2_a) takes in (n_b, m_b, M2_b), n_b > 0
__device__ __forceinline__ void chan_merge(double &na, double &ma, double &qa, double nb, double mb, double qb) {
    const double n = na + nb, d = mb - ma;
    ma += d * (nb / n);
    qa += qb + d * d * (na * nb / n);
    na = n;
}

__global__ __launch_bounds__(kThreads) void k_obs_partial(const float *__restrict__ x, int n, int D,
                                                         double *__restrict__ ws) {
    __shared__ double sN[kWaves][64], sM[kWaves][64], sQ[kWaves][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = blockIdx.y * 64 + lane;
    const int per = rows_per_slab(n);
    const int r_begin = blockIdx.x * per, r_end = min(r_begin + per, n);
    double cnt = 0., mean = 0., m2 = 0.;
    if (col < D) {
        for (int r = r_begin + wave; r < r_end; r += kWaves) {
            const double v = (double)x[(size_t)r * D + col];
            cnt += 1.;
            const double d = v - mean;
            mean += d / cnt;
            m2 += d * (v - mean);
        }
    }
    sN[wave][lane] = cnt;
    sM[wave][lane] = mean;
    sQ[wave][lane] = m2;
    __syncthreads();
    if (wave == 0 && col < D) {
        for (int w = 1; w < kWaves; ++w)
            if (sN[w][lane] > 0.) chan_merge(cnt, mean, m2, sN[w][lane], sM[w][lane], sQ[w][lane]);
        double *__restrict__ out = ws + (size_t)blockIdx.x * 2 * D;
        out[col] = mean;
        out[D + col] = m2;
    }
}

__global__ __launch_bounds__(kMaxD) void k_obs_merge(const double *__restrict__ ws, int n, int D,
                                                    float *__restrict__ mean, float *__restrict__ var,
                                                    long long *__restrict__ count, long long until) {
    const int col = threadIdx.x;
    const long long seen = *count;
    __syncthreads();                                          // (every thread has read count)
    if (until >= 0 && seen >= until) return;
    if (col == 0) *count = seen + n;
    if (col >= D) return;
    const int per = rows_per_slab(n), slabs = slab_count(n);
    double nb = (double)min(per, n), mb = ws[col], qb = ws[D + col];
    for (int s = 1; s < slabs; ++s) {
        const double *__restrict__ p = ws + (size_t)s * 2 * D;
        chan_merge(nb, mb, qb, (double)(min((s + 1) * per, n) - s * per), p[col], p[D + col]);
    }
    const double vx = qb / nb;
    const double m0 = (double)mean[col], v0 = (double)var[col];
    const double rate = (double)n / (double)(seen + n);
    const double d = mb - m0;
    const double m1 = m0 + rate * d;
    mean[col] = (float)m1;
    var[col] = (float)(v0 + rate * (vx - v0 + d * (mb - m1)));
}

}  // namespace

extern "C" int pfrl_obs_stats_update(const float *x, int32_t n, int32_t D, float *mean, float *var, int64_t *count,
                                     int64_t until, double *ws, int64_t ws_doubles, void *stream) {
    if (n == 0) return 0;
    PFRL_CHECK_ARG(n >= 1 && n <= kMaxN, "pfrl_obs_stats_update: 0 <= n <= 65536");
    PFRL_CHECK_ARG(D >= 1 && D <= kMaxD, "pfrl_obs_stats_update: 1 <= D <= 512");
    PFRL_CHECK_ARG(x != nullptr && mean != nullptr && var != nullptr && count != nullptr && ws != nullptr,
                   "pfrl_obs_stats_update: null pointer");
    PFRL_CHECK_ARG(((uintptr_t)x & 3) == 0 && ((uintptr_t)mean & 3) == 0 && ((uintptr_t)var & 3) == 0 &&
                       ((uintptr_t)count & 7) == 0 && ((uintptr_t)ws & 7) == 0,
                   "pfrl_obs_stats_update: misaligned pointer");
    const int slabs = slab_count(n);
    PFRL_CHECK_ARG(ws_doubles >= (int64_t)slabs * 2 * D,
                   "pfrl_obs_stats_update: workspace below slabs * 2 * D doubles");
    hipLaunchKernelGGL(k_obs_partial, dim3(slabs, (D + 63) / 64), dim3(kThreads), 0, (hipStream_t)stream, x, (int)n,
                       (int)D, ws);
    hipLaunchKernelGGL(k_obs_merge, dim3(1), dim3(kMaxD), 0, (hipStream_t)stream, (const double *)ws, (int)n, (int)D,
                       mean, var, (long long *)count, (long long)until);
    PFRL_LAUNCH_CHECK();
}
