"""NumPy restatement of the row arithmetic of csrc/boltzmann_row.h (``pfrl_dqn_act_head_boltzmann``,
``pfrl_boltzmann_select``), shared by tests/test_boltzmann_cpu.py and tests/test_boltzmann_head.py.

Two halves.  ``probs_f32``: softmax(q / T) in float32, every step one rounded operation in the
header's order -- equal to the kernels' up to the ``expf`` implementation.  ``actions``: from float32
probabilities on, ``np.random.choice(arange(A), p=p)`` with the uniform given instead of drawn
(numpy/random/mtrand.pyx: ``cdf = p.cumsum(); cdf /= cdf[-1]; cdf.searchsorted(u, side="right")``
on p as float64) -- everything float64 in a fixed order, so equal to the kernels' bit for bit.
"""
import numpy as np

U_MAX = 1.0 - 2.0 ** -53            # the largest value random_sample() returns


def probs_f32(q, T):
    q = np.asarray(q, dtype=np.float32)
    T = np.float32(T)
    with np.errstate(all="ignore"):
        z = q / T
        e = np.exp(z - z.max(axis=1, keepdims=True))
        s = e[:, 0].copy()
        for n in range(1, q.shape[1]):
            s = s + e[:, n]
        p = e / s[:, None]
    assert p.dtype == np.float32
    return p


def actions(p, u):
    """int64 [M]: the number of cdf entries <= u per row; -1 where a probability is NaN."""
    p = np.asarray(p)
    assert p.dtype == np.float32 and p.ndim == 2
    u = np.asarray(u, dtype=np.float64)
    with np.errstate(all="ignore"):
        c = np.zeros(p.shape, dtype=np.float64)
        acc = np.zeros(p.shape[0], dtype=np.float64)
        for n in range(p.shape[1]):             # c_n = c_(n-1) + (double) p_n, as np.cumsum
            acc = acc + p[:, n].astype(np.float64)
            c[:, n] = acc
        c = c / c[:, -1:]
        a = (c <= u[:, None]).sum(axis=1).astype(np.int64)
    a[np.isnan(p).any(axis=1)] = -1
    return a


def planted_rows(A=6):
    """(q f32 [R, A], T, u f64 [R], nan_rows bool [R]): the edge rows both tiers check."""
    assert A >= 3
    inf = np.float32(np.inf)
    rows, us, bad = [], [], []

    def add(row, u, nan=False):
        rows.append(np.asarray(row, dtype=np.float32))
        us.append(u)
        bad.append(nan)

    ramp = np.linspace(-1.0, 1.0, A)
    for u in (0.0, U_MAX, 0.5):
        add(ramp, u)                                    # the ends of the uniform's range
        add(np.zeros(A), u)                             # all tied
        add(np.r_[np.full(A - 1, 2.0), 0.0], u)         # ties in front of a smaller entry
        add(np.r_[0.0, 1000.0, np.zeros(A - 2)], u)     # all the mass on one action, the rest 0
        add(np.r_[np.zeros(A - 1), 1000.0], u)          # ... on the last: leading zeros in the cdf
        add(np.r_[1000.0, np.zeros(A - 1)], u)          # ... on the first: a flat tail of ones
        add(np.r_[-inf, 0.5, np.full(A - 2, -inf)], u)  # -inf entries: probability 0
        add(np.r_[0.0, -inf, ramp[2:]], u)
        add(np.r_[0.0, np.nan, ramp[2:]], u, nan=True)  # choice: "probabilities contain NaN"
        add(np.r_[np.nan, ramp[1:]], u, nan=True)
        add(np.r_[0.0, inf, ramp[2:]], u, nan=True)     # inf - inf
        add(np.full(A, -inf), u, nan=True)              # -inf - -inf
    return np.stack(rows), 1.0, np.asarray(us, dtype=np.float64), np.asarray(bad)
