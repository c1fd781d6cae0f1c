"""The NumPy references of tests/test_rollout_layer_envelope.py against the committed C oracle
(oracle/pfrl_oracle.c), the routes its case lists reach (the launchers' conditions restated here and
pinned to the sources), the exactness of its integer operands and the uncertainty of its float64
advantage statistics: no GPU needed."""
import math
import os
import re

import numpy as np
import pytest

import oracle
from test_rollout_layer_envelope import (A2C_N, A2C_T, ADV_BLOCK, ADV_CAP, ADV_CONST_C, ADV_CONST_N,
                                         ADV_N, BWD_C, BWD_HW, BWD_MULTI, EXACT_LIMIT, FWD_CAP_ITEMS,
                                         FWD_PLANAR, FWD_ROWMAJOR, GAE_CUTS, GAE_EDGE, GAE_HYPER,
                                         GAE_N, GAE_T, MB_CASES, NOISY_BWD_PTRS, NOISY_CAP_ITEMS,
                                         NOISY_FWD_PTRS, NOISY_MISALIGN_SHAPES, NOISY_SHAPES,
                                         NOISY_SPECIALS, REUSE, SMALL_C, SMALL_ROWS, a2c_inputs,
                                         adv_blocks, adv_input, bias_relu_plan, exact_operands,
                                         gae_cut, gae_inputs, noisy_r, noisy_v4, ref_a2c_returns,
                                         ref_adv_stats, ref_bwd, ref_gae, reuse_operand_sets, shaped)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64


def _same_bits(a, b, what=""):
    assert a.dtype == b.dtype == np.float32 and a.shape == b.shape
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32), err_msg=what)


def _src(name):
    return open(os.path.join(ROOT, "pfrl_amd", "csrc", name)).read()


# ---------------------------------------------------------------------------
# oracle pins
# ---------------------------------------------------------------------------
def oracle_gae(reward, v, nv, nt, cut, gamma, lambd, mode):
    """``orc_gae_fragment`` per env, on the fragments the cut flags delimit (a cut at t zeroes adv
    BEFORE step t, so step t is the last of a fragment that began after the previous cut)."""
    T, N = reward.shape
    adv, vt = np.empty((T, N), dtype=f32), np.empty((T, N), dtype=f32)
    for e in range(N):
        t0 = 0
        for t in range(T):
            if cut[t, e] or t == T - 1:
                sl = slice(t0, t + 1)
                a, b = oracle.gae_fragment(reward[sl, e], v[sl, e], nv[sl, e],
                                           (nt[sl, e] != 0).astype(f64), gamma, lambd, mode)
                adv[sl, e], vt[sl, e] = a.astype(f32), b.astype(f32)
                t0 = t + 1
    return adv, vt


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("T", [1, 2, 15, 16, 17, 33, 48])
def test_gae_reference_is_the_oracle(T, mode):
    rs = np.random.RandomState(T + mode)
    for N in (1, 9):
        for cut_kind in GAE_CUTS:
            for gamma, lambd in [(0.99, 0.95)] + GAE_HYPER:
                reward, v, nv, nt, cut = gae_inputs(rs, T, N, cut_kind)
                got = ref_gae(reward, v, nv, nt, cut, gamma, lambd, mode)
                want = oracle_gae(reward, v, nv, nt, cut, gamma, lambd, mode)
                what = "T=%d N=%d %s mode=%d" % (T, N, cut_kind, mode)
                _same_bits(got[0], want[0], what + " adv")
                _same_bits(got[1], want[1], what + " v_teacher")
                assert T * N < 100 or 0.1 < (nt == 0).mean() < 0.3


def test_gae_cut_patterns():
    for T in GAE_T + [630, 911]:
        assert not gae_cut("none", T, 9).any() and gae_cut("all", T, 9).all()
        first, last = gae_cut("first", T, 9), gae_cut("last", T, 9)
        assert first[0].all() and first.sum() == 9 and last[T - 1].all() and last.sum() == 9
        chunk = gae_cut("chunk", T, 9)
        u = (T - 1 - np.arange(T)) % 16
        assert (chunk[:, 0] != 0).tolist() == ((u == 0) | (u == 15)).tolist()
        assert chunk[T - 1, 0] and not chunk[:, 1].any()
        if T >= 17:
            assert chunk[T - 16, 0] and chunk[T - 17, 0] and not chunk[T - 2, 0]


@pytest.mark.parametrize("use_gae", [0, 1])
@pytest.mark.parametrize("T", A2C_T)
def test_a2c_reference_is_the_oracle(T, use_gae):
    rs = np.random.RandomState(T)
    for N in (1, 7, 257):
        rewards, masks, value_preds, bootstrap = a2c_inputs(rs, T, N)
        assert (masks[0] == 0).any() and (masks[T - 1] == 0).any() and set(masks.ravel()) <= {0, 1}
        init = np.zeros((T + 1, N), dtype=f32)
        vp = value_preds.copy()
        if use_gae:
            vp[T] = bootstrap
        else:
            init[T] = bootstrap
        got = ref_a2c_returns(rewards, masks, vp, init, 0.99, 0.95, use_gae)
        want = oracle.a2c_returns(rewards, masks, vp, bootstrap, 0.99, 0.95, use_gae)
        _same_bits(got[:T], want[:T])
        _same_bits(got[T], init[T])


def _exact_stats(x):
    """(mean, var, E[x^2]) from exactly rounded sums (``math.fsum``; x^2 is exact in float64)."""
    x = x.astype(f64)
    n = float(x.size)
    s1, s2 = math.fsum(x.tolist()), math.fsum((x * x).tolist())
    mean = s1 / n
    return mean, s2 / n - mean * mean, s2 / n


@pytest.mark.parametrize("n", ADV_N)
def test_adv_stats_reference_uncertainty_is_below_a_quarter_ulp(n):
    """The reference's own error: its distance from the same formula on exactly rounded sums, plus
    what the formula itself loses on those (two roundings on the mean; on the variance 4 u64 E[x^2],
    halved and divided by std for the root)."""
    x = adv_input(n)
    mean, std = ref_adv_stats(x)
    mean_e, var_e, ex2 = _exact_stats(x)
    u64 = 2.0 ** -53
    unc_mean = abs(mean - mean_e) + 2 * u64 * abs(mean_e)
    assert unc_mean < 0.25 * f64(np.spacing(np.abs(f32(mean)))), n
    if n == 1:
        assert std == 0.0 and var_e == 0.0
        return
    std_e = math.sqrt(var_e)
    assert abs(mean) <= 100 * std
    unc_std = abs(std - std_e) + 4 * u64 * ex2 / (2 * std_e) + u64 * std_e
    assert unc_std < 0.25 * f64(np.spacing(f32(std))), n
    # ... and the C oracle's two-pass statistics agree to well below an f32 ulp
    m_o, s_o = oracle.adv_stats(x)
    assert abs(m_o - mean) < 0.25 * f64(np.spacing(np.abs(f32(mean))))
    assert abs(s_o - std) < 0.25 * f64(np.spacing(f32(std)))


def test_adv_stats_constant_column_is_exact_in_float64():
    n, c = ADV_CONST_N, f32(ADV_CONST_C)
    assert f64(c) == ADV_CONST_C and (ADV_CONST_C * 128) == int(ADV_CONST_C * 128) < 256
    assert n < 2 ** 24
    x = np.full(n, c, dtype=f32)
    mean, std = ref_adv_stats(x)
    assert mean == f64(c) and std == 0.0
    assert _exact_stats(x)[:2] == (f64(c), 0.0)
    # what pfrl_ppo_minibatch makes of it
    assert ((x - f32(mean)) / (f32(std) + f32(1e-8)) == 0).all()


# ---------------------------------------------------------------------------
# route census: the launchers' conditions, restated and pinned to the sources
# ---------------------------------------------------------------------------
def test_launcher_conditions_are_the_ones_restated_here():
    rollout, bias, noisy = _src("rollout.hip"), _src("bias_act.hip"), _src("noisy.hip")
    assert "const int E = N >= 4096 ? 16 : 8;" in rollout
    assert "(size_t)T * E * ((mode == 0 ? 4 : 8) + 4 + 1)" in rollout
    assert "if (lds <= 64 * 1024 && T < (1 << 20))" in rollout
    assert "constexpr int kGaeChunk = 16;" in rollout
    assert "(n + kThreads * 8 - 1) / (kThreads * 8)" in rollout and ADV_BLOCK == 256 * 8
    assert "if (blocks > 1024) blocks = 1024;" in rollout and ADV_CAP == 1024
    assert "if (blocks > 2048) blocks = 2048;" in bias and FWD_CAP_ITEMS == 2048 * 256
    assert "if (blocks > 4096) blocks = 4096;" in noisy and NOISY_CAP_ITEMS == 4096 * 256
    for src in (rollout, bias, noisy):
        assert re.search(r"constexpr int kThreads = 256;", src)
    v4 = re.findall(r"const bool v4 = \(in_features & 3\) == 0 && ([^;]+);", noisy)
    assert len(v4) == 2
    assert re.findall(r"aligned16\((\w+)\)", v4[0]) == NOISY_FWD_PTRS
    assert re.findall(r"aligned16\((\w+)\)", v4[1]) == NOISY_BWD_PTRS
    # after the LDS launch the launcher returns: the macro returns on both branches
    common = _src("common.h")
    body = common[common.index("#define PFRL_LAUNCH_CHECK()"):]
    body = body[:body.index("while (0)")]
    assert "return (int)e__;" in body and "return 0;" in body


def gae_route(mode, T, N):
    E = 16 if N >= 4096 else 8
    lds = T * E * (9 if mode == 0 else 13)
    return ("lds" if lds <= 65536 else "lane"), E, mode, lds


def test_gae_cases_reach_every_route():
    cases = ([(m, T, N) for m in (0, 1, 2) for T in GAE_T for N in GAE_N] + GAE_EDGE
             + [(m, 33, 9) for m in (0, 1, 2)])
    routes = {gae_route(*c)[:3] for c in cases}
    assert {("lds", E, m) for E in (8, 16) for m in (0, 1, 2)} <= routes
    assert {("lane", 8, m) for m in (0, 1, 2)} | {("lane", 16, 0), ("lane", 16, 1)} <= routes
    # the limit from both sides: the largest rollouts that take the LDS form ask for 65 520 bytes
    for mode, T, N in [(0, 910, 9), (1, 630, 9), (2, 630, 9), (0, 455, 4097), (1, 315, 4097)]:
        assert (mode, T, N) in GAE_EDGE and (mode, T + 1, N) in GAE_EDGE
        assert gae_route(mode, T, N)[0] == "lds" and gae_route(mode, T, N)[3] == 65520
        assert gae_route(mode, T + 1, N)[0] == "lane"
    # the switch to E = 16 and a last workgroup with 1 / 15 live envs
    for m in (0, 1, 2):
        assert [gae_route(m, 17, N)[1] for N in (4095, 4096, 4097, 4111)] == [8, 16, 16, 16]
        assert all((m, 17, N) in GAE_EDGE for N in (4095, 4096, 4097, 4111))
        assert {N % 256 for mm, T, N in GAE_EDGE if mm == m and T == 1200} == {255, 0, 1}
    assert 4097 % 16 == 1 and 4111 % 16 == 15 and {N % 8 for N in GAE_N} >= {0, 1, 7}
    # the register chunk: fewer than one, exactly one, one more; two; three
    assert {T % 16 for T in GAE_T} >= {0, 1, 15} and {-(-T // 16) for T in GAE_T} == {1, 2, 3}
    assert (0.99, 0.0) in GAE_HYPER and (1.0, 0.95) in GAE_HYPER
    assert A2C_T == [1, 2, 5, 17] and A2C_N == [1, 255, 256, 257]


def test_adv_stats_cases_reach_the_cap_from_both_sides():
    planned = {n: -(-n // ADV_BLOCK) for n in ADV_N}
    assert [planned[n] for n in (2047, 2048, 2049)] == [1, 1, 2]
    assert planned[1024 * 2048 - 1] == planned[1024 * 2048] == 1024 and planned[1024 * 2048 + 1] == 1025
    assert max(planned.values()) > 1024 and {adv_blocks(n) for n in ADV_N} >= {1, 2, 1024}
    assert {n % 64 for n in ADV_N} >= {0, 1, 63} and ADV_CONST_N == 2049


def test_minibatch_cases():
    assert {M % 256 for M, _, _ in MB_CASES} == {0, 1, 255} and max(M for M, _, _ in MB_CASES) > 256
    assert {(k, A) for _, k, A in MB_CASES} == ({(k, None) for k in (1, 4)}
                                                | {(k, A) for k in (0, 1, 4) for A in (1, 3, 6)})


def test_bias_relu_cases_reach_every_path():
    n4 = [rows * C // 4 for rows, C in FWD_ROWMAJOR]
    assert min(n4) == 1 and sum(n > FWD_CAP_ITEMS for n in n4) == 2
    assert all(C % 4 == 0 for _, C in FWD_ROWMAJOR) and {12, 100} <= {C for _, C in FWD_ROWMAJOR}
    n4p = [N * C * HW // 4 for N, C, HW in FWD_PLANAR]
    assert min(n4p) == 1 and max(n4p) > FWD_CAP_ITEMS and sorted(n4p)[-2] <= FWD_CAP_ITEMS
    for C in BWD_C:
        for hw in [0] + BWD_HW:
            mine = [(rows, b) for rows, c, b, h in BWD_MULTI if c == C and h == hw]
            blocks = {b for _, b in mine}
            assert {1, 2, 3, 2048, 8 * 256 // C + 1} <= blocks
            assert any(b == bias_relu_plan(rows, C) for rows, b in mine)
            rpb = lambda rows, b: -(-rows // b)        # noqa: E731
            assert any((b - 1) * rpb(rows, b) >= rows for rows, b in mine)       # idle workgroups
            assert any(rows % rpb(rows, b) for rows, b in mine if b > 1)         # a partial range
            assert any(b * C > 8 * 256 for _, b in mine)                         # a second trip
    assert (5, 64, 8, 0) in BWD_MULTI and any(rows == 1 for rows, _, _, _ in BWD_MULTI)
    assert any(rows % b for rows, _, b, _ in BWD_MULTI)
    assert {hw for _, _, _, hw in BWD_MULTI} == {0, 1, 9, 49}
    assert all(hw == 0 or rows % hw == 0 for rows, _, _, hw in BWD_MULTI)
    assert all(256 % C == 0 and C % 4 == 0 for _, C, _, _ in BWD_MULTI)
    assert SMALL_C == [1, 3, 4, 255, 256, 257, 512, 1000] and SMALL_ROWS == [1, 32, 256, 1024]
    assert REUSE == [(300, 64, 7, 0), (98, 32, 5, 49)]


def test_noisy_cases_reach_both_forms_and_the_cap():
    forms = {(noisy_v4(i, None), o * (i // (4 if noisy_v4(i, None) else 1)) + o > NOISY_CAP_ITEMS)
             for o, i in NOISY_SHAPES}
    assert forms == {(True, False), (True, True), (False, False), (False, True)}
    assert all(noisy_v4(i, None) and not noisy_v4(i, "r") for _, i in NOISY_MISALIGN_SHAPES)
    assert (1, 1) in NOISY_SHAPES and {i % 4 for _, i in NOISY_SHAPES} >= {0, 1, 3}
    # the planted draws: both zeros in both parts of the smallest layers, everything at (51, 512)
    r = noisy_r(np.random.RandomState(0), 1, 1)
    assert np.signbit(r).tolist() == [False, True] and (r == 0).all()
    r = noisy_r(np.random.RandomState(0), 51, 512)
    for part in (r[:512], r[512:]):
        assert set(part.view(np.uint32).tolist()) >= set(NOISY_SPECIALS.view(np.uint32).tolist())
    f = shaped(NOISY_SPECIALS)
    assert f.view(np.uint32).tolist()[:8] == np.array([0.0, -0.0, 1, -1, 2, -2, 0.5, -0.5],
                                                      dtype=f32).view(np.uint32).tolist()
    # sqrt of the smallest subnormal 2^-149 is 2^-74.5, a normal number
    assert f[8] == f32(2.0 ** -74.5) == -f[9]


# ---------------------------------------------------------------------------
# the "exact" bias + ReLU operands
# ---------------------------------------------------------------------------
def _assert_exact(gy, y):
    gx, s, a = ref_bwd(gy, y)
    assert (gx == np.round(gx)).all()
    # every partial sum of a column, in any order, is an integer of magnitude <= sum|g| < 2^24
    assert a.max() < EXACT_LIMIT
    assert set(np.unique(y).tolist()) <= {-1.0, 0.0, 1.0, 2.0}


def test_exact_operands_stay_below_2_to_24():
    rs = np.random.RandomState(0)
    shapes = {(rows, C) for rows, C, _, _ in BWD_MULTI} | {(r, c) for r in SMALL_ROWS for c in SMALL_C}
    for rows, C in sorted(shapes):
        gy, y = exact_operands(rs, rows, C)
        _assert_exact(gy, y)
        assert np.abs(gy).max() <= 3 and 3 * rows < EXACT_LIMIT
        if rows * C >= 4096:
            assert 0.25 < (gy == 0).mean() < 0.6
            assert np.signbit(y[y == 0]).any() and not np.signbit(y[y == 0]).all()
    for rows, C, _, _ in REUSE:
        for gy, y in reuse_operand_sets(rows, C):
            _assert_exact(gy, y)
