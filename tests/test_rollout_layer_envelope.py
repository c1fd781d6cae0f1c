"""csrc/rollout.hip (scan and assembly part), ``pfrl_ppo_minibatch_f32act`` of csrc/ppo_gaussian.hip,
csrc/bias_act.hip and csrc/noisy.hip -- the kernels every PPO, A2C and Rainbow run goes through --
over every path their launchers select and every tail their loops have, through the C ABI
(``_native.lib()``: the wrappers of ``pfrl_amd.ops`` allocate their own outputs and choose ``blocks``,
alignment and workspace themselves), against plain NumPy.  The method of tests/test_gather_envelope.py.

The library is built with ``-ffp-contract=off -fno-fast-math`` (asserted below from
``_native.HIPCC_FLAGS``), so every kernel here except the two sums is a fixed sequence of correctly
rounded IEEE operations and is compared BIT FOR BIT (uint32 view, the sign of zero included) with
that sequence restated in NumPy scalar types.  No reference is taken from another kernel;
tests/test_rollout_layer_envelope_cpu.py pins the restatements to the C oracle without a GPU.

References
* GAE, mode 0      adv = fl32(fl32(fl32(f32(r) + fl32(f32(g_n) nv)) - v) + fl32(f32(g l) adv)),
                   v_teacher = fl32(adv + v); modes 1 / 2: float64 as in ``k_gae_scan`` (mode 1: the
                   product g_n nv is rounded to f32 first); adv = 0 at a cut, before the step;
                   g_n = g or g * 0.0; vectorised over N, a loop over T
* A2C returns      both branches of ``k_a2c_returns`` step by step in f32; g and g tau each rounded
                   once, from the f64 product
* ppo_minibatch    a gather; the advantage fl32(fl32(a - mean) / fl32(std + 1e-8f))
* bias + ReLU      y = max(fl32(x + b), 0) compared as VALUES (fmaxf may return either zero);
                   gx = where(y > 0, gy, 0) bit for bit
* noisy weights    f(r) = +-sqrt32(|r|), r * 0.0 at zero; W = fl32(mu + fl32(sigma fl32(f_o f_i))),
                   b = fl32(mu_b + fl32(sigma_b f_o)), g_sigma_W = fl32(g_W fl32(f_o f_i)),
                   g_sigma_b = fl32(g_b f_o).  ``np.sqrt`` on float32 is correctly rounded; the device's
                   ``sqrtf`` has to agree in every bit (no tolerance)

The two sums
* gb               exact part: gy in -3..3 with a third zero, y in {-1, -0.0, +0.0, 1, 2}: every
                   partial sum is an integer below 2^24 (asserted on the CPU), gb equals the float64
                   column sum.  Rounded part: randn operands, per column
                   |gb - ref64| <= 2 (rows + blocks + 2) 2^-24 sum|g| (the forward-error bound of an
                   f32 sum of rows terms folded over blocks partials in any order, factor 2);
                   ``MAX RATIO`` lines per kernel form after the last test (``pytest -s``).
* adv_stats        mean and sqrt(max(E[x^2] - mean^2, 0)) in float64 with ``np.sum``, rounded to f32;
                   inputs with |mean| <= 100 std; 1 f32 ulp allowed; the CPU file asserts that the
                   reference's own uncertainty stays below a quarter ulp for every case.  A constant
                   column c (<= 8 significant bits, n < 2^24): n c and n c^2 are exact in f64, so are
                   the two quotients, and E[x^2] - mean^2 is exactly 0: the mean must be c, std 0,
                   and the advantages ``pfrl_ppo_minibatch`` standardises with them exactly 0.

Guards: every output (and every workspace) is a slice of a larger buffer with 4 KiB before and after
it, filled -- payload included -- with the NaN 0x7FA5A5A5 (f32) or 0xA5 bytes (integers); the guard
zones must hold the fill after the launch and no payload element may keep it.

The 65 520-byte launch: ``pfrl_gae_scan`` takes ``k_gae_scan_lds`` while T E (9 or 13) <= 65 536 bytes;
the largest rollouts that do ask for 65 520 bytes of dynamic LDS next to ``__launch_bounds__(256)``
(T = 910 / 630 at E = 8, 455 / 315 at E = 16).  They run here, with the first rollout past the limit
(the lane-per-env kernel) next to them; on the MI355X the launch succeeds.  After the LDS launch
``PFRL_LAUNCH_CHECK()`` RETURNS (csrc/common.h: ``return (int)e__`` on an error, ``return 0``
otherwise; the CPU file pins it), so control never falls through to the second launch: a refused LDS
launch would come back as a non-zero code, which these tests would report.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 4096                       # bytes on each side of every output
NAN_BITS = 0x7FA5A5A5              # f32 fill pattern (a NaN)
ERR_ARG = -2                       # PFRL_ERR_ARG, include/pfrl_amd.h
U8, I32, I64, F32, F64 = "u8", "i32", "i64", "f32", "f64"
_NP = {U8: np.uint8, I32: np.int32, I64: np.int64, F32: np.float32, F64: np.float64}
_TORCH = {U8: torch.uint8, I32: torch.int32, I64: torch.int64, F32: torch.float32,
          F64: torch.float64}
f32, f64 = np.float32, np.float64
U24 = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from pfrl_amd import _native

    _native.lib()  # fail loudly if the HIP library is missing
    assert "-ffp-contract=off" in _native.HIPCC_FLAGS and "-fno-fast-math" in _native.HIPCC_FLAGS
    assert not any(f in _native.HIPCC_FLAGS for f in ("-ffast-math", "-Ofast"))
    return torch.device("cuda:0")


def _lib():
    from pfrl_amd import _native

    return _native.lib()


def P(t):
    """Device pointer of a tensor (``None`` -> NULL)."""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def S():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


_RATIO = {}


@pytest.fixture(scope="module", autouse=True)
def _ratio_summary():
    yield
    for name in sorted(_RATIO):
        print("MAX RATIO %s %.4f" % (name, _RATIO[name]))


def _note(name, ratio):
    _RATIO[name] = max(_RATIO.get(name, 0.0), float(ratio))


# ---------------------------------------------------------------------------
# guarded buffers
# ---------------------------------------------------------------------------
def _bits(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.float32:
        return a.view(np.uint32)
    if a.dtype == np.float64:
        return a.view(np.uint64)
    return a


def assert_bits_equal(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype,
                                                                 got.shape, want.shape)
    np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=what)


def fill_pattern(kind, shape):
    """What a guarded buffer of this type holds before a launch, as a NumPy array."""
    if kind == F32:
        return np.full(shape, NAN_BITS, dtype=np.uint32).view(np.float32)
    n = int(np.prod(shape, dtype=np.int64)) * np.dtype(_NP[kind]).itemsize
    return np.full(n, 0xA5, dtype=np.uint8).view(_NP[kind]).reshape(shape)


def holds_fill(kind, a):
    """Boolean array: which elements of ``a`` still are the fill pattern."""
    a = np.ascontiguousarray(a)
    return _bits(a) == _bits(fill_pattern(kind, a.shape))


class Guarded:
    """``shape`` elements of ``kind`` inside a larger device buffer: GUARD bytes of fill pattern on
    both sides, the payload holding the fill pattern too (or ``init``).  The payload starts 16-byte
    aligned plus ``shift`` bytes."""

    def __init__(self, dev, kind, shape, init=None, shift=0):
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        self.kind, self.shape = kind, shape
        self.nbytes = int(np.prod(shape, dtype=np.int64)) * np.dtype(_NP[kind]).itemsize
        total = GUARD + 16 + (self.nbytes + 15) // 16 * 16 + GUARD
        if kind == F32:
            self.buf = torch.full((total // 4,), NAN_BITS, dtype=torch.int32,
                                  device=dev).view(torch.uint8)
        else:
            self.buf = torch.full((total,), 0xA5, dtype=torch.uint8, device=dev)
        self.lo = GUARD + shift
        self.t = self.buf[self.lo:self.lo + self.nbytes].view(_TORCH[kind]).view(shape)
        assert self.t.data_ptr() % 16 == shift and self.t.is_contiguous()
        if init is not None:
            init = np.ascontiguousarray(init, dtype=_NP[kind]).reshape(shape)
            self.t.copy_(torch.from_numpy(init.copy()).to(dev))
        self.pristine = self.buf.cpu().numpy().copy()

    def check(self, want=None, what="", written=True):
        """Guards intact; payload == ``want`` bit for bit (when given); no payload element keeps the
        fill (``written``).  Returns the payload."""
        torch.cuda.synchronize()
        now = self.buf.cpu().numpy()
        end = self.lo + self.nbytes
        np.testing.assert_array_equal(now[:self.lo], self.pristine[:self.lo],
                                      err_msg="%s: write BEFORE the output" % what)
        np.testing.assert_array_equal(now[end:], self.pristine[end:],
                                      err_msg="%s: write PAST the output" % what)
        got = now[self.lo:end].copy().view(_NP[self.kind]).reshape(self.shape)
        if want is not None:
            assert_bits_equal(got, np.asarray(want, dtype=_NP[self.kind]).reshape(self.shape), what)
        elif written:
            assert not holds_fill(self.kind, got).any(), "%s: payload not fully written" % what
        return got

    def untouched(self, what=""):
        torch.cuda.synchronize()
        np.testing.assert_array_equal(self.buf.cpu().numpy(), self.pristine,
                                      err_msg="%s was written" % what)


def _T(dev, a, shift=0, slack=64):
    """``a`` on the device inside a longer allocation (``slack`` elements follow it), based ``shift``
    bytes past a 16-byte boundary.  The tensor stays alive until the test ends (the launches take
    bare pointers, and a freed block would be handed to the next operand)."""
    a = np.ascontiguousarray(a)
    raw = torch.zeros(a.nbytes + 16 + slack * a.itemsize, dtype=torch.uint8, device=dev)
    t = raw[shift:shift + a.nbytes].view(_TORCH_OF[a.dtype.type]).view(a.shape)
    t.copy_(torch.from_numpy(a).to(dev))
    assert t.data_ptr() % 16 == shift
    _KEEP.append(raw)
    return t


_KEEP = []


@pytest.fixture(autouse=True)
def _release_operands():
    yield
    torch.cuda.synchronize()
    del _KEEP[:]


_TORCH_OF = {np.uint8: torch.uint8, np.int32: torch.int32, np.int64: torch.int64,
             np.float32: torch.float32, np.float64: torch.float64}


# ---------------------------------------------------------------------------
# 1. pfrl_gae_scan
# ---------------------------------------------------------------------------
GAE_T = [1, 2, 15, 16, 17, 31, 32, 33, 48]
GAE_N = [1, 7, 8, 9, 17]
GAE_CUTS = ["none", "all", "first", "last", "chunk"]
# (mode, T, N): the LDS limit from both sides (E = 8 at N = 9, E = 16 at N = 4097), the switch to
# E = 16 and its last workgroup with 1 / 15 live envs, the lane-per-env kernel's workgroup edge
GAE_EDGE = ([(0, 910, 9), (0, 911, 9), (1, 630, 9), (1, 631, 9), (2, 630, 9), (2, 631, 9)]
            + [(m, 17, n) for m in (0, 1, 2) for n in (4095, 4096, 4097, 4111)]
            + [(0, 455, 4097), (0, 456, 4097), (1, 315, 4097), (1, 316, 4097)]
            + [(m, 1200, n) for m in (0, 1, 2) for n in (255, 256, 257)])
GAE_HYPER = [(0.99, 0.0), (1.0, 0.95)]          # lambda = 0, gamma = 1 (at T = 33, N = 9)


def gae_cut(kind, T, N):
    cut = np.zeros((T, N), dtype=np.uint8)
    if kind == "all":
        cut[:] = 1
    elif kind == "first":
        cut[0] = 1
    elif kind == "last":
        cut[T - 1] = 1
    elif kind == "chunk":
        # counted from the end: the first (u = 0) and the last (u = 15) step of a register chunk
        u = (T - 1 - np.arange(T)) % 16
        cut[(u == 0) | (u == 15)] = 5           # any non-zero byte is a cut
        cut[:, 1::3] = 0                        # (not in every env)
    return cut


def gae_inputs(rs, T, N, cut_kind):
    """reward f64 (no f32 holds it), v / nv f32, nonterminal 0 in about a fifth, cut."""
    reward = rs.randn(T, N) * np.exp2(rs.randint(-3, 4, size=(T, N)).astype(np.float64))
    reward[::7, ::2] = 1.0 / 3.0
    assert (reward.astype(f32).astype(f64) != reward).all()
    v = rs.randn(T, N).astype(f32)
    nv = rs.randn(T, N).astype(f32)
    nt = (rs.rand(T, N) >= 0.2).astype(np.uint8) * np.uint8(3)     # any non-zero byte
    return reward, v, nv, nt, gae_cut(cut_kind, T, N)


def ref_gae(reward, v, nv, nt, cut, gamma, lambd, mode):
    T, N = reward.shape
    gamma, lambd = f64(gamma), f64(lambd)
    gl, g0 = gamma * lambd, gamma * f64(0.0)
    adv_out, vt_out = np.empty((T, N), dtype=f32), np.empty((T, N), dtype=f32)
    if mode == 0:
        glf = f32(gl)
        adv = np.zeros(N, dtype=f32)
        for t in range(T - 1, -1, -1):
            adv = np.where(cut[t] != 0, f32(0), adv)
            gn = np.where(nt[t] != 0, gamma, g0).astype(f32)
            prod = gn * nv[t]
            s1 = reward[t].astype(f32) + prod
            td = s1 - v[t]
            adv = td + glf * adv
            assert adv.dtype == f32
            adv_out[t], vt_out[t] = adv, adv + v[t]
        return adv_out, vt_out
    adv = np.zeros(N, dtype=f64)
    for t in range(T - 1, -1, -1):
        adv = np.where(cut[t] != 0, f64(0), adv)
        gn = np.where(nt[t] != 0, gamma, g0)
        if mode == 2:
            prod = gn * nv[t].astype(f64)
        else:
            prod = (gn.astype(f32) * nv[t]).astype(f64)
        s1 = reward[t] + prod
        td = s1 - v[t].astype(f64)
        adv = td + gl * adv
        assert adv.dtype == f64
        adv_out[t], vt_out[t] = adv.astype(f32), (adv + v[t].astype(f64)).astype(f32)
    return adv_out, vt_out


def run_gae(dev, rs, mode, T, N, cut_kind, gamma=0.99, lambd=0.95):
    reward, v, nv, nt, cut = gae_inputs(rs, T, N, cut_kind)
    adv, vt = Guarded(dev, F32, (T, N)), Guarded(dev, F32, (T, N))
    rc = _lib().pfrl_gae_scan(T, N, P(_T(dev, reward)), P(_T(dev, v)), P(_T(dev, nv)),
                              P(_T(dev, nt)), P(_T(dev, cut)), gamma, lambd, mode, P(adv.t),
                              P(vt.t), S())
    what = "mode=%d T=%d N=%d cut=%s" % (mode, T, N, cut_kind)
    assert rc == 0, what
    want_adv, want_vt = ref_gae(reward, v, nv, nt, cut, gamma, lambd, mode)
    adv.check(want_adv, what + " adv")
    vt.check(want_vt, what + " v_teacher")


@pytest.mark.parametrize("T", GAE_T)
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_gae_scan_chunks_and_cuts(dev, mode, T):
    rs = np.random.RandomState(100 * mode + T)
    for N in GAE_N:
        for cut_kind in GAE_CUTS:
            run_gae(dev, rs, mode, T, N, cut_kind)


@pytest.mark.parametrize("gamma,lambd", GAE_HYPER)
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_gae_scan_lambda_zero_and_gamma_one(dev, mode, gamma, lambd):
    run_gae(dev, np.random.RandomState(mode), mode, 33, 9, "chunk", gamma, lambd)


@pytest.mark.parametrize("mode,T,N", GAE_EDGE)
def test_gae_scan_route_edges(dev, mode, T, N):
    rs = np.random.RandomState(T + N + mode)
    run_gae(dev, rs, mode, T, N, "chunk")
    if T >= 300 and N < 4096:
        run_gae(dev, rs, mode, T, N, "none")


@pytest.mark.parametrize("T,N", [(0, 5), (5, 0), (0, 0)])
def test_gae_scan_empty_writes_nothing(dev, T, N):
    adv, vt = Guarded(dev, F32, (8,)), Guarded(dev, F32, (8,))
    d = _T(dev, np.zeros(8))
    for mode in (0, 1, 2):
        assert _lib().pfrl_gae_scan(T, N, P(d), P(d), P(d), P(d), P(d), 0.99, 0.95, mode, P(adv.t),
                                    P(vt.t), S()) == 0
    assert _lib().pfrl_gae_scan(4, 2, P(d), P(d), P(d), P(d), P(d), 0.99, 0.95, 3, P(adv.t),
                                P(vt.t), S()) == ERR_ARG
    adv.untouched("adv")
    vt.untouched("v_teacher")


# ---------------------------------------------------------------------------
# 2. pfrl_a2c_returns
# ---------------------------------------------------------------------------
A2C_T, A2C_N = [1, 2, 5, 17], [1, 255, 256, 257]


def a2c_inputs(rs, T, N):
    rewards = rs.randn(T, N).astype(f32)
    masks = (rs.rand(T, N) >= 0.2).astype(f32)
    masks[0, ::2] = 0.0                        # a terminal at t = 0 ...
    masks[T - 1, ::3] = 0.0                    # ... and at t = T - 1
    value_preds = rs.randn(T + 1, N).astype(f32)
    bootstrap = rs.randn(N).astype(f32)
    return rewards, masks, value_preds, bootstrap


def ref_a2c_returns(rewards, masks, value_preds, returns, gamma, tau, use_gae):
    """``returns`` [T + 1, N] as the launch finds it -> as it leaves it."""
    T, N = rewards.shape
    out = returns.copy()
    g = f32(f64(gamma))
    if use_gae:
        gt = f32(f64(gamma) * f64(tau))
        gae = np.zeros(N, dtype=f32)
        for t in range(T - 1, -1, -1):
            a = g * value_preds[t + 1]
            b = a * masks[t]
            c = rewards[t] + b
            delta = c - value_preds[t]
            g3 = (gt * masks[t]) * gae
            gae = delta + g3
            assert gae.dtype == f32
            out[t] = gae + value_preds[t]
        return out
    nxt = out[T].copy()
    for t in range(T - 1, -1, -1):
        nxt = rewards[t] + (g * nxt) * masks[t]
        assert nxt.dtype == f32
        out[t] = nxt
    return out


@pytest.mark.parametrize("use_gae", [0, 1])
@pytest.mark.parametrize("T", A2C_T)
def test_a2c_returns(dev, T, use_gae):
    rs = np.random.RandomState(10 * T + use_gae)
    for N in A2C_N:
        rewards, masks, value_preds, bootstrap = a2c_inputs(rs, T, N)
        init = fill_pattern(F32, (T + 1, N)).copy()
        if not use_gae:
            init[T] = bootstrap                # preset, must be unchanged
        ret = Guarded(dev, F32, (T + 1, N), init=init)
        rc = _lib().pfrl_a2c_returns(T, N, P(_T(dev, rewards)), P(_T(dev, masks)),
                                     P(_T(dev, value_preds)), P(ret.t), 0.99, 0.95, use_gae, S())
        assert rc == 0
        want = ref_a2c_returns(rewards, masks, value_preds, init, 0.99, 0.95, use_gae)
        got = ret.check(want, "T=%d N=%d use_gae=%d" % (T, N, use_gae))
        assert not holds_fill(F32, got[:T]).any()


def test_a2c_returns_empty_writes_nothing(dev):
    ret = Guarded(dev, F32, (8,))
    d = _T(dev, np.zeros(8, dtype=f32))
    for T, N in [(0, 4), (4, 0)]:
        for use_gae in (0, 1):
            assert _lib().pfrl_a2c_returns(T, N, P(d), P(d), P(d), P(ret.t), 0.99, 0.95, use_gae,
                                           S()) == 0
    ret.untouched("returns")


# ---------------------------------------------------------------------------
# 3. pfrl_adv_stats
# ---------------------------------------------------------------------------
ADV_BLOCK, ADV_CAP = 2048, 1024               # elements per workgroup, workgroups at most
ADV_N = [1, 2, 63, 64, 65, 2047, 2048, 2049, 1024 * 2048 - 1, 1024 * 2048, 1024 * 2048 + 1,
         3 * 2 ** 20 + 5]
ADV_CONST_N, ADV_CONST_C = 2049, 207.0 / 128.0          # 8 significant bits


def adv_blocks(n):
    return min(ADV_CAP, -(-n // ADV_BLOCK))


def adv_input(n):
    """mean 0.75, std 1.5 (|mean| <= 100 std)."""
    rs = np.random.RandomState(n % 100003)
    return (rs.randn(n) * 1.5 + 0.75).astype(f32)


def ref_adv_stats(x):
    """(mean, std) in float64 with ``np.sum``; the caller rounds to f32."""
    x = x.astype(f64)
    n = f64(x.size)
    mean = np.sum(x) / n
    var = np.sum(x * x) / n - mean * mean
    return mean, np.sqrt(max(var, 0.0))


def run_adv_stats(dev, x):
    out = Guarded(dev, F32, (2,))
    ws = Guarded(dev, F64, (2 * ADV_CAP,))
    assert _lib().pfrl_adv_stats(P(_T(dev, x)), x.size, P(out.t), P(ws.t), S()) == 0
    got = out.check(None, "mean_std")
    # the partial rows the launch wrote: exactly the planned workgroups', the rest still fill
    part = ws.check(None, "partials", written=False).reshape(ADV_CAP, 2)
    kept = holds_fill(F64, part)
    blocks = adv_blocks(x.size)
    assert not kept[:blocks].any() and kept[blocks:].all(), \
        "n=%d: %d partial rows written, %d planned" % (x.size, int((~kept[:, 0]).sum()), blocks)
    return got, out


@pytest.mark.parametrize("n", ADV_N)
def test_adv_stats(dev, n):
    x = adv_input(n)
    got, _ = run_adv_stats(dev, x)
    for name, g, r in zip(("mean", "std"), got, ref_adv_stats(x)):
        r32 = f32(r)
        ulp = f64(np.spacing(np.abs(r32)))
        assert abs(f64(g) - f64(r32)) <= ulp, (name, n, g, r32)
        _note("adv_stats %s (ulp)" % name, abs(f64(g) - f64(r32)) / ulp)


def test_adv_stats_constant_column_and_the_minibatch_standardised_with_it(dev):
    n, c = ADV_CONST_N, f32(ADV_CONST_C)
    x = np.full(n, c, dtype=f32)
    got, ms = run_adv_stats(dev, x)
    assert got[0] == c, "mean of a constant column"
    assert np.isfinite(got[1]) and got[1] >= 0
    M = 257
    idx = np.random.RandomState(0).randint(0, n, size=M).astype(np.int64)
    outs = {k: Guarded(dev, F32, (M,)) for k in ("adv", "lp", "v", "vt")}
    act, refs = Guarded(dev, I64, (M,)), Guarded(dev, I32, (M, 1))
    col = _T(dev, x)
    assert _lib().pfrl_ppo_minibatch(M, P(_T(dev, idx)), P(col), P(ms.t), 1, P(col), P(col), P(col),
                                     P(_T(dev, np.zeros(n, dtype=np.int64))),
                                     P(_T(dev, np.zeros((n, 1), dtype=np.int32))), 1,
                                     P(outs["adv"].t), P(outs["lp"].t), P(outs["v"].t),
                                     P(outs["vt"].t), P(act.t), P(refs.t), S()) == 0
    a = outs["adv"].check(None, "adv")
    assert (a == 0).all(), "standardised advantages of a constant column"


def test_adv_stats_rejects(dev):
    out, ws = Guarded(dev, F32, (2,)), Guarded(dev, F64, (2 * ADV_CAP,))
    d = _T(dev, np.zeros(8, dtype=f32))
    assert _lib().pfrl_adv_stats(P(d), 0, P(out.t), P(ws.t), S()) == ERR_ARG
    assert _lib().pfrl_adv_stats(P(d), 8, P(out.t), None, S()) == ERR_ARG
    out.untouched("mean_std")
    ws.untouched("partials")


# ---------------------------------------------------------------------------
# 4. pfrl_ppo_minibatch / pfrl_ppo_minibatch_f32act
# ---------------------------------------------------------------------------
MB_M = [1, 255, 256, 257]
MB_CASES = ([(M, k, None) for M in MB_M for k in (1, 4)]
            + [(M, k, A) for M in MB_M for k in (0, 1, 4) for A in (1, 3, 6)])
MB_EXTRA = 37                                  # the source columns are this much longer than M


def mb_inputs(rs, M, k, A):
    D = M + MB_EXTRA
    idx = rs.randint(0, D, size=M).astype(np.int64)
    idx[-1] = D - 1
    if M >= 2:
        idx[0] = 0
    if M >= 4:
        idx[2] = idx[1]
    assert M == 1 or (idx != np.arange(M)).any()
    col = lambda: rs.randn(D).astype(f32)      # noqa: E731
    if A is None:
        action = rs.randint(0, 1 << 62, size=D, dtype=np.int64) | (np.int64(1) << 31)
        action[1::5] *= -1
    else:
        action = rs.randn(D, A).astype(f32)
    refs = rs.randint(0, 1 << 31, size=(D, k), dtype=np.int64).astype(np.int32)
    mean_std = np.array([0.3, 1.7], dtype=f32)
    return idx, col(), mean_std, col(), col(), col(), action, refs


def ref_mb_adv(adv, idx, mean_std, standardize):
    a = adv[idx]
    if standardize:
        den = mean_std[1] + f32(1e-8)
        a = (a - mean_std[0]) / den
    assert a.dtype == f32
    return a


def launch_mb(dev, M, idx, adv, mean_std, standardize, lp, v, vt, action, refs, k, A, outs):
    L = _lib()
    if A is None:
        return L.pfrl_ppo_minibatch(M, P(idx), P(adv), P(mean_std), standardize, P(lp), P(v), P(vt),
                                    P(action), P(refs), k, P(outs["adv"].t), P(outs["lp"].t),
                                    P(outs["v"].t), P(outs["vt"].t), P(outs["action"].t),
                                    P(outs["refs"].t), S())
    return L.pfrl_ppo_minibatch_f32act(M, P(idx), P(adv), P(mean_std), standardize, P(lp), P(v),
                                       P(vt), P(action), A, P(refs), k, P(outs["adv"].t),
                                       P(outs["lp"].t), P(outs["v"].t), P(outs["vt"].t),
                                       P(outs["action"].t), P(outs["refs"].t), S())


def mb_outputs(dev, M, k, A):
    outs = {key: Guarded(dev, F32, (M,)) for key in ("adv", "lp", "v", "vt")}
    outs["action"] = Guarded(dev, I64, (M,)) if A is None else Guarded(dev, F32, (M, A))
    outs["refs"] = Guarded(dev, I32, (M, k))
    return outs


@pytest.mark.parametrize("standardize", [0, 1])
@pytest.mark.parametrize("M,k,A", MB_CASES)
def test_ppo_minibatch(dev, M, k, A, standardize):
    rs = np.random.RandomState(M * 100 + k * 10 + (A or 0))
    idx, adv, mean_std, lp, v, vt, action, refs = mb_inputs(rs, M, k, A)
    outs = mb_outputs(dev, M, k, A)
    d = [_T(dev, a) for a in (idx, adv, mean_std, lp, v, vt, action, refs)]
    rc = launch_mb(dev, M, d[0], d[1], d[2], standardize, d[3], d[4], d[5], d[6], d[7], k, A, outs)
    what = "M=%d k=%d A=%s std=%d" % (M, k, A, standardize)
    assert rc == 0, what
    outs["adv"].check(ref_mb_adv(adv, idx, mean_std, standardize), what + " adv")
    outs["lp"].check(lp[idx], what + " log_prob")
    outs["v"].check(v[idx], what + " v_pred")
    outs["vt"].check(vt[idx], what + " v_teacher")
    outs["action"].check(action[idx], what + " action")
    outs["refs"].check(refs[idx], what + " refs")
    if A is None:
        assert (np.abs(action[idx]) > 1 << 31).all()


@pytest.mark.parametrize("A", [None, 3])
def test_ppo_minibatch_empty_writes_nothing(dev, A):
    rs = np.random.RandomState(1)
    idx, adv, mean_std, lp, v, vt, action, refs = mb_inputs(rs, 4, 1, A)
    outs = mb_outputs(dev, 4, 1, A)
    d = [_T(dev, a) for a in (idx, adv, mean_std, lp, v, vt, action, refs)]
    assert launch_mb(dev, 0, d[0], d[1], d[2], 1, d[3], d[4], d[5], d[6], d[7], 1, A, outs) == 0
    for key, g in outs.items():
        g.untouched(key)


# ---------------------------------------------------------------------------
# 5. pfrl_bias_relu_fwd
# ---------------------------------------------------------------------------
FWD_CAP_ITEMS = 2048 * 256                     # float4s one trip of the capped grid covers
FWD_ROWMAJOR = ([(rows, C) for C in (4, 8, 32, 64, 256, 12, 100) for rows in (1, 5, 257)]
                + [(8193, 256), (131073, 16)])
FWD_PLANAR = [(1, 4, 1), (3, 32, 9), (5, 64, 49), (2, 12, 35), (33, 64, 1024)]     # (N, C, HW)


def fwd_inputs(rs, rows, C):
    x = rs.randn(rows, C).astype(f32)
    b = rs.randn(C).astype(f32)
    x[::3, ::2] = -b[::2]                      # sums of exactly zero
    x[1::5, 1::4] = -0.0
    return x, b


def ref_bias_relu(x, b):
    s = x + b
    assert s.dtype == f32
    return np.maximum(s, f32(0))


def check_values(g, want, what):
    got = g.check(None, what)
    assert not np.isnan(got).any()
    np.testing.assert_array_equal(got, want, err_msg=what)       # +0.0 == -0.0


@pytest.mark.parametrize("rows,C", FWD_ROWMAJOR)
def test_bias_relu_fwd_rowmajor(dev, rows, C):
    x, b = fwd_inputs(np.random.RandomState(rows + C), rows, C)
    y = Guarded(dev, F32, (rows, C))
    assert _lib().pfrl_bias_relu_fwd(P(_T(dev, x)), P(_T(dev, b)), P(y.t), rows, C, 0, S()) == 0
    check_values(y, ref_bias_relu(x, b), "rows=%d C=%d" % (rows, C))


@pytest.mark.parametrize("N,C,HW", FWD_PLANAR)
def test_bias_relu_fwd_planar(dev, N, C, HW):
    """x channels-last rows [N HW][C] -> y [N][C][HW]."""
    x, b = fwd_inputs(np.random.RandomState(N + C + HW), N * HW, C)
    y = Guarded(dev, F32, (N, C, HW))
    assert _lib().pfrl_bias_relu_fwd(P(_T(dev, x)), P(_T(dev, b)), P(y.t), N * HW, C, HW, S()) == 0
    want = ref_bias_relu(x, b).reshape(N, HW, C).transpose(0, 2, 1)
    check_values(y, np.ascontiguousarray(want), "N=%d C=%d HW=%d" % (N, C, HW))


@pytest.mark.parametrize("rows,C,hw", [(10, 4, 3), (7, 8, 49), (10, 4, -1), (4, 6, 0), (4, 0, 0)])
def test_bias_relu_fwd_rejects(dev, rows, C, hw):
    x, b = fwd_inputs(np.random.RandomState(0), rows, max(C, 4))
    y = Guarded(dev, F32, (rows, max(C, 4)))
    assert _lib().pfrl_bias_relu_fwd(P(_T(dev, x)), P(_T(dev, b)), P(y.t), rows, C, hw,
                                     S()) == ERR_ARG
    y.untouched("y")


# ---------------------------------------------------------------------------
# 6. pfrl_bias_relu_bwd
# ---------------------------------------------------------------------------
BWD_C = [4, 32, 64, 256]
BWD_ROWS = 1000                                # 1000 % 3 == 1; 2048 workgroups: 1048 own no rows
BWD_PLANAR_N, BWD_HW = 21, [1, 9, 49]
SMALL_C, SMALL_ROWS = [1, 3, 4, 255, 256, 257, 512, 1000], [1, 32, 256, 1024]
REUSE = [(300, 64, 7, 0), (2 * 49, 32, 5, 49)]            # (rows, C, blocks, hw)
EXACT_LIMIT = 2.0 ** 24


def bias_relu_plan(rows, C):
    from pfrl_amd import ops

    return ops._bias_relu_plan(rows, C)


def bwd_blocks(rows, C):
    return sorted({1, 2, 3, bias_relu_plan(rows, C), 8 * 256 // C + 1, 2048})


def bwd_multi_cases():
    """(rows, C, blocks, hw) of the multi-workgroup form."""
    cases = [(BWD_ROWS, C, b, 0) for C in BWD_C for b in bwd_blocks(BWD_ROWS, C)]
    for C in BWD_C:
        for hw in BWD_HW:
            rows = BWD_PLANAR_N * hw
            cases += [(rows, C, b, hw) for b in bwd_blocks(rows, C)]
    cases += [(5, 64, 8, 0), (1, 32, 1, 0), (1, 4, 3, 0), (1, 256, 2, 1), (98, 64, 8, 49)]
    return cases


BWD_MULTI = bwd_multi_cases()


def exact_operands(rs, rows, C, shift=0):
    """gy integers -3..3 with a third zero, y in {-1, -0.0, +0.0, 1, 2}.  ``shift``: row 0 passes
    (y = 1) and carries 4096 shift more, which moves every column sum by more than the other rows
    can (|sum| <= 3 rows < 2048 for rows < 683)."""
    gy = rs.randint(-3, 4, size=(rows, C)).astype(f32)
    gy[rs.rand(rows, C) < 1.0 / 3.0] = 0.0
    y = rs.choice(np.array([-1.0, -0.0, 0.0, 1.0, 2.0], dtype=f32), size=(rows, C))
    if shift:
        assert 3 * rows < 2048
        y[0] = 1.0
        gy[0] += f32(4096.0 * shift)
    return gy, y


def randn_operands(rs, rows, C):
    return rs.randn(rows, C).astype(f32), rs.randn(rows, C).astype(f32)


def ref_bwd(gy, y):
    """gx (f32, bit for bit), the float64 column sum and the column sum of |gx|."""
    gx = np.where(y > 0, gy, f32(0))
    assert gx.dtype == f32
    g64 = gx.astype(f64)
    return gx, g64.sum(axis=0), np.abs(g64).sum(axis=0)


def to_layout(a, hw):
    """Row-major [rows][C] operand -> what the kernel reads: the same, or planar [N][C][HW]."""
    if not hw:
        return a
    rows, C = a.shape
    return np.ascontiguousarray(a.reshape(rows // hw, hw, C).transpose(0, 2, 1))


class Workspace:
    """``blocks * C`` zeroed granules + 2 zeroed counters, each between guards, for ONE (C, blocks)."""

    def __init__(self, dev, C, blocks):
        self.C, self.blocks = C, blocks
        self.granules = Guarded(dev, I64, (blocks * C,), init=np.zeros(blocks * C, dtype=np.int64))
        self.counters = Guarded(dev, I64, (2,), init=np.zeros(2, dtype=np.int64))

    def check(self, launches, what):
        """Both counters read launches * blocks; every granule carries the last launch's epoch."""
        ctr = self.counters.check(None, what + " counters", written=False)
        assert ctr.tolist() == [launches * self.blocks] * 2, (what, ctr)
        gr = self.granules.check(None, what + " granules", written=False)
        np.testing.assert_array_equal(gr >> 32, launches, err_msg=what + ": granule epochs")


def launch_bwd(dev, d_gy, d_y, gx, gb, ws, rows, C, blocks, hw):
    return _lib().pfrl_bias_relu_bwd(P(d_gy), P(d_y), P(gx.t), P(gb.t),
                                     P(ws.granules.t) if ws else None,
                                     P(ws.counters.t) if ws else None, rows, C, blocks, hw, S())


def check_bwd(name, gx, gb, gy, y, rows, blocks, exact, what):
    want_gx, sum64, abs64 = ref_bwd(gy, y)
    gx.check(want_gx, what + " gx")
    got = gb.check(None, what + " gb").astype(f64)
    if exact:
        assert abs64.max() < EXACT_LIMIT
        np.testing.assert_array_equal(got, sum64, err_msg=what + " gb (exact)")
        return
    bound = 2.0 * (rows + blocks + 2) * U24 * abs64
    err = np.abs(got - sum64)
    assert (err <= bound).all(), (what, float((err / np.maximum(bound, 1e-300)).max()))
    if (bound > 0).any():
        _note(name, (err[bound > 0] / bound[bound > 0]).max())


def run_bwd(dev, rs, rows, C, blocks, hw, exact, name):
    gy, y = exact_operands(rs, rows, C) if exact else randn_operands(rs, rows, C)
    gx, gb = Guarded(dev, F32, (rows, C)), Guarded(dev, F32, (C,))
    ws = Workspace(dev, C, blocks) if blocks else None
    what = "%s rows=%d C=%d blocks=%d hw=%d %s" % (name, rows, C, blocks, hw,
                                                   "exact" if exact else "randn")
    rc = launch_bwd(dev, _T(dev, to_layout(gy, hw)), _T(dev, to_layout(y, hw)), gx, gb, ws, rows, C,
                    blocks, hw)
    assert rc == 0, what
    check_bwd(name, gx, gb, gy, y, rows, max(blocks, 1), exact, what)
    if ws:
        ws.check(1, what)


@pytest.mark.parametrize("C", BWD_C)
@pytest.mark.parametrize("hw", [0] + BWD_HW)
def test_bias_relu_bwd_multi(dev, C, hw):
    rs = np.random.RandomState(C + hw)
    mine = [c for c in BWD_MULTI if c[1] == C and c[3] == hw]
    assert mine
    for rows, _, blocks, _ in mine:
        for exact in (True, False):
            run_bwd(dev, rs, rows, C, blocks, hw, exact,
                    "bias_relu_bwd planar" if hw else "bias_relu_bwd row-major")


@pytest.mark.parametrize("C", SMALL_C)
def test_bias_relu_bwd_small(dev, C):
    rs = np.random.RandomState(C)
    for rows in SMALL_ROWS:
        for exact in (True, False):
            run_bwd(dev, rs, rows, C, 0, 0, exact, "bias_relu_bwd small")


@pytest.mark.parametrize("rows,C,blocks,hw", [
    (16, 12, 2, 0), (16, 48, 2, 0), (16, 512, 2, 0), (16, 64, -1, 0), (10, 64, 2, 3),
    (16, 64, 2, -1), (1025, 64, 0, 0), (49, 64, 0, 49), (16, 0, 0, 0)])
def test_bias_relu_bwd_rejects(dev, rows, C, blocks, hw):
    rs = np.random.RandomState(0)
    Cb = max(C, 4)
    gy, y = randn_operands(rs, rows, Cb)
    gx, gb = Guarded(dev, F32, (rows, Cb)), Guarded(dev, F32, (Cb,))
    ws = Workspace(dev, Cb, max(blocks, 2))
    assert launch_bwd(dev, _T(dev, gy), _T(dev, y), gx, gb, ws, rows, C, blocks, hw) == ERR_ARG
    for g, what in ((gx, "gx"), (gb, "gb"), (ws.granules, "granules"), (ws.counters, "counters")):
        g.untouched(what)


def reuse_operand_sets(rows, C):
    """Four exact operand sets whose column sums differ pairwise in every column."""
    rs = np.random.RandomState(rows + C)
    sets = [exact_operands(rs, rows, C, shift=j + 1) for j in range(4)]
    sums = [ref_bwd(gy, y)[1] for gy, y in sets]
    assert all((sums[i] != sums[j]).all() for i in range(4) for j in range(i))
    return sets


@pytest.mark.parametrize("rows,C,blocks,hw", REUSE)
def test_bias_relu_bwd_one_workspace_launched_again_and_again(dev, rows, C, blocks, hw):
    """Four launches with four operand sets on ONE workspace, one stream: the epoch protocol must
    not accept a granule of an earlier launch."""
    sets = reuse_operand_sets(rows, C)
    ws = Workspace(dev, C, blocks)
    for j, (gy, y) in enumerate(sets):
        gx, gb = Guarded(dev, F32, (rows, C)), Guarded(dev, F32, (C,))
        what = "launch %d" % j
        assert launch_bwd(dev, _T(dev, to_layout(gy, hw)), _T(dev, to_layout(y, hw)), gx, gb, ws,
                          rows, C, blocks, hw) == 0
        check_bwd("reuse", gx, gb, gy, y, rows, blocks, True, what)
        ws.check(j + 1, what)


@pytest.mark.parametrize("rows,C,blocks,hw", REUSE)
def test_bias_relu_bwd_one_workspace_replayed_from_a_graph(dev, rows, C, blocks, hw):
    """The same with the launch captured once (after one eager launch on the capture stream) and
    replayed three times, the operands rewritten in place between the replays."""
    sets = reuse_operand_sets(rows, C)
    ws = Workspace(dev, C, blocks)
    gx, gb = Guarded(dev, F32, (rows, C)), Guarded(dev, F32, (C,))
    d_gy, d_y = _T(dev, to_layout(sets[0][0], hw)), _T(dev, to_layout(sets[0][1], hw))
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        assert launch_bwd(dev, d_gy, d_y, gx, gb, ws, rows, C, blocks, hw) == 0
    stream.synchronize()
    check_bwd("reuse", gx, gb, sets[0][0], sets[0][1], rows, blocks, True, "eager launch")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        rc = launch_bwd(dev, d_gy, d_y, gx, gb, ws, rows, C, blocks, hw)
    assert rc == 0
    ws.check(1, "after the capture")             # a capture launches nothing
    for j in (1, 2, 3):
        gy, y = sets[j]
        d_gy.copy_(torch.from_numpy(to_layout(gy, hw)).to(dev))
        d_y.copy_(torch.from_numpy(to_layout(y, hw)).to(dev))
        gb.t.copy_(torch.from_numpy(fill_pattern(F32, (C,)).copy()).to(dev))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        check_bwd("reuse", gx, gb, gy, y, rows, blocks, True, "replay %d" % j)
        ws.check(j + 1, "replay %d" % j)


# ---------------------------------------------------------------------------
# 7. pfrl_noisy_weights_fwd / _bwd
# ---------------------------------------------------------------------------
NOISY_CAP_ITEMS = 4096 * 256
NOISY_SHAPES = [(1, 1), (3, 5), (7, 4), (51, 512), (5, 1023), (16, 1024), (1025, 4096), (1024, 1025)]
NOISY_MISALIGN_SHAPES = [(7, 4), (51, 512)]
NOISY_FWD_PTRS, NOISY_BWD_PTRS = ["mu_w", "sigma_w", "r", "w_out"], ["g_w", "r", "g_sigma_w"]
SUBNORMAL = np.array([1], dtype=np.uint32).view(f32)[0]
NOISY_SPECIALS = np.array([0.0, -0.0, 1.0, -1.0, 4.0, -4.0, 0.25, -0.25, SUBNORMAL, -SUBNORMAL],
                          dtype=f32)


def noisy_r(rs, out_f, in_f):
    """in + out draws, eps_x first; the specials planted in both parts (as far as they fit)."""
    r = rs.randn(in_f + out_f).astype(f32)
    for lo, n, rot in ((0, in_f, 0), (in_f, out_f, 1)):
        pos = np.arange(0, n, 3)[:len(NOISY_SPECIALS)]
        r[lo + pos] = np.roll(NOISY_SPECIALS, -rot)[:len(pos)]
    return r


def shaped(r):
    s = np.sqrt(np.abs(r))
    assert s.dtype == f32
    return np.where(r > 0, s, np.where(r < 0, -s, r * f32(0.0)))


def ref_noisy_fwd(mu_w, sigma_w, mu_b, sigma_b, r):
    out_f, in_f = mu_w.shape
    fi, fo = shaped(r[:in_f]), shaped(r[in_f:])
    w = mu_w + sigma_w * (fo[:, None] * fi[None, :])
    b = mu_b + sigma_b * fo
    assert w.dtype == f32 and b.dtype == f32
    return w, b


def ref_noisy_bwd(g_w, g_b, r):
    out_f, in_f = g_w.shape
    fi, fo = shaped(r[:in_f]), shaped(r[in_f:])
    gsw = g_w * (fo[:, None] * fi[None, :])
    gsb = g_b * fo
    assert gsw.dtype == f32 and gsb.dtype == f32
    return gsw, gsb


def noisy_v4(in_f, shifted):
    """The launcher's rule for the float4 kernel."""
    return in_f % 4 == 0 and shifted is None


def run_noisy(dev, out_f, in_f, bias, shifted=None, direction="fwd"):
    rs = np.random.RandomState(out_f * 7 + in_f)
    r = noisy_r(rs, out_f, in_f)
    sh = lambda name: 4 if shifted == name else 0          # noqa: E731
    what = "%s out=%d in=%d bias=%s shifted=%s" % (direction, out_f, in_f, bias, shifted)
    if direction == "fwd":
        mu_w, sigma_w = (rs.randn(out_f, in_f).astype(f32) for _ in range(2))
        mu_b, sigma_b = (rs.randn(out_f).astype(f32) for _ in range(2))
        w = Guarded(dev, F32, (out_f, in_f), shift=sh("w_out"))
        b = Guarded(dev, F32, (out_f,))
        rc = _lib().pfrl_noisy_weights_fwd(
            P(_T(dev, mu_w, sh("mu_w"))), P(_T(dev, sigma_w, sh("sigma_w"))),
            P(_T(dev, mu_b)) if bias else None, P(_T(dev, sigma_b)) if bias else None,
            P(_T(dev, r, sh("r"))), P(w.t), P(b.t) if bias else None, out_f, in_f, S())
        want_w, want_b = ref_noisy_fwd(mu_w, sigma_w, mu_b, sigma_b, r)
    else:
        g_w, g_b = rs.randn(out_f, in_f).astype(f32), rs.randn(out_f).astype(f32)
        w = Guarded(dev, F32, (out_f, in_f), shift=sh("g_sigma_w"))
        b = Guarded(dev, F32, (out_f,))
        rc = _lib().pfrl_noisy_weights_bwd(
            P(_T(dev, g_w, sh("g_w"))), P(_T(dev, g_b)) if bias else None, P(_T(dev, r, sh("r"))),
            P(w.t), P(b.t) if bias else None, out_f, in_f, S())
        want_w, want_b = ref_noisy_bwd(g_w, g_b, r)
    assert rc == 0, what
    w.check(want_w, what + " weights")
    if bias:
        b.check(want_b, what + " bias")
    else:
        b.untouched(what + " bias")


@pytest.mark.parametrize("direction", ["fwd", "bwd"])
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("out_f,in_f", NOISY_SHAPES)
def test_noisy_weights(dev, out_f, in_f, bias, direction):
    run_noisy(dev, out_f, in_f, bias, None, direction)


@pytest.mark.parametrize("direction,shifted", [("fwd", p) for p in NOISY_FWD_PTRS]
                         + [("bwd", p) for p in NOISY_BWD_PTRS])
@pytest.mark.parametrize("out_f,in_f", NOISY_MISALIGN_SHAPES)
def test_noisy_weights_one_pointer_off_the_16_byte_boundary(dev, out_f, in_f, direction, shifted):
    run_noisy(dev, out_f, in_f, True, shifted, direction)


def test_noisy_weights_rejects(dev):
    L = _lib()
    d = _T(dev, np.ones(64, dtype=f32))
    w, b = Guarded(dev, F32, (4, 4)), Guarded(dev, F32, (4,))
    assert L.pfrl_noisy_weights_fwd(P(d), P(d), None, P(d), P(d), P(w.t), P(b.t), 4, 4,
                                    S()) == ERR_ARG
    assert L.pfrl_noisy_weights_fwd(P(d), P(d), P(d), None, P(d), P(w.t), P(b.t), 4, 4,
                                    S()) == ERR_ARG
    assert L.pfrl_noisy_weights_bwd(P(d), None, P(d), P(w.t), P(b.t), 4, 4, S()) == ERR_ARG
    for out_f, in_f in [(0, 4), (4, 0)]:
        assert L.pfrl_noisy_weights_fwd(P(d), P(d), P(d), P(d), P(d), P(w.t), P(b.t), out_f, in_f,
                                        S()) == ERR_ARG
        assert L.pfrl_noisy_weights_bwd(P(d), P(d), P(d), P(w.t), P(b.t), out_f, in_f,
                                        S()) == ERR_ARG
    w.untouched("weights")
    b.untouched("bias")
