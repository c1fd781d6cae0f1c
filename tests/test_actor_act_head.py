"""pfrl_squashed_head_act and pfrl_deterministic_head_act (csrc/actor_act.hip) called directly, every
output between guard zones.

Shapes: K in {1, 63, 64, 65, 256, 300, 1024} (one lane-trip, its tail on either side, the example
widths, the gate), A in {1, 2, 3, 17, 32}, M in {1, 2, 63, 64, 65, 257}; every (K, M) pair with A
rotated through its values, so that every pair of values of two parameters occurs (42 shapes).

What is exact (==, a NaN standing for a NaN): the SAC action against pfrl_squashed_head_fwd on the
kernel's own x_out and the same eps (the shared __device__ function), both scale formulas; the
mode against that function on eps = 0; the bounded greedy action against torch.tanh(y) * scale +
shift on the device; the explored action against np.clip(greedy + noise, low, high) in NumPy
float32; a row of a 65-row launch against the 1-row launch on that row; a captured graph's replays
against direct launches.  What is measured: the layer against the float64 product, next to torch's
float32 ``F.linear`` on the CPU on the same operands -- another legitimate summation order; the
kernels may err twice as much (the margin of tests/test_boltzmann_head.py, for the same reason).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pfrl_amd import _native

pytestmark = pytest.mark.gpu

GUARD = 4096
PFRL_ERR_ARG = -2
K_LIST, A_LIST, M_LIST = (1, 63, 64, 65, 256, 300, 1024), (1, 2, 3, 17, 32), (1, 2, 63, 64, 65, 257)
SHAPES = [(K, A_LIST[(i + j) % len(A_LIST)], M) for i, K in enumerate(K_LIST) for j, M in enumerate(M_LIST)]
CLAMP = (-20.0, 2.0)


def _dev():
    return torch.device("cuda:0")


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class _Guarded:
    """n float32 between two guard zones of NaN, the payload NaN too until it is written."""

    def __init__(self, n):
        self.n = n
        self.full = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32, device=_dev())
        self.t = self.full[GUARD:GUARD + n]

    def done(self, what, nan_ok=False):
        assert bool(torch.isnan(self.full[:GUARD]).all()), "guard zone before %s was written" % what
        assert bool(torch.isnan(self.full[GUARD + self.n:]).all()), "guard zone after %s was written" % what
        if not nan_ok:
            assert not bool(torch.isnan(self.t).any()), "%s: payload not fully written" % what
        return self.t.cpu().numpy()

    def untouched(self, what):
        assert bool(torch.isnan(self.full).all()), "%s was written" % what


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


def _same(tag, a, b):
    """Bit-identical, except that any NaN stands for any NaN."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    assert a.shape == b.shape and np.array_equal(na, nb), tag
    bad = np.flatnonzero(_bits(a).reshape(-1)[~na.reshape(-1)] != _bits(b).reshape(-1)[~nb.reshape(-1)])
    assert bad.size == 0, "%s: %d of %d elements differ, first %r vs %r" % (
        tag, bad.size, a.size, a.reshape(-1)[~na.reshape(-1)][bad[:1]], b.reshape(-1)[~nb.reshape(-1)][bad[:1]])


def _operands(K, n_out, M, seed):
    """Operands of the size the networks produce: unit-variance h, Xavier-size w, a small bias."""
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(M, K, generator=g)
    w = torch.randn(n_out, K, generator=g) * (2.0 / (K + n_out)) ** 0.5
    b = 0.1 * torch.randn(n_out, generator=g)
    return h, w, b


def _squashed(h, w, b, mode, eps, A, want_x=True, clamp=CLAMP):
    M, K = h.shape
    o = {"x": _Guarded(M * 2 * A) if want_x else None, "action": _Guarded(M * A)}
    rc = _native.lib().pfrl_squashed_head_act(_p(h), _p(w), _p(b), clamp[0], clamp[1], mode, _p(eps),
                                              _p(o["x"].t if want_x else None), _p(o["action"].t), M, K, A,
                                              _stream())
    assert rc == 0
    return o


def _head_fwd(x, mode, eps, A, clamp=CLAMP):
    """pfrl_squashed_head_fwd's action on x [M, 2A]."""
    M = x.shape[0]
    action, logp = _Guarded(M * A), _Guarded(M)
    assert _native.lib().pfrl_squashed_head_fwd(_p(x), 2 * A, clamp[0], clamp[1], mode, _p(eps), _p(action.t),
                                                _p(logp.t), None, M, A, _stream()) == 0
    return action.done("head_fwd action", nan_ok=True).reshape(M, A)


def _deterministic(h, w, b, bound, noise, low, high, want=("y", "greedy")):
    M, K = h.shape
    A = w.shape[0]
    o = {"y": _Guarded(M * A) if "y" in want else None, "greedy": _Guarded(M * A) if "greedy" in want else None,
         "action": _Guarded(M * A)}
    rc = _native.lib().pfrl_deterministic_head_act(
        _p(h), _p(w), _p(b), _p(bound[0]) if bound else None, _p(bound[1]) if bound else None, _p(noise),
        _p(low), _p(high), _p(o["y"].t) if o["y"] else None, _p(o["greedy"].t) if o["greedy"] else None,
        _p(o["action"].t), M, K, A, _stream())
    assert rc == 0
    return o


def _np_clip(g, noise, low, high):
    t = g + noise
    assert t.dtype == np.float32
    return np.clip(t, low, high)


def _layer_errors(h, w, b, got):
    """(max |torch f32 CPU F.linear - float64|, max |got - float64|)"""
    ref = F.linear(h.double(), w.double(), b.double())
    yard = F.linear(h, w, b).double()
    return float((yard - ref).abs().max()), float((torch.from_numpy(got).double() - ref).abs().max())


@functools.lru_cache(maxsize=None)
def _squashed_sweep():
    """Every shape, both scale formulas, sampled and mode: exactness asserted on the way, the layer's
    errors returned."""
    dev = _dev()
    errs = []
    for K, A, M in SHAPES:
        h, w, b = _operands(K, 2 * A, M, 31 * K + 7 * A + M)
        g = torch.Generator().manual_seed(K + A + M)
        eps = torch.randn(M, A, generator=g).to(dev)
        hd, wd, bd = h.to(dev), w.to(dev), b.to(dev)
        zero = torch.zeros(M, A, device=dev)
        for mode in (0, 1):
            tag = "K=%d A=%d M=%d mode=%d" % (K, A, M, mode)
            o = _squashed(hd, wd, bd, mode, eps, A)
            x = o["x"].done("x_out " + tag).reshape(M, 2 * A)
            xd = o["x"].t.view(M, 2 * A)
            _same("action " + tag, o["action"].done("action " + tag).reshape(M, A), _head_fwd(xd, mode, eps, A))
            o2 = _squashed(hd, wd, bd, mode, None, A, want_x=False)
            _same("mode " + tag, o2["action"].done("mode action " + tag).reshape(M, A), _head_fwd(xd, mode, zero, A))
            errs.append((tag,) + _layer_errors(h, w, b, x))
    return errs


@functools.lru_cache(maxsize=None)
def _deterministic_sweep():
    dev = _dev()
    errs, tanh_err = [], [0.0, 0.0]
    for n, (K, A, M) in enumerate(SHAPES):
        h, w, b = _operands(K, A, M, 17 * K + 5 * A + M)
        g = torch.Generator().manual_seed(K * A + M)
        lo_a, hi_a = -0.5 - torch.rand(A, generator=g), 0.5 + torch.rand(A, generator=g)
        bound = ((hi_a - lo_a) / 2, (hi_a + lo_a) / 2) if n % 2 == 0 else None
        noise = 0.5 * torch.randn(M, A, generator=g)
        low, high = lo_a + 0.3, hi_a - 0.3
        low[0::3], high[1::3] = -float("inf"), float("inf")         # absent sides
        hd, wd, bd = h.to(dev), w.to(dev), b.to(dev)
        bd_ = tuple(t.to(dev) for t in bound) if bound else None
        tag = "K=%d A=%d M=%d %s" % (K, A, M, "bounded" if bound else "unbounded")
        o = _deterministic(hd, wd, bd, bd_, noise.to(dev), low.to(dev), high.to(dev))
        y = o["y"].done("y_out " + tag).reshape(M, A)
        greedy = o["greedy"].done("greedy_out " + tag).reshape(M, A)
        yd = o["y"].t.view(M, A)
        if bound:
            want = torch.tanh(yd) * bd_[0] + bd_[1]
            if not torch.equal(want, o["greedy"].t.view(M, A)):
                # this build's tanhf is not torch's: both against float64, the kernel no worse
                ref = torch.tanh(yd.double()) * bd_[0].double() + bd_[1].double()
                tanh_err[0] = max(tanh_err[0], float((want.double() - ref).abs().max()))
                tanh_err[1] = max(tanh_err[1], float((o["greedy"].t.view(M, A).double() - ref).abs().max()))
        else:
            _same("greedy is y " + tag, greedy, y)
        _same("action " + tag, o["action"].done("action " + tag).reshape(M, A),
              _np_clip(greedy, noise.numpy(), low.numpy(), high.numpy()))
        o2 = _deterministic(hd, wd, bd, bd_, None, None, None, want=())
        _same("greedy action " + tag, o2["action"].done("action, no noise " + tag).reshape(M, A), greedy)
        errs.append((tag,) + _layer_errors(h, w, b, y))
    return errs, tanh_err


def test_squashed_every_shape_matches_head_fwd_bit_for_bit():
    assert len(_squashed_sweep()) == 2 * len(SHAPES)
    assert {s[0] for s in SHAPES} == set(K_LIST) and {s[1] for s in SHAPES} == set(A_LIST)
    assert {s[2] for s in SHAPES} == set(M_LIST)


def test_deterministic_every_shape_matches_torch_and_numpy_bit_for_bit():
    errs, (torch_err, kernel_err) = _deterministic_sweep()
    assert len(errs) == len(SHAPES)
    print("TANH torch_max_err %.3e kernel_max_err %.3e (0: equal bits everywhere)" % (torch_err, kernel_err))
    assert kernel_err <= torch_err


def _report(entry, errs):
    yard, mine = max(e[1] for e in errs), max(e[2] for e in errs)
    for tag, y, m in errs:
        print("LAYER %s %s torch_f32_max_err %.3e kernel_max_err %.3e" % (entry, tag, y, m))
    print("MAX %s torch_f32_max_err %.3e kernel_max_err %.3e ratio %.3f" % (entry, yard, mine, mine / yard))
    assert mine <= 2 * yard, "%s: kernel %.3e > 2 x torch float32 %.3e" % (entry, mine, yard)


def test_squashed_layer_against_float64():
    _report("pfrl_squashed_head_act", _squashed_sweep())


def test_deterministic_layer_against_float64():
    _report("pfrl_deterministic_head_act", _deterministic_sweep()[0])


@pytest.mark.parametrize("mode", [0, 1])
def test_squashed_planted_log_scales(mode):
    """Log-scales below clamp_lo, above clamp_hi and at +-1e4, as the bias over a zero product: x is
    the planted row itself."""
    dev = _dev()
    A = 6
    row = torch.tensor([0.3, -1.2, 2.5, 0.5, 7.0, -40.0, -25.0, 5.0, 1e4, -1e4, 0.3, -20.0])
    h, w = torch.zeros(1, 1, device=dev), torch.zeros(2 * A, 1, device=dev)
    eps = torch.tensor([[0.5, -1.5, 2.0, 1.0, -0.25, 3.0]], device=dev)
    o = _squashed(h, w, row.to(dev), mode, eps, A)
    x = o["x"].done("x_out").reshape(1, 2 * A)
    _same("x is the planted row", x, row.numpy().reshape(1, -1))
    got = o["action"].done("action").reshape(1, A)
    _same("planted action", got, _head_fwd(o["x"].t.view(1, 2 * A), mode, eps, A))
    scale = np.exp(np.clip(row.numpy()[A:].astype(np.float64), *CLAMP))
    want = np.tanh(row.numpy()[:A].astype(np.float64) + eps.cpu().numpy()[0].astype(np.float64) * scale)
    np.testing.assert_allclose(got[0], want, rtol=1e-5, atol=1e-6)
    o = _squashed(h, w, row.to(dev), mode, None, A, want_x=False)
    np.testing.assert_allclose(o["action"].done("mode")[:A], np.tanh(row.numpy()[:A].astype(np.float64)),
                               rtol=1e-6, atol=1e-7)


def test_deterministic_planted_rows():
    """Rows on each bound, outside each bound, with infinite bounds and with a NaN: np.clip in
    float32.  The policy output is the bias over a zero product."""
    dev = _dev()
    inf, nan = float("inf"), float("nan")
    g = np.array([0.25, -0.5, 0.75, 0.1, 0.3, 0.2, -0.9, 0.6], dtype=np.float32)
    low = np.array([-1.0, -1.0, -inf, -inf, -1.0, -inf, -0.5, 0.5], dtype=np.float32)
    high = np.array([1.0, 1.0, 1.0, inf, inf, inf, 0.5, 0.5], dtype=np.float32)
    A = g.size
    noise = np.stack([
        low - g, high - g,                                       # on (or next to) each bound
        np.full(A, -3.0, dtype=np.float32), np.full(A, 3.0, dtype=np.float32),        # outside each
        np.array([nan, 0.1, nan, nan, 0.2, nan, 0.0, nan], dtype=np.float32),
        np.array([inf, -inf, inf, inf, -inf, -inf, inf, -inf], dtype=np.float32),
        np.zeros(A, dtype=np.float32)])
    M = noise.shape[0]
    want = _np_clip(np.broadcast_to(g, (M, A)), noise, low, high)
    assert np.isnan(want[4, 0]) and want[2, 0] == -1.0 and want[3, 0] == 1.0 and want[3, 3] == g[3] + 3.0
    h, w = torch.zeros(M, 1, device=dev), torch.zeros(A, 1, device=dev)
    o = _deterministic(h, w, torch.from_numpy(g).to(dev), None, torch.from_numpy(noise).to(dev),
                       torch.from_numpy(low).to(dev), torch.from_numpy(high).to(dev))
    _same("y is the planted row", o["y"].done("y_out").reshape(M, A), np.broadcast_to(g, (M, A)))
    _same("planted action", o["action"].done("action", nan_ok=True).reshape(M, A), want)


def test_rows_do_not_depend_on_the_batch():
    """Every row of an M = 65 launch is the M = 1 launch on that row alone, bit for bit."""
    dev = _dev()
    K, A, M = 300, 17, 65
    h, w, b = _operands(K, 2 * A, M, 5)
    g = torch.Generator().manual_seed(6)
    eps = torch.randn(M, A, generator=g).to(dev)
    noise = torch.randn(M, A, generator=g).to(dev)
    low, high = torch.full((A,), -0.8, device=dev), torch.full((A,), 0.9, device=dev)
    bound = (torch.full((A,), 1.5, device=dev), torch.full((A,), 0.25, device=dev))
    hd, wd, bd = h.to(dev), w.to(dev), b.to(dev)
    whole = _squashed(hd, wd, bd, 0, eps, A)
    wx, wa = whole["x"].done("x").reshape(M, 2 * A), whole["action"].done("action").reshape(M, A)
    dwhole = _deterministic(hd, wd[:A].contiguous(), bd[:A].contiguous(), bound, noise, low, high)
    dy, da = dwhole["y"].done("y").reshape(M, A), dwhole["action"].done("action").reshape(M, A)
    for m in range(M):
        one = _squashed(hd[m:m + 1].contiguous(), wd, bd, 0, eps[m:m + 1].contiguous(), A)
        _same("x row %d" % m, one["x"].done("x"), wx[m])
        _same("action row %d" % m, one["action"].done("action"), wa[m])
        one = _deterministic(hd[m:m + 1].contiguous(), wd[:A].contiguous(), bd[:A].contiguous(), bound,
                             noise[m:m + 1].contiguous(), low, high)
        _same("y row %d" % m, one["y"].done("y"), dy[m])
        _same("deterministic action row %d" % m, one["action"].done("action"), da[m])


def test_refusals_write_nothing():
    dev = _dev()
    h, w, b = torch.zeros(4, 8, device=dev), torch.zeros(64, 8, device=dev), torch.zeros(64, device=dev)
    eps = torch.zeros(4, 32, device=dev)
    vec = torch.zeros(32, device=dev)
    L = _native.lib()
    cases = [dict(A=0), dict(A=33), dict(K=0), dict(K=1025), dict(M=-1), dict(M=4097), dict(h=None),
             dict(w=None), dict(b=None), dict(action=None)]
    for kw in cases:
        outs = [_Guarded(4 * 64), _Guarded(4 * 32)]
        action = kw["action"] if "action" in kw else outs[1].t
        rc = L.pfrl_squashed_head_act(_p(kw.get("h", h)), _p(kw.get("w", w)), _p(kw.get("b", b)), -20.0, 2.0, 0,
                                      _p(eps), _p(outs[0].t), _p(action), kw.get("M", 4), kw.get("K", 8),
                                      kw.get("A", 2), _stream())
        assert rc == PFRL_ERR_ARG, ("squashed", kw)
        outs += [_Guarded(4 * 32), _Guarded(4 * 32), _Guarded(4 * 32)]
        action = kw["action"] if "action" in kw else outs[4].t
        rc = L.pfrl_deterministic_head_act(_p(kw.get("h", h)), _p(kw.get("w", w)), _p(kw.get("b", b)), _p(vec),
                                           _p(vec), _p(eps), _p(vec), _p(vec), _p(outs[2].t), _p(outs[3].t),
                                           _p(action), kw.get("M", 4), kw.get("K", 8), kw.get("A", 2), _stream())
        assert rc == PFRL_ERR_ARG, ("deterministic", kw)
        torch.cuda.synchronize()
        for i, o in enumerate(outs):
            o.untouched("output %d (%r)" % (i, kw))
    for kw in (dict(mode=2), dict(lo=3.0)):                 # (no such head)
        outs = [_Guarded(4 * 64), _Guarded(4 * 32)]
        assert L.pfrl_squashed_head_act(_p(h), _p(w), _p(b), kw.get("lo", -20.0), 2.0, kw.get("mode", 0), _p(eps),
                                        _p(outs[0].t), _p(outs[1].t), 4, 8, 2, _stream()) == PFRL_ERR_ARG
        torch.cuda.synchronize()
        for o in outs:
            o.untouched("output (%r)" % kw)
    outs = [_Guarded(4 * 64), _Guarded(4 * 32), _Guarded(4 * 32), _Guarded(4 * 32), _Guarded(4 * 32)]
    assert L.pfrl_squashed_head_act(_p(h), _p(w), _p(b), -20.0, 2.0, 0, _p(eps), _p(outs[0].t), _p(outs[1].t),
                                    0, 8, 2, _stream()) == 0
    assert L.pfrl_deterministic_head_act(_p(h), _p(w), _p(b), _p(vec), _p(vec), _p(eps), _p(vec), _p(vec),
                                         _p(outs[2].t), _p(outs[3].t), _p(outs[4].t), 0, 8, 2, _stream()) == 0
    torch.cuda.synchronize()
    for i, o in enumerate(outs):
        o.untouched("output %d (M = 0)" % i)


def test_graph_replays_equal_direct_launches():
    """One captured graph of both launches, replayed three times on inputs rewritten in place: the
    direct launch's bits each time."""
    dev = _dev()
    K, A, M = 256, 17, 37
    h, w, b = _operands(K, 2 * A, M, 9)
    hd, wd, bd = h.to(dev), w.to(dev), b.to(dev)
    wa, ba = wd[:A].contiguous(), bd[:A].contiguous()
    eps, noise = torch.zeros(M, A, device=dev), torch.zeros(M, A, device=dev)
    low, high = torch.full((A,), -0.7, device=dev), torch.full((A,), 0.7, device=dev)
    bound = (torch.full((A,), 2.0, device=dev), torch.full((A,), -0.5, device=dev))
    L = _native.lib()
    og = {"x": _Guarded(M * 2 * A), "a": _Guarded(M * A), "y": _Guarded(M * A), "g": _Guarded(M * A),
          "d": _Guarded(M * A)}

    def both(o):
        assert L.pfrl_squashed_head_act(_p(hd), _p(wd), _p(bd), -20.0, 2.0, 0, _p(eps), _p(o["x"].t),
                                        _p(o["a"].t), M, K, A, _stream()) == 0
        assert L.pfrl_deterministic_head_act(_p(hd), _p(wa), _p(ba), _p(bound[0]), _p(bound[1]), _p(noise),
                                             _p(low), _p(high), _p(o["y"].t), _p(o["g"].t), _p(o["d"].t), M, K,
                                             A, _stream()) == 0

    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        both(og)
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        both(og)
    seen = []
    for rep in range(3):
        g = torch.Generator().manual_seed(50 + rep)
        hd.copy_(torch.randn(M, K, generator=g).to(dev))
        eps.copy_(torch.randn(M, A, generator=g).to(dev))
        noise.copy_(torch.randn(M, A, generator=g).to(dev))
        for o in og.values():
            o.full.fill_(float("nan"))
        graph.replay()
        got = {k: o.done("replayed " + k) for k, o in og.items()}
        oe = {k: _Guarded(o.n) for k, o in og.items()}
        both(oe)
        for k, o in oe.items():
            _same("replay %d, %s" % (rep, k), got[k], o.done("direct " + k))
        seen.append(got["a"].copy())
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])
