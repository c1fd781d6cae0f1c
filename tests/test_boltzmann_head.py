"""``pfrl_dqn_act_head_boltzmann`` (csrc/qnet.hip) and ``pfrl_boltzmann_select`` (csrc/frames.hip)
through the C ABI, in the style of tests/test_loss_head_envelope.py: every output lies between two
guard zones that must be untouched after the launch, and the payload must be fully written.

What is exact and what is rounded:

* ``q`` of the fused entry equals ``pfrl_linear_small_fwd`` bit for bit.
* From the float32 probabilities on, the kernels work in float64 in a fixed order (cumulative sum,
  normalisation, count of entries <= u), so ``action`` equals the NumPy restatement
  (tests/_boltzmann_restatement.py, pinned to ``np.random.choice`` in tests/test_boltzmann_cpu.py)
  applied to the kernel's OWN ``probs`` with ``==``, in every row of every case.
* Both entries give the same ``probs`` and ``action`` bits on the same ``q``.
* ``probs`` against the float64 softmax of the same ``q`` (z = q / T with T the float32 the kernel
  reads): the yardstick is torch's own float32 CPU softmax of the same ``q / T``, measured against
  the same float64 reference on the same inputs; the kernels may err twice as much (another ``expf``,
  a sequential denominator).  Maxima are taken per entry and temperature over all shapes of the
  entry (RATIO lines with ``pytest -s``), because the temperature sets the size of the shared
  rounding error of z: at T = 0.01 it hides everything else.
"""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _boltzmann_restatement as R  # noqa: E402

from pfrl_amd import _native  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 4096
PFRL_ERR_ARG = -2
TEMPERATURES = (0.01, 1.0, 50.0)
FUSED_M, FUSED_N, FUSED_K = (1, 2, 255, 257), (1, 2, 3, 6, 16), (1, 512, 1023, 1024, 1025)
SELECT_M, SELECT_A = (1, 255, 256, 257), (1, 2, 17, 18, 63, 64)


def _dev():
    return torch.device("cuda:0")


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class _Guarded:
    """n elements between two guard zones holding a mark no kernel writes (NaN for floats)."""

    def __init__(self, n, dtype):
        self.n = n
        self.mark = float("nan") if dtype.is_floating_point else -(1 << 30)
        self.full = torch.full((n + 2 * GUARD,), self.mark, dtype=dtype, device=_dev())
        self.t = self.full[GUARD:GUARD + n]

    def _marked(self, t):
        return torch.isnan(t) if self.full.dtype.is_floating_point else t == self.mark

    def done(self, what, nan_ok=False):
        assert bool(self._marked(self.full[:GUARD]).all()), "guard zone before %s was written" % what
        assert bool(self._marked(self.full[GUARD + self.n:]).all()), "guard zone after %s was written" % what
        if not nan_ok:
            assert not bool(self._marked(self.t).any()), "%s: payload not fully written" % what
        return self.t.cpu().numpy()

    def untouched(self, what):
        assert bool(self._marked(self.full).all()), "%s was written" % what


def _outputs(M, A, want_q=True):
    return dict(q=_Guarded(M * A, torch.float32) if want_q else None, probs=_Guarded(M * A, torch.float32),
                action=_Guarded(M, torch.int64), status=_Guarded(1, torch.int32))


def _collect(o, M, A, nan_ok=False):
    """Guard zones checked; the status word is a plain OR into whatever it held: it starts at 0."""
    out = {"probs": o["probs"].done("probs", nan_ok).reshape(M, A), "action": o["action"].done("action"),
           "status": int(o["status"].done("status")[0])}
    if o["q"] is not None:
        out["q"] = o["q"].done("q", nan_ok).reshape(M, A)
    return out


def _draws(M, seed):
    u = np.random.RandomState(seed).random_sample(M)
    u[0], u[-1] = 0.0, R.U_MAX                 # (M == 1: the largest uniform)
    return u


def _launch_fused(h, w, b, u, T, o):
    M, K = h.shape
    o["status"].t.zero_()
    return _native.lib().pfrl_dqn_act_head_boltzmann(
        _p(h), _p(w), _p(b), _p(u), _p(T), _p(o["q"].t if o["q"] is not None else None), _p(o["probs"].t),
        _p(o["action"].t), _p(o["status"].t), M, K, w.shape[0], _stream())


def _launch_select(q, u, T, o):
    M, A = q.shape
    o["status"].t.zero_()
    return _native.lib().pfrl_boltzmann_select(_p(q), _p(u), _p(T), _p(o["probs"].t), _p(o["action"].t),
                                               _p(o["status"].t), M, A, _stream())


def _bits(x):
    return np.ascontiguousarray(x).view(np.int32)


def _same_bits_nan_for_nan(a, b):
    """Bit-identical, except that any NaN stands for any NaN (payloads are not part of the contract)."""
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(_bits(a)[~na], _bits(b)[~nb])


def _check_rows(tag, got, u, nan_rows=None):
    """action == restatement(kernel's own probs) with ==, every row; -1 and status exactly for NaN rows."""
    want = R.actions(got["probs"], u)
    np.testing.assert_array_equal(got["action"], want, err_msg=tag)
    bad = np.isnan(got["probs"]).any(axis=1)
    if nan_rows is None:
        nan_rows = np.zeros(len(u), dtype=bool)
    np.testing.assert_array_equal(bad, nan_rows, err_msg=tag)
    np.testing.assert_array_equal(got["action"] == -1, nan_rows, err_msg=tag)
    assert (got["status"] != 0) == bool(nan_rows.any()), tag
    ok = ~nan_rows
    A = got["probs"].shape[1]
    assert ((got["action"][ok] >= 0) & (got["action"][ok] <= A - 1)).all(), tag


@functools.lru_cache(maxsize=None)
def _fused_case(M, N, K, with_bias):
    """One launch of the fused entry (+ pfrl_linear_small_fwd and the standalone entry on its q);
    everything back on the host."""
    dev = _dev()
    g = torch.Generator().manual_seed(M * 7919 + N * 131 + K * 3 + with_bias)
    h = torch.randn(M, K, generator=g).to(dev)
    w = (torch.randn(N, K, generator=g) * (2.0 / K ** 0.5)).to(dev)
    b = torch.randn(N, generator=g).to(dev) if with_bias else None
    T32 = np.float32(TEMPERATURES[(M + N + K + with_bias) % 3])
    T = torch.tensor([T32], dtype=torch.float32, device=dev)
    u = _draws(M, M + N + K)
    ud = torch.from_numpy(u).to(dev)
    q_ref = _Guarded(M * N, torch.float32)
    assert _native.lib().pfrl_linear_small_fwd(_p(h), _p(w), _p(b), _p(q_ref.t), M, K, N, _stream()) == 0
    o = _outputs(M, N)
    assert _launch_fused(h, w, b, ud, T, o) == 0
    fused = _collect(o, M, N)
    o2 = _outputs(M, N, want_q=False)
    assert _launch_select(o["q"].t.view(M, N), ud, T, o2) == 0
    return dict(fused=fused, select=_collect(o2, M, N), q_ref=q_ref.done("q_ref").reshape(M, N), u=u, T=T32)


@functools.lru_cache(maxsize=None)
def _select_case(M, A):
    dev = _dev()
    g = torch.Generator().manual_seed(M * 101 + A)
    q = (torch.randn(M, A, generator=g) * 3).to(dev)
    T32 = np.float32(TEMPERATURES[(M + A) % 3])
    T = torch.tensor([T32], dtype=torch.float32, device=dev)
    u = _draws(M, M + A)
    o = _outputs(M, A, want_q=False)
    assert _launch_select(q, torch.from_numpy(u).to(dev), T, o) == 0
    return dict(select=_collect(o, M, A), q=q.cpu().numpy(), u=u, T=T32)


@pytest.mark.parametrize("N", FUSED_N)
def test_fused_entry_every_shape(N):
    """M in {1, 2, 255, 257} x K on both sides of small_fwd_row's 1024-element trip x bias / NULL:
    q bit-identical to pfrl_linear_small_fwd, actions exact, no status, and the standalone entry
    gives the same probs and action bits on the same q."""
    for K in FUSED_K:
        for M in FUSED_M:
            for with_bias in (True, False):
                c = _fused_case(M, N, K, with_bias)
                tag = "M=%d N=%d K=%d bias=%d T=%g" % (M, N, K, with_bias, c["T"])
                assert np.array_equal(_bits(c["fused"]["q"]), _bits(c["q_ref"])), tag
                _check_rows(tag, c["fused"], c["u"])
                assert np.array_equal(_bits(c["fused"]["probs"]), _bits(c["select"]["probs"])), tag
                np.testing.assert_array_equal(c["fused"]["action"], c["select"]["action"], err_msg=tag)
                assert c["select"]["status"] == 0


@pytest.mark.parametrize("A", SELECT_A)
def test_select_entry_every_shape(A):
    """A on both sides of the fused head's width and at the limit, M around the 64-row workgroup
    and the 256 of the benchmark: actions exact, no status."""
    for M in SELECT_M:
        c = _select_case(M, A)
        _check_rows("M=%d A=%d T=%g" % (M, A, c["T"]), c["select"], c["u"])


def _errors(q, T32, probs):
    """(max |torch f32 CPU softmax - float64|, max |probs - float64|) on the same q and T."""
    q = torch.from_numpy(np.ascontiguousarray(q))
    ref = torch.softmax(q.double() / float(T32), dim=-1)
    yard = torch.softmax(q / float(T32), dim=-1).double()
    return float((yard - ref).abs().max()), float((torch.from_numpy(probs).double() - ref).abs().max())


def _accuracy(entry, cases):
    worst = {}
    for q, T32, probs in cases:
        yard, mine = _errors(q, T32, probs)
        w = worst.setdefault(float(T32), [0.0, 0.0])
        w[0], w[1] = max(w[0], yard), max(w[1], mine)
    for T32, (yard, mine) in sorted(worst.items()):
        print("RATIO %s T=%g torch_f32_max_err %.3e kernel_max_err %.3e ratio %.3f"
              % (entry, T32, yard, mine, mine / yard if yard else 0.0))
    print("MAX %s torch_f32_max_err %.3e kernel_max_err %.3e"
          % (entry, max(v[0] for v in worst.values()), max(v[1] for v in worst.values())))
    for T32, (yard, mine) in sorted(worst.items()):
        assert mine <= 2 * yard, "%s T=%g: kernel %.3e > 2 x torch float32 %.3e" % (entry, T32, mine, yard)


def test_fused_entry_probs_against_float64():
    _accuracy("pfrl_dqn_act_head_boltzmann",
              [(c["fused"]["q"], c["T"], c["fused"]["probs"])
               for c in (_fused_case(M, N, K, wb) for N in FUSED_N for K in FUSED_K for M in FUSED_M
                         for wb in (True, False))])


def test_select_entry_probs_against_float64():
    _accuracy("pfrl_boltzmann_select",
              [(c["q"], c["T"], c["select"]["probs"])
               for c in (_select_case(M, A) for A in SELECT_A for M in SELECT_M)])


def test_select_entry_refusals_write_nothing():
    dev = _dev()
    q = torch.zeros(4, 65, device=dev)
    u = torch.zeros(4, dtype=torch.float64, device=dev)
    T = torch.ones(1, device=dev)
    for kw in (dict(A=65), dict(A=0), dict(A=-1), dict(M=-1, A=6), dict(A=6, q=None), dict(A=6, u=None),
               dict(A=6, T=None), dict(A=6, action=None), dict(A=6, status=None)):
        o = _outputs(4, 65, want_q=False)
        o["status"].full.fill_(o["status"].mark)
        args = dict(kw)
        rc = _native.lib().pfrl_boltzmann_select(
            _p(args.get("q", q)), _p(args.get("u", u)), _p(args.get("T", T)), _p(o["probs"].t),
            _p(args.get("action", o["action"].t)), _p(args.get("status", o["status"].t)),
            args.get("M", 4), args["A"], _stream())
        assert rc == PFRL_ERR_ARG, kw
        torch.cuda.synchronize()
        for name in ("probs", "action", "status"):
            o[name].untouched("%s (%r)" % (name, kw))
    o = _outputs(4, 6, want_q=False)
    o["status"].full.fill_(o["status"].mark)
    assert _native.lib().pfrl_boltzmann_select(_p(q), _p(u), _p(T), _p(o["probs"].t), _p(o["action"].t),
                                               _p(o["status"].t), 0, 6, _stream()) == 0
    torch.cuda.synchronize()
    for name in ("probs", "action", "status"):
        o[name].untouched("%s (M = 0)" % name)


@pytest.mark.parametrize("A", [3, 6, 16, 18, 64])
def test_planted_rows(A):
    """The rows of tests/test_boltzmann_cpu.py on the device: the ends of the uniform's range, ties,
    all the mass on one action, -inf entries; action == -1 and status != 0 exactly for the NaN,
    +inf and all -inf rows.  The fused entry gets a row as its bias over a zero product, so that
    q is the planted row itself (A <= 16); both entries agree bit for bit."""
    dev = _dev()
    q, T32, u, nan_rows = R.planted_rows(A)
    Rn = q.shape[0]
    T = torch.tensor([T32], dtype=torch.float32, device=dev)
    ud = torch.from_numpy(u).to(dev)
    o = _outputs(Rn, A, want_q=False)
    assert _launch_select(torch.from_numpy(q).to(dev), ud, T, o) == 0
    sel = _collect(o, Rn, A, nan_ok=True)
    _check_rows("select A=%d" % A, sel, u, nan_rows)
    # ... and without the NaN rows the status word stays 0
    keep = np.flatnonzero(~nan_rows)
    o = _outputs(len(keep), A, want_q=False)
    assert _launch_select(torch.from_numpy(q[keep]).to(dev), torch.from_numpy(u[keep]).to(dev), T, o) == 0
    _check_rows("select A=%d, finite rows" % A, _collect(o, len(keep), A), u[keep])
    if A > 16:
        return
    h = torch.zeros(1, 1, device=dev)
    w = torch.zeros(A, 1, device=dev)
    for i in range(Rn):
        o = _outputs(1, A)
        assert _launch_fused(h, w, torch.from_numpy(q[i]).to(dev), ud[i:i + 1], T, o) == 0
        got = _collect(o, 1, A, nan_ok=True)
        assert _same_bits_nan_for_nan(got["q"], q[i:i + 1]), i
        _check_rows("fused A=%d row %d" % (A, i), got, u[i:i + 1], nan_rows[i:i + 1])
        assert _same_bits_nan_for_nan(got["probs"], sel["probs"][i:i + 1]), i
        assert got["action"][0] == sel["action"][i], i


def test_eager_launch_and_graph_replays_with_draws_and_temperature_rewritten_in_place():
    """One eager launch, then a ``torch.cuda.graph`` capture of both entries replayed three times
    with ``u`` and ``T`` rewritten in place: every replay equals the eager launch on the same
    inputs bit for bit and the restatement on its own probs."""
    dev = _dev()
    M, N, K = 37, 6, 512
    g = torch.Generator().manual_seed(5)
    h = torch.randn(M, K, generator=g).to(dev)
    w = (torch.randn(N, K, generator=g) * (2.0 / K ** 0.5)).to(dev)
    b = torch.randn(N, generator=g).to(dev)
    u = torch.zeros(M, dtype=torch.float64, device=dev)
    T = torch.ones(1, dtype=torch.float32, device=dev)
    og, og2 = _outputs(M, N), _outputs(M, N, want_q=False)

    def both(o, o2):
        assert _launch_fused(h, w, b, u, T, o) == 0
        assert _launch_select(o["q"].t.view(M, N), u, T, o2) == 0

    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        both(og, og2)
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        both(og, og2)
    seen = []
    for rep, T32 in enumerate((np.float32(1.0), np.float32(0.01), np.float32(50.0))):
        draws = _draws(M, 100 + rep)
        u.copy_(torch.from_numpy(draws).to(dev))
        T.fill_(float(T32))
        for o in (og, og2):                     # fresh marks: the replay has to write everything again
            for name in ("q", "probs", "action"):
                if o[name] is not None:
                    o[name].full.fill_(o[name].mark)
        graph.replay()
        rf, rs = _collect(og, M, N), _collect(og2, M, N)
        oe, oe2 = _outputs(M, N), _outputs(M, N, want_q=False)
        both(oe, oe2)
        ef = _collect(oe, M, N)
        for name in ("q", "probs"):
            assert np.array_equal(_bits(rf[name]), _bits(ef[name])), (rep, name)
        np.testing.assert_array_equal(rf["action"], ef["action"])
        assert np.array_equal(_bits(rf["probs"]), _bits(rs["probs"]))
        np.testing.assert_array_equal(rf["action"], rs["action"])
        _check_rows("replay %d" % rep, rf, draws)
        seen.append(rf["action"].copy())
    assert not np.array_equal(seen[0], seen[1]) or not np.array_equal(seen[1], seen[2])
