"""Boltzmann exploration on the device step, CPU tier: the NumPy restatement of the kernels' row
arithmetic (tests/_boltzmann_restatement.py) is pinned to what the reference does --
``np.random.choice(np.arange(A), p=softmax(q / T))`` per env on NumPy's global stream
(pfrl/explorers/boltzmann.py:18-26) -- and the gate of agents/_dqn_device_step.py is checked as a
decision table.  The kernels themselves are compared with the same restatement in
tests/test_boltzmann_head.py.
"""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _boltzmann_restatement as R  # noqa: E402

from pfrl_amd import _native, action_value, explorers  # noqa: E402
from pfrl_amd.agents import _dqn_device_step as ds  # noqa: E402
from pfrl_amd.agents.dqn import DQN  # noqa: E402
from pfrl_amd.device_store import DeviceObsBatch  # noqa: E402


def _same_rng_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def _reference_probs(q, T):
    """What Boltzmann.select_action hands to choice, on the CPU (where the reference's fixtures
    come from): float32 softmax of q / T, one row at a time."""
    q = torch.from_numpy(q)
    return np.stack([torch.softmax(q[i:i + 1] / T, dim=-1).numpy().ravel() for i in range(q.shape[0])])


@pytest.mark.parametrize("T", [0.01, 1.0, 50.0])
@pytest.mark.parametrize("A", [1, 2, 3, 6, 18, 64])
@pytest.mark.parametrize("source", ["reference", "restatement"])
def test_actions_equal_scalar_choice_calls_on_the_same_stream(A, T, source):
    """N scalar ``choice`` calls against the restatement on ``random_sample(N)`` from the same
    saved state: the same actions, and the stream ends at the same position."""
    N = 64
    rs = np.random.RandomState(1000 * A + int(T * 100))
    q = (rs.standard_normal((N, A)) * 3).astype(np.float32)
    p = _reference_probs(q, T) if source == "reference" else R.probs_f32(q, T)
    assert p.dtype == np.float32
    saved = np.random.get_state()
    try:
        np.random.seed(7 + A)
        s0 = np.random.get_state()
        want = np.array([np.random.choice(np.arange(A), p=p[i]) for i in range(N)], dtype=np.int64)
        s_choice = np.random.get_state()
        np.random.set_state(s0)
        u = np.random.random_sample(N)
        s_batch = np.random.get_state()
    finally:
        np.random.set_state(saved)
    assert _same_rng_state(s_choice, s_batch)
    got = R.actions(p, u)
    np.testing.assert_array_equal(got, want)
    assert got.min() >= 0 and got.max() <= A - 1


def test_restated_softmax_is_the_reference_softmax_to_rounding():
    """The float32 half of the restatement against torch's float32 CPU softmax.  z = q / T and
    z - max z are the same correctly rounded operations on both sides; what differs is the ``exp``
    (taken as accurate to 1 ulp = 2 u on either side, u = 2^-24) and the order of the A - 1
    additions of the denominator (at most (A - 1) u relative on either side), then one division
    each: |dp| <= (2 + 2 + 2 (A - 1) + 2) u p = (2 A + 4) u p, plus 2^-126 where p is subnormal."""
    rs = np.random.RandomState(3)
    u = 2.0 ** -24
    for A in (1, 2, 3, 6, 18, 64):
        for T in (0.01, 1.0, 50.0):
            q = (rs.standard_normal((64, A)) * 3).astype(np.float32)
            ref = _reference_probs(q, T).astype(np.float64)
            err = np.abs(R.probs_f32(q, T).astype(np.float64) - ref)
            assert (err <= (2 * A + 4) * u * ref + 2.0 ** -126).all(), (A, T, err.max())


@pytest.mark.parametrize("A", [3, 6, 18, 64])
def test_planted_rows(A):
    """The ends of the uniform's range, ties, all the mass on one action (zeros in the cdf), -inf
    entries: the restatement equals numpy's own three lines on the given uniform.  NaN, +inf and
    all -inf rows: ``choice`` raises its ValueError, the restatement answers -1."""
    q, T, u, nan_rows = R.planted_rows(A)
    p = R.probs_f32(q, T)
    got = R.actions(p, u)
    assert np.array_equal(np.isnan(p).any(axis=1), nan_rows)
    for i in range(q.shape[0]):
        if nan_rows[i]:
            assert got[i] == -1
            with pytest.raises(ValueError, match="NaN"):
                np.random.choice(np.arange(A), p=p[i])
            continue
        cdf = p[i].astype(np.float64).cumsum()
        cdf /= cdf[-1]
        assert got[i] == cdf.searchsorted(u[i], side="right"), i
        assert 0 <= got[i] <= A - 1 and p[i, got[i]] > 0, i    # never an action of probability 0
    # spot checks of what the rows were planted for
    first = {tuple(r): int(a) for r, a, x in zip(q.tolist(), got, u) if x == 0.0 and a >= 0}
    assert first[tuple([0.0, 1000.0] + [0.0] * (A - 2))] == 1          # u = 0 skips the leading zero
    assert first[tuple([0.0] * (A - 1) + [1000.0])] == A - 1
    last = {tuple(r): int(a) for r, a, x in zip(q.tolist(), got, u) if x == R.U_MAX and a >= 0}
    assert last[tuple([1000.0] + [0.0] * (A - 1))] == 0                # u -> 1 stays on the mass
    assert last[tuple([0.0] * A)] == A - 1


# ------------------------------------------------------------------ the gate
def _agent(explorer, training=True, recurrent=False, device="cuda"):
    a = types.SimpleNamespace(explorer=explorer, training=training, recurrent=recurrent,
                              device=torch.device(device))
    a._explorer_draws_before_greedy = lambda: DQN._explorer_draws_before_greedy(a)
    return a


def _batch():
    return DeviceObsBatch(None, np.zeros((2, 4), dtype=np.int32), np.zeros(2, dtype=np.int64))


class _SubBoltzmann(explorers.Boltzmann):
    pass


def _overridden():
    ex = explorers.Boltzmann(1.0)
    ex.select_action = lambda t, greedy_action_func, action_value=None: 0
    return ex


def _eps():
    return explorers.LinearDecayEpsilonGreedy(1.0, 0.1, 100, lambda: 0)


@pytest.mark.parametrize("make, kw, want", [
    (lambda: explorers.Boltzmann(1.0), {}, ds.BOLTZMANN),
    (lambda: explorers.Boltzmann(0.01), {}, ds.BOLTZMANN),
    (lambda: explorers.Boltzmann(np.float32(50)), {}, ds.BOLTZMANN),
    (lambda: explorers.Boltzmann(2), {}, ds.BOLTZMANN),
    (lambda: explorers.Boltzmann(0.0), {}, None),
    (lambda: explorers.Boltzmann(-1.0), {}, None),
    (lambda: explorers.Boltzmann(float("inf")), {}, None),
    (lambda: explorers.Boltzmann(float("nan")), {}, None),
    (lambda: explorers.Boltzmann(1e-50), {}, None),          # 0 as float32
    (lambda: explorers.Boltzmann(1e50), {}, None),           # inf as float32
    (lambda: explorers.Boltzmann("1"), {}, None),
    (lambda: explorers.Boltzmann(True), {}, None),
    (lambda: _SubBoltzmann(1.0), {}, None),
    (_overridden, {}, None),
    (lambda: explorers.Boltzmann(1.0), {"training": False}, None),
    (lambda: explorers.Boltzmann(1.0), {"recurrent": True}, None),
    (lambda: explorers.Boltzmann(1.0), {"device": "cpu"}, None),
    (_eps, {}, ds.EPS_GREEDY),
    (lambda: explorers.ConstantEpsilonGreedy(0.1, lambda: 0), {}, ds.EPS_GREEDY),
    (_eps, {"recurrent": True}, None),
    (_eps, {"device": "cpu"}, None),
    (lambda: explorers.Greedy(), {}, None),
])
def test_gate_decision_table(make, kw, want):
    assert ds.act_kind(_agent(make(), **kw), _batch()) == want
    # a host batch (list of observations) never takes the device step
    assert ds.act_kind(_agent(make(), **kw), [np.zeros(4)] * 2) is None


def test_gate_on_the_action_values():
    """Plain ``DiscreteActionValue`` rows of 1 .. 64 float32 actions; a distributional action value,
    a 65th action or another dtype keep the per-env branch."""
    mk = lambda A, dt=torch.float32: action_value.DiscreteActionValue(torch.zeros(3, A, dtype=dt))  # noqa: E731
    for A in (1, 16, 17, 64):
        q = ds.boltzmann_action_values(mk(A))
        assert q is not None and q.shape == (3, A) and q.is_contiguous()
    assert ds.boltzmann_action_values(mk(65)) is None
    assert ds.boltzmann_action_values(mk(6, torch.float64)) is None
    dist = action_value.DistributionalDiscreteActionValue(torch.full((3, 6, 5), 0.2), torch.arange(5.0))
    assert ds.boltzmann_action_values(dist) is None
    assert ds.MAX_BOLTZMANN_ACTIONS == 64


def test_entry_points_are_declared_bound_and_documented():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "pfrl_amd.h")).read()
    doc = open(os.path.join(root, "INTEGRATION.md")).read()
    from pfrl_amd import ops

    for name in ("pfrl_dqn_act_head_boltzmann", "pfrl_boltzmann_select"):
        assert name + "(" in header and name in _native.EXPORTS and name in doc, name
    assert "pfrl/explorers/boltzmann.py:18-26" in header and "pfrl/agents/dqn.py:490-507" in header
    assert callable(ops.dqn_act_head_boltzmann) and callable(ops.boltzmann_select)
