"""The host side of the continuous agents' device acting step (agents/_actor_device_step.py,
agents/_policy_split.py), where no GPU is needed:

* the explorers' noise restated (``gaussian_noise``, ``ou_noise``) against N scalar ``select_action``
  calls of the explorers themselves (reference pfrl/explorers/additive_gaussian.py:26-36,
  additive_ou.py:49-66), value for value, with NumPy's stream and the explorer left where the loop
  leaves them.  The action arithmetic next to it is the kernel's, in NumPy float32: g + noise, then
  the two compares;
* the table of what the step takes and what it leaves to the agents' own code;
* the two recognisers on the reference examples' policies and on near misses.
"""
import copy
import logging

import numpy as np
import pytest
import torch
from torch import nn

import pfrl_amd
from pfrl_amd import explorers
from pfrl_amd.agents import _actor_device_step as ads
from pfrl_amd.agents import _policy_split as ps
from pfrl_amd.utils import squashed_gaussian as sg

N_LIST, A_LIST = (1, 2, 7), (1, 3, 17)


def _state_equal(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def _kernel_clip(g, noise, low, high):
    """pfrl_deterministic_head_act behind g, in NumPy float32."""
    t = g + noise
    assert t.dtype == np.float32
    t = np.where(t < low, low, t)
    return np.where(t > high, high, t)


def _actions(N, A, seed):
    return np.random.RandomState(seed).uniform(-1.5, 1.5, size=(N, A)).astype(np.float32)


GAUSSIAN_SCALES = {"scalar": lambda A: 0.3, "array": lambda A: np.linspace(0.05, 0.8, A)}
GAUSSIAN_BOUNDS = {
    "none": lambda A: (None, None),
    "scalar": lambda A: (-1.0, 1),
    "float32 arrays": lambda A: (np.linspace(-1.2, -0.4, A).astype(np.float32),
                                 np.linspace(0.3, 1.1, A).astype(np.float32)),
    "low only": lambda A: (-0.5, None),
    "high only": lambda A: (None, np.full(1, 0.25, dtype=np.float32)),
}


@pytest.mark.parametrize("bounds", sorted(GAUSSIAN_BOUNDS))
@pytest.mark.parametrize("scale", sorted(GAUSSIAN_SCALES))
@pytest.mark.parametrize("A", A_LIST)
@pytest.mark.parametrize("N", N_LIST)
def test_additive_gaussian_restated(N, A, scale, bounds):
    low, high = GAUSSIAN_BOUNDS[bounds](A)
    ex = explorers.AdditiveGaussian(scale=GAUSSIAN_SCALES[scale](A), low=low, high=high)
    assert ads.explorer_kind(ex, A) == ads.GAUSSIAN
    a = _actions(N, A, 100 * N + A)
    np.random.seed(7)
    want = [ex.select_action(0, lambda i=i: a[i]) for i in range(N)]
    after = np.random.get_state()
    np.random.seed(7)
    noise = np.empty((N, A), dtype=np.float32)
    ads.gaussian_noise(ex, noise)
    assert _state_equal(np.random.get_state(), after)
    lo, hi = ads.gaussian_bounds(ex, A)
    assert lo.dtype == hi.dtype == np.float32 and lo.shape == hi.shape == (A,)
    got = _kernel_clip(a, noise, lo, hi)
    for i in range(N):
        assert want[i].dtype == np.float32 and want[i].shape == (A,)
        assert np.array_equal(got[i], want[i]), (i, got[i], want[i])


@pytest.mark.parametrize("sigma", ["scalar", "array"])
@pytest.mark.parametrize("start_with_mu", [False, True])
@pytest.mark.parametrize("A", A_LIST)
@pytest.mark.parametrize("N", N_LIST)
def test_additive_ou_restated(N, A, start_with_mu, sigma):
    sig = 0.3 if sigma == "scalar" else np.linspace(0.1, 0.5, A)
    ex = explorers.AdditiveOU(mu=0.1, theta=0.15, sigma=sig, start_with_mu=start_with_mu)
    ref = copy.deepcopy(ex)
    assert ex.ou_state is None
    np.random.seed(11)
    state = np.random.get_state()
    for step in range(3):                   # the first call creates the state, later ones evolve it
        assert ads.explorer_kind(ex, A) == ads.OU
        a = _actions(N, A, 1000 * step + 10 * N + A)
        np.random.set_state(state)
        want = [ref.select_action(step, lambda i=i: a[i]) for i in range(N)]
        after = np.random.get_state()
        np.random.set_state(state)
        noise = np.empty((N, A), dtype=np.float32)
        ads.ou_noise(ex, noise)
        state = np.random.get_state()
        assert _state_equal(state, after)
        assert ex.ou_state.dtype == np.float32 and ex.ou_state.shape == (A,)
        assert np.array_equal(ex.ou_state, ref.ou_state)
        got = _kernel_clip(a, noise, np.float32(-np.inf), np.float32(np.inf))
        for i in range(N):
            assert want[i].dtype == np.float32
            assert np.array_equal(got[i], want[i]), (step, i)
        assert np.array_equal(noise[N - 1], ex.ou_state)
    if start_with_mu:                       # (the first call of all drew nothing)
        np.random.seed(11)
        first = explorers.AdditiveOU(mu=0.1, sigma=sig, start_with_mu=True)
        ads.ou_noise(first, np.empty((1, A), dtype=np.float32))
        np.random.seed(11)
        fresh = np.random.get_state()
        ads.ou_noise(explorers.AdditiveOU(mu=0.1, sigma=sig, start_with_mu=True),
                     np.empty((1, A), dtype=np.float32))
        assert _state_equal(np.random.get_state(), fresh)
        assert np.array_equal(first.ou_state, np.full(A, 0.1, dtype=np.float32))


class _SubGaussian(explorers.AdditiveGaussian):
    pass


class _SubOU(explorers.AdditiveOU):
    pass


def _patched(ex, name="select_action"):
    setattr(ex, name, getattr(ex, name))
    return ex


def _ou(state=None, logger=None):
    ex = explorers.AdditiveOU() if logger is None else explorers.AdditiveOU(logger=logger)
    ex.ou_state = state
    return ex


def _debug_logger():
    lg = logging.getLogger("test_actor_act_cpu.debug")
    lg.setLevel(logging.DEBUG)
    return lg


A0 = 3
EXPLORER_TABLE = [
    ("greedy", lambda: explorers.Greedy(), ads.GREEDY),
    ("gaussian, no bounds", lambda: explorers.AdditiveGaussian(0.1), ads.GAUSSIAN),
    ("gaussian, Python scalars", lambda: explorers.AdditiveGaussian(0.1, low=-1, high=1.0), ads.GAUSSIAN),
    ("gaussian, float32 arrays", lambda: explorers.AdditiveGaussian(
        0.1, low=-np.ones(A0, dtype=np.float32), high=np.ones(A0, dtype=np.float32)), ads.GAUSSIAN),
    ("gaussian, infinite scalar", lambda: explorers.AdditiveGaussian(0.1, high=float("inf")), ads.GAUSSIAN),
    ("gaussian, float64 arrays", lambda: explorers.AdditiveGaussian(
        0.1, low=-np.ones(A0), high=np.ones(A0)), None),
    ("gaussian, one float64 array", lambda: explorers.AdditiveGaussian(
        0.1, low=-1.0, high=np.ones(A0)), None),
    ("gaussian, float64 NumPy scalar", lambda: explorers.AdditiveGaussian(0.1, low=np.float64(-1)), None),
    ("gaussian, float32 NumPy scalar", lambda: explorers.AdditiveGaussian(0.1, low=np.float32(-1)), None),
    ("gaussian, bool", lambda: explorers.AdditiveGaussian(0.1, high=True), None),
    ("gaussian, NaN", lambda: explorers.AdditiveGaussian(0.1, low=float("nan")), None),
    ("gaussian, scalar beyond float32", lambda: explorers.AdditiveGaussian(0.1, high=1e40), None),
    ("gaussian, array of another width", lambda: explorers.AdditiveGaussian(
        0.1, low=-np.ones(A0 + 1, dtype=np.float32)), None),
    ("gaussian, a list", lambda: explorers.AdditiveGaussian(0.1, low=[-1.0] * A0), None),
    ("gaussian, subclass", lambda: _SubGaussian(0.1), None),
    ("gaussian, patched select_action", lambda: _patched(explorers.AdditiveGaussian(0.1)), None),
    ("ou, fresh", lambda: _ou(), ads.OU),
    ("ou, float32 state", lambda: _ou(np.zeros(A0, dtype=np.float32)), ads.OU),
    ("ou, float64 state", lambda: _ou(np.zeros(A0)), None),
    ("ou, state of another width", lambda: _ou(np.zeros(A0 + 1, dtype=np.float32)), None),
    ("ou, 2-d state", lambda: _ou(np.zeros((1, A0), dtype=np.float32)), None),
    ("ou, DEBUG logging", lambda: _ou(logger=_debug_logger()), None),
    ("ou, subclass", lambda: _SubOU(), None),
    ("ou, patched evolve", lambda: _patched(_ou(), "evolve"), None),
    ("epsilon-greedy", lambda: explorers.ConstantEpsilonGreedy(0.1, lambda: 0), None),
    ("boltzmann", lambda: explorers.Boltzmann(), None),
]


@pytest.mark.parametrize("name,make,kind", EXPLORER_TABLE, ids=[row[0] for row in EXPLORER_TABLE])
def test_explorer_decision_table(name, make, kind):
    state = np.random.get_state()
    assert ads.explorer_kind(make(), A0) == kind
    assert _state_equal(np.random.get_state(), state)


def test_float64_bounds_would_change_the_reference_dtype():
    """Why they are refused: the reference's own result is float64 there."""
    ex = explorers.AdditiveGaussian(0.1, low=-np.ones(A0), high=np.ones(A0))
    assert ex.select_action(0, lambda: np.zeros(A0, dtype=np.float32)).dtype == np.float64


def test_observation_table():
    f32 = [np.zeros(11, dtype=np.float32) for _ in range(5)]
    assert ads.observation_shape(f32) == (11,)
    assert ads.observation_shape(tuple(f32)) == (11,)
    assert ads.observation_shape(np.zeros((5, 11), dtype=np.float32)) == (11,)
    assert ads.observation_shape([np.zeros((2, 3)) for _ in range(4)]) == (2, 3)
    assert ads.observation_shape([]) is None
    assert ads.observation_shape(f32[:4] + [np.zeros(12, dtype=np.float32)]) is None
    assert ads.observation_shape(f32[:4] + [np.zeros(11)]) is None
    assert ads.observation_shape([np.zeros(11, dtype=np.uint8)] * 3) is None
    assert ads.observation_shape([(o, o) for o in f32]) is None
    assert ads.observation_shape([list(o) for o in f32]) is None
    assert ads.observation_shape([np.float32(1.0)] * 3) is None
    assert ads.observation_shape([torch.zeros(11)] * 3) is None


def test_switches_and_cpu_agents(monkeypatch):
    assert ads.head_enabled() and ads.graph_enabled()
    monkeypatch.setenv("PFRL_ACTOR_ACT_HEAD", "0")
    monkeypatch.setenv("PFRL_ACTOR_ACT_GRAPH", "0")
    assert not ads.head_enabled() and not ads.graph_enabled()
    monkeypatch.delenv("PFRL_ACTOR_ACT_HEAD")
    # an agent on the CPU keeps its own acting code: actions as before, nothing counted
    policy = nn.Sequential(nn.Linear(4, 8), nn.ReLU(), nn.Linear(8, 2),
                           pfrl_amd.nn.BoundByTanh(low=-np.ones(2, dtype=np.float32),
                                                   high=np.ones(2, dtype=np.float32)),
                           pfrl_amd.policies.DeterministicHead())
    q = nn.Sequential(pfrl_amd.nn.ConcatObsAndAction(), nn.Linear(6, 8), nn.ReLU(), nn.Linear(8, 1))
    agent = pfrl_amd.agents.DDPG(policy, q, torch.optim.Adam(policy.parameters()),
                                 torch.optim.Adam(q.parameters()), pfrl_amd.replay_buffers.ReplayBuffer(100),
                                 gamma=0.99, explorer=explorers.AdditiveGaussian(0.1, low=-1.0, high=1.0),
                                 gpu=None, replay_start_size=10, minibatch_size=4)
    obs = [np.full(4, 0.1 * i, dtype=np.float32) for i in range(3)]
    before = ads.calls
    assert ads.deterministic_act(agent, obs, explore=True) is None
    assert ads.deterministic_act(agent, obs, explore=False) is None
    actions = agent.batch_act(obs)
    assert isinstance(actions, list) and len(actions) == 3
    assert all(a.dtype == np.float32 and a.shape == (2,) for a in actions)
    with agent.eval_mode():
        greedy = agent.batch_act(obs)
    assert isinstance(greedy, np.ndarray) and greedy.shape == (3, 2) and greedy.dtype == np.float32
    assert ads.calls == before


# -------------------------------------------------------------------------------------------------
# recognisers
# -------------------------------------------------------------------------------------------------
def _ddpg_example_policy(obs=17, A=6, last=None):
    """examples/mujoco/reproduction/ddpg/train_ddpg.py:133-141"""
    return nn.Sequential(nn.Linear(obs, 400), nn.ReLU(), nn.Linear(400, 300), nn.ReLU(),
                         last if last is not None else nn.Linear(300, A),
                         pfrl_amd.nn.BoundByTanh(low=-np.ones(A, dtype=np.float32),
                                                 high=np.ones(A, dtype=np.float32)),
                         pfrl_amd.policies.DeterministicHead())


def test_deterministic_policy_recognised():
    pol = _ddpg_example_policy()
    split = ps.deterministic_policy(pol)
    assert split is not None and split.layer is pol[4] and split.bound is pol[5]
    assert [id(m) for m in split.body.children()] == [id(m) for m in list(pol.children())[:4]]
    x = torch.randn(3, 17)
    with torch.no_grad():
        assert torch.equal(split.body(x), pol[3](pol[2](pol[1](pol[0](x)))))
    # without the bound (and a body of one module)
    bare = nn.Sequential(nn.ReLU(), nn.Linear(8, 2), pfrl_amd.policies.DeterministicHead())
    split = ps.deterministic_policy(bare)
    assert split is not None and split.layer is bare[1] and split.bound is None
    assert len(list(split.body.children())) == 1
    # the widest admitted layer
    assert ps.deterministic_policy(_ddpg_example_policy(A=32)) is not None
    wide = nn.Sequential(nn.Linear(4, 1024), nn.ReLU(), nn.Linear(1024, 2), pfrl_amd.policies.DeterministicHead())
    assert ps.deterministic_policy(wide) is not None


DETERMINISTIC_MISSES = {
    "no bias": lambda: _ddpg_example_policy(last=nn.Linear(300, 6, bias=False)),
    "float64 layer": lambda: _ddpg_example_policy(last=nn.Linear(300, 6).double()),
    "float64 body": lambda: _ddpg_example_policy().double(),
    "A = 33": lambda: _ddpg_example_policy(A=33),
    "K = 1025": lambda: nn.Sequential(nn.Linear(4, 1025), nn.ReLU(), nn.Linear(1025, 2),
                                       pfrl_amd.policies.DeterministicHead()),
    "empty body": lambda: nn.Sequential(nn.Linear(17, 6), pfrl_amd.policies.DeterministicHead()),
    "empty body, bound": lambda: nn.Sequential(nn.Linear(17, 6), pfrl_amd.nn.BoundByTanh(-1.0, 1.0),
                                                pfrl_amd.policies.DeterministicHead()),
    # the reference's TD3 example squashes with nn.Tanh (train_td3.py:122-130): not taken
    "nn.Tanh": lambda: nn.Sequential(nn.Linear(17, 400), nn.ReLU(), nn.Linear(400, 300), nn.ReLU(),
                                      nn.Linear(300, 6), nn.Tanh(), pfrl_amd.policies.DeterministicHead()),
    "no head": lambda: nn.Sequential(nn.Linear(17, 400), nn.ReLU(), nn.Linear(400, 6)),
    "another head": lambda: nn.Sequential(nn.Linear(17, 400), nn.ReLU(), nn.Linear(400, 6),
                                           pfrl_amd.policies.GaussianHeadWithFixedCovariance()),
    "not a Sequential": lambda: nn.Linear(17, 6),
}


@pytest.mark.parametrize("name", sorted(DETERMINISTIC_MISSES))
def test_deterministic_policy_near_misses(name):
    assert ps.deterministic_policy(DETERMINISTIC_MISSES[name]()) is None


def _head(x):
    raise AssertionError("the head function is only ever probed by recognise_head")


def _sac_example_policy(obs=17, A=6, last=None):
    """examples/mujoco/reproduction/soft_actor_critic/train_soft_actor_critic.py:172-179"""
    return nn.Sequential(nn.Linear(obs, 256), nn.ReLU(), nn.Linear(256, 256), nn.ReLU(),
                         last if last is not None else nn.Linear(256, 2 * A), pfrl_amd.nn.Lambda(_head))


def _accepting(calls):
    def recognise_head(fn, width, device):
        calls.append((fn, width, device))
        return sg.HeadSpec(-20.0, 2.0, 0, width // 2, True)
    return recognise_head


def test_squashed_gaussian_policy_recognised(monkeypatch):
    calls = []
    monkeypatch.setattr(sg, "recognise_head", _accepting(calls))
    pol = _sac_example_policy()
    split = ps.squashed_gaussian_policy(pol, "cuda:0")
    assert calls == [(_head, 12, "cuda:0")]
    assert split is not None and split.layer is pol[4] and split.spec.A == 6
    assert (split.spec.lo, split.spec.hi, split.spec.mode) == (-20.0, 2.0, 0)
    assert [id(m) for m in split.body.children()] == [id(m) for m in list(pol.children())[:4]]
    x = torch.randn(3, 17)
    with torch.no_grad():
        assert torch.equal(split.body(x), pol[3](pol[2](pol[1](pol[0](x)))))
    # what the agent's own probe found is taken as it is: no second probe
    mine = sg.HeadSpec(-5.0, 1.0, 1, 6, False)
    assert ps.squashed_gaussian_policy(pol, "cuda:0", spec=mine).spec is mine
    assert len(calls) == 1
    # ... unless it describes another width
    assert ps.squashed_gaussian_policy(pol, "cuda:0", spec=sg.HeadSpec(-5.0, 1.0, 1, 5, False)) is None
    assert ps.squashed_gaussian_policy(_sac_example_policy(A=32), "cuda:0") is not None


SQUASHED_MISSES = {
    "no bias": lambda: _sac_example_policy(last=nn.Linear(256, 12, bias=False)),
    "float64 layer": lambda: _sac_example_policy(last=nn.Linear(256, 12).double()),
    "A = 33": lambda: _sac_example_policy(A=33),
    "odd width": lambda: _sac_example_policy(last=nn.Linear(256, 13)),
    "K = 1025": lambda: nn.Sequential(nn.Linear(4, 1025), nn.ReLU(), nn.Linear(1025, 4),
                                       pfrl_amd.nn.Lambda(_head)),
    "empty body": lambda: nn.Sequential(nn.Linear(17, 12), pfrl_amd.nn.Lambda(_head)),
    "no Lambda": lambda: nn.Sequential(nn.Linear(17, 256), nn.ReLU(), nn.Linear(256, 12), nn.Tanh()),
    "not a Sequential": lambda: nn.Linear(17, 12),
}


@pytest.mark.parametrize("name", sorted(SQUASHED_MISSES))
def test_squashed_gaussian_policy_near_misses(monkeypatch, name):
    calls = []
    monkeypatch.setattr(sg, "recognise_head", _accepting(calls))
    assert ps.squashed_gaussian_policy(SQUASHED_MISSES[name](), "cuda:0") is None
    assert calls == []                                  # refused before any probe


def test_squashed_gaussian_policy_with_a_rejected_head(monkeypatch):
    monkeypatch.setattr(sg, "recognise_head", lambda fn, width, device: None)
    assert ps.squashed_gaussian_policy(_sac_example_policy(), "cuda:0") is None
