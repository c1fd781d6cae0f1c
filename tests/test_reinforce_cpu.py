"""REINFORCE, the part that needs no GPU: the constructor against the reference's recorded signature,
the host route against a trace of the reference (tests/golden/make_reinforce_fixtures.py), the returns
helper against the reference's expression, and the closed forms pfrl_reinforce_loss /
pfrl_reinforce_gaussian_loss implement against autograd through torch.distributions in float64.
The scripted env, the models and the loop that the recorder and the device tests
(tests/test_reinforce.py) share live here."""
import json
import os
import warnings

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
OBS, HIDDEN, UPDATES = 5, 16, 6
EPISODE_LENGTHS = (1, 7, 12)
HYPER = dict(beta=0.01, max_grad_norm=1.0)
LR = 1e-2
# prefix -> (head, batchsize, backward_separately, integer rewards)
CONFIGS = {
    "sm_b1_": ("softmax", 1, False, False),
    "sm_b3_": ("softmax", 3, True, True),
    "ga_b1_": ("gaussian", 1, False, False),
    "ga_b3_": ("gaussian", 3, True, False),
}
N_ACTIONS = {"softmax": 3, "gaussian": 2}
NEW_ENTRY_POINTS = ("pfrl_reinforce_loss", "pfrl_reinforce_gaussian_loss")


def _exp2(x):
    return torch.exp(2 * x)


class ScriptedEnv:
    """Observations of ``OBS`` float32 numbers from a seeded generator; episodes end after 1, 7 and 12
    steps in turn, whatever the actions; rewards alternate between two Python floats scaled by the
    step (or two Python ints)."""

    def __init__(self, seed=5, int_rewards=False):
        self.rng = np.random.RandomState(seed)
        self.int_rewards = int_rewards
        self.episode = -1
        self.t = 0          # steps of all episodes

    def _obs(self):
        return self.rng.uniform(-1, 1, OBS).astype(np.float32)

    def reset(self):
        self.episode += 1
        self.left = EPISODE_LENGTHS[self.episode % len(EPISODE_LENGTHS)]
        return self._obs()

    def step(self, action):
        t = self.t
        self.t += 1
        self.left -= 1
        if self.int_rewards:
            reward = (2, -1)[t % 2] * (1 + t % 3)
            assert type(reward) is int
        else:
            reward = (1.5, -0.75)[t % 2] * (1 + t % 3)
            assert type(reward) is float
        return self._obs(), reward, self.left == 0, {}


def make_model(pkg, head):
    """The fixture's policy: a 16-unit tanh network on 5-number observations (``pkg``: the package
    that supplies the head -- the reference for the recorder, pfrl_amd for the tests)."""
    nn = torch.nn
    if head == "softmax":
        last = pkg.policies.SoftmaxCategoricalHead()
    else:
        last = pkg.policies.GaussianHeadWithStateIndependentCovariance(
            action_size=N_ACTIONS[head], var_type="diagonal", var_func=_exp2, var_param_init=0)
    return nn.Sequential(nn.Linear(OBS, HIDDEN), nn.Tanh(), nn.Linear(HIDDEN, N_ACTIONS[head]), last)


def make_agent(pkg, prefix, model, gpu=None, **kw):
    _, batchsize, separately, _ = CONFIGS[prefix]
    return pkg.agents.REINFORCE(model, torch.optim.Adam(model.parameters(), lr=LR), gpu=gpu,
                                batchsize=batchsize, backward_separately=separately, **HYPER, **kw)


def run_loop(ag, prefix, updates=UPDATES, seed=8642):
    """The fixture's loop: act / observe on the scripted env until ``updates`` optimizer steps have
    been taken.  Returns (actions of every step, the parameters after every update)."""
    env = ScriptedEnv(int_rewards=CONFIGS[prefix][3])
    torch.manual_seed(seed)
    steps = [0]
    after = []
    orig_step = ag.optimizer.step

    def counting_step(*a, **k):
        out = orig_step(*a, **k)
        steps[0] += 1
        after.append(_flat(ag.model.parameters()))
        return out

    ag.optimizer.step = counting_step
    actions = []
    obs = env.reset()
    while steps[0] < updates:
        a = ag.act(obs)
        actions.append(np.asarray(a).copy())
        obs, r, done, _ = env.step(a)
        ag.observe(obs, r, done, False)
        if done:
            obs = env.reset()
    ag.optimizer.step = orig_step
    return np.asarray(actions), after


def _trace():
    return np.load(os.path.join(GOLDEN, "agent_trace_reinforce.npz"))


def update_of(g, prefix, k):
    """Update ``k`` of one configuration of the fixture: parameters before / after, gradient before
    clipping, and its rows, actions, returns (float64), rows per accumulate_grad call and their
    losses."""
    calls = g[prefix + "update_calls"]
    c0, c1 = int(calls[:k].sum()), int(calls[:k + 1].sum())
    call_rows = g[prefix + "call_rows"]
    r0, r1 = int(call_rows[:c0].sum()), int(call_rows[:c1].sum())
    return dict(params_before=g[prefix + "params_before"][k], grad=g[prefix + "grad"][k],
                params_after=g[prefix + "params_after"][k], rows=g[prefix + "rows"][r0:r1],
                actions=g[prefix + "actions"][r0:r1], returns=g[prefix + "returns"][r0:r1],
                call_rows=call_rows[c0:c1], loss=g[prefix + "loss"][c0:c1])


def _load_flat(tensors, flat):
    off = 0
    with torch.no_grad():
        for p in tensors:
            n = p.numel()
            p.copy_(torch.as_tensor(flat[off:off + n]).view_as(p))
            off += n
    assert off == len(flat)


def _flat(tensors):
    return np.concatenate([p.detach().cpu().numpy().ravel() for p in tensors])


def _flat_grads(tensors):
    return np.concatenate([p.grad.detach().cpu().numpy().ravel() for p in tensors])


def fixture_agent(g, prefix, gpu=None, **kw):
    """The fixture's agent of one configuration, its model at the recorded initial parameters."""
    import pfrl_amd as pfrl

    model = make_model(pfrl, CONFIGS[prefix][0])
    _load_flat(model.parameters(), g[prefix + "init_params"])
    return make_agent(pfrl, prefix, model, gpu=gpu, **kw)


def test_library_exports_the_reinforce_entry_points():
    from pfrl_amd import _native

    if not _native.available():
        _native.build()
    lib = _native.lib()
    for name in NEW_ENTRY_POINTS:
        assert name in _native.EXPORTS, name
        assert hasattr(lib, name), "library does not export %s" % name


def test_reinforce_signature_is_the_references():
    """Parameter for parameter -- names, order, kinds, literal defaults -- then this package's
    keyword-only switch with a default; the methods and ``saved_attributes`` too."""
    from _api_surface import describe_signature
    from pfrl_amd import agents

    want = json.load(open(os.path.join(GOLDEN, "api_signatures_reinforce.json")))
    got = describe_signature(agents.REINFORCE)
    ref = want["agents.REINFORCE"]
    assert got[:len(ref)] == ref
    assert got[len(ref):] == [["recompute_forward", "KEYWORD_ONLY", "True"]]
    for key, sig in want.items():
        parts = key.split(".")
        if len(parts) == 3 and parts[2] != "saved_attributes":
            assert describe_signature(getattr(agents.REINFORCE, parts[2])) == sig, key
    assert list(agents.REINFORCE.saved_attributes) == want["agents.REINFORCE.saved_attributes"]
    for name in ("accumulate_grad", "batch_update", "update_with_accumulated_grad"):
        assert callable(getattr(agents.REINFORCE, name))
    ag = fixture_agent(_trace(), "sm_b1_")
    assert [name for name, _ in ag.get_statistics()] == ["average_entropy"]


def _pinned_environment(g):
    """The settings the fixture was recorded under (stored in it): one CPU code path of torch and of
    its BLAS / vector-math library on every processor, one thread."""
    return dict(zip([str(k) for k in g["pinned_env_names"]], [str(v) for v in g["pinned_env_values"]]))


def _record_host_traces(path):
    """Child process: the host route on the fixture's four configurations, written to ``path``."""
    g = _trace()
    for name, value in _pinned_environment(g).items():
        assert os.environ.get(name) == value, name
    assert torch.backends.cpu.get_cpu_capability() == "DEFAULT" and torch.get_num_threads() == 1
    out = {}
    for prefix in CONFIGS:
        ag = fixture_agent(g, prefix)
        assert not ag.device_route
        actions, after = run_loop(ag, prefix)
        out[prefix + "actions"] = actions
        out[prefix + "params_after"] = np.stack(after)
        out[prefix + "average_entropy"] = np.asarray(ag.average_entropy)
    np.savez(path, **out)


@pytest.fixture(scope="module")
def host_traces(tmp_path_factory):
    """All configurations in ONE fresh interpreter under the fixture's pinned settings (which vector
    code torch's CPU kernels and its math library run is chosen per processor when the process
    starts; "bit for bit" is only defined on one code path)."""
    import subprocess
    import sys

    path = str(tmp_path_factory.mktemp("reinforce") / "host_traces.npz")
    env = dict(os.environ)
    env.update(_pinned_environment(_trace()))
    subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, check=True, timeout=600)
    return np.load(path)


@pytest.mark.parametrize("prefix", sorted(CONFIGS))
def test_host_route_follows_the_reference_trace(host_traces, prefix):
    """gpu=None: the reference's algorithm statement for statement, so under the pinned settings every
    action, the parameters after each of the six updates and ``average_entropy`` equal the
    reference's bit for bit.

    Measured: on the recording machine (Intel Xeon) every figure of all four configurations is
    bit-equal.  On an AMD EPYC host, under the same pinned settings, ``ga_b1_`` is bit-equal through
    the first update (the one-step episode) and then is not: parameters after updates 2..6 differ by
    7.5e-9, 3.0e-8, 3.0e-8, 3.0e-8 (one unit in the last place; the fixture's ``param_tol`` is
    1.6e-7) and 8 of the 80 action components by at most 6.0e-8, so the equalities below fail there
    for the Gaussian configurations.  As for TRPO's host trace (tests/test_trpo_cpu.py), some CPU
    kernel behind the Gaussian head still depends on the processor with these settings, and which
    one is not found yet.  The equalities stay as the criterion."""
    g, got = _trace(), host_traces
    want_actions = g[prefix + "actions"]
    print(prefix, "actions differing:", int((got[prefix + "actions"] != want_actions).sum()),
          "of", want_actions.size)
    key = prefix + "params_after"
    assert got[key].shape == g[key].shape and len(g[key]) == UPDATES
    print(prefix, "max parameter difference per update", np.abs(got[key] - g[key]).max(1))
    np.testing.assert_array_equal(got[prefix + "actions"], want_actions)
    np.testing.assert_array_equal(got[key], g[key])
    assert float(got[prefix + "average_entropy"]) == float(g[prefix + "average_entropy"])


def test_fixture_covers_what_it_is_meant_to():
    """Four configurations, six updates each; the first update of the ``batchsize=1`` runs is the
    one-step episode; one run has integer rewards (an int64 returns column); measured tolerances."""
    g = _trace()
    for prefix, (head, batchsize, separately, ints) in CONFIGS.items():
        steps = 0
        for k in range(UPDATES):
            u = update_of(g, prefix, k)
            calls = u["call_rows"]
            assert len(calls) == (batchsize if separately else 1) and len(u["loss"]) == len(calls)
            M = int(calls.sum())
            steps += M
            assert u["rows"].shape == (M, OBS) and len(u["returns"]) == M
            assert u["actions"].shape == ((M,) if head == "softmax" else (M, 2))
        assert steps == len(g[prefix + "actions"]) == len(g[prefix + "rows"])
        assert int(update_of(g, prefix, 0)["call_rows"][0]) == 1
        assert np.array_equal(g[prefix + "params_before"][0], g[prefix + "init_params"])
        assert bool(g[prefix + "int_rewards"]) == ints
        assert 0 < float(g[prefix + "grad_tol"]) < 1e-4 and 0 < float(g[prefix + "param_tol"]) < 1e-4
    assert sum(bool(g[p + "int_rewards"]) for p in CONFIGS) == 1


def test_returns_helper_is_the_references_expression():
    """Float, int and single-step episodes: values and dtype of
    ``np.cumsum(list(reversed(r_seq[1:])))[::-1]`` (the first reward dropped, the last twice)."""
    from pfrl_amd.agents.reinforce import returns_of

    for r_seq in ([0.5, -1.25, 3.0, 0.1, 0.1], [1, 2, -3, 4, 4], [2.5, 2.5], [7, 7],
                  [1, 2.5, 3, 3]):
        want = np.cumsum(list(reversed(r_seq[1:])))[::-1]
        got = returns_of(r_seq)
        assert got.dtype == want.dtype and len(got) == len(r_seq) - 1
        np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(returns_of([1, 2, -3, 4, 4]), [7, 5, 8, 4])
    assert returns_of([1, 2, -3, 4, 4]).dtype == np.int64
    np.testing.assert_array_equal(returns_of([2.5, 2.5]), [2.5])


def test_closed_form_softmax_gradient_equals_autograd_through_the_distribution():
    """float64 on the CPU, 1e-12: out2 and d total / d logits of pfrl_reinforce_loss's formulas."""
    from pfrl_amd import ops

    torch.manual_seed(31)
    M, A, beta, inv_b = 97, 7, 0.03, 1.0 / 3
    dt = torch.float64
    logits = (2 * torch.randn(M, A, dtype=dt)).requires_grad_(True)
    action = torch.randint(0, A, (M,))
    ret = 3 * torch.randn(M, dtype=dt)
    dist = torch.distributions.Categorical(logits=logits)
    total = (-ret * dist.log_prob(action) - beta * dist.entropy()).sum() * inv_b
    total.backward()
    out2, dlogits = ops.reinforce_loss_closed_form(logits.detach(), action, ret, inv_b, beta)
    want2 = torch.stack([total.detach(), dist.entropy().mean().detach()])
    np.testing.assert_allclose(out2.numpy(), want2.numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(dlogits.numpy(), logits.grad.numpy(), rtol=1e-12, atol=1e-12)


def test_closed_form_gaussian_gradient_equals_autograd_through_the_distribution():
    """float64 on the CPU, 1e-12: out2, d total / d mean and d total / d scale (the entropy term's
    -beta M inv_batchsize / scale_j included) of pfrl_reinforce_gaussian_loss's formulas."""
    from pfrl_amd import ops

    torch.manual_seed(32)
    M, A, beta, inv_b = 97, 5, 0.03, 1.0 / 3
    dt = torch.float64
    mean = torch.randn(M, A, dtype=dt, requires_grad=True)
    scale = torch.exp(0.3 * torch.randn(A, dtype=dt)).requires_grad_(True)
    dist = torch.distributions.Independent(torch.distributions.Normal(mean, scale.expand_as(mean)), 1)
    action = dist.sample()
    ret = 3 * torch.randn(M, dtype=dt)
    total = (-ret * dist.log_prob(action) - beta * dist.entropy()).sum() * inv_b
    total.backward()
    out2, dmean, dscale = ops.reinforce_gaussian_loss_closed_form(mean.detach(), scale.detach(), action,
                                                                  ret, inv_b, beta)
    want2 = torch.stack([total.detach(), dist.entropy().mean().detach()])
    np.testing.assert_allclose(out2.numpy(), want2.numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(dmean.numpy(), mean.grad.numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(dscale.numpy(), scale.grad.numpy(), rtol=1e-12, atol=1e-12)


def test_reset_without_done_discards_the_episode_and_warns():
    """Reference :133-141: the rewards and graphs of the interrupted episode are dropped, nothing is
    learned from it, and the next finished episode updates from its own steps alone."""
    ag = fixture_agent(_trace(), "sm_b1_")
    before = _flat(ag.model.parameters())
    env = ScriptedEnv()
    obs = env.reset()
    for t in range(3):
        obs = env.step(ag.act(obs))[0]
        if t < 2:
            ag.observe(obs, 0.5, False, False)
    assert len(ag.log_prob_sequences[0]) == 3 and ag.reward_sequences == [[0.5, 0.5]]
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        ag.observe(obs, 1.0, False, True)
    assert any("throw away the last episode" in str(w.message) for w in caught)
    assert ag.reward_sequences == [[]] and ag.log_prob_sequences == [[]] and ag.entropy_sequences == [[]]
    assert ag.n_backward == 0 and np.array_equal(_flat(ag.model.parameters()), before)
    ag.act(obs)
    ag.observe(obs, 2.0, True, False)
    assert ag.reward_sequences == [[]] and not np.array_equal(_flat(ag.model.parameters()), before)


def test_recurrent_model_takes_the_host_route():
    """``recurrent=True`` keeps the reference's per-step graphs and ``one_step_forward`` whatever the
    other switches say; one two-step episode moves the parameters."""
    import pfrl_amd as pfrl

    torch.manual_seed(3)
    nn = torch.nn
    model = pfrl.nn.RecurrentSequential(nn.LSTM(num_layers=1, input_size=OBS, hidden_size=8),
                                        nn.Linear(8, 3), pfrl.policies.SoftmaxCategoricalHead())
    ag = pfrl.agents.REINFORCE(model, torch.optim.Adam(model.parameters(), lr=LR), gpu=-1,
                               recurrent=True, recompute_forward=True, beta=0.01)
    assert not ag.device_route
    before = _flat(model.parameters())
    env = ScriptedEnv()
    env.reset()
    obs = env.reset()                  # (the second episode: seven steps)
    for t in range(2):
        a = ag.act(obs)
        assert ag.train_recurrent_states is not None
        obs = env.step(a)[0]
        ag.observe(obs, 1.0, t == 1, False)
    assert ag.train_recurrent_states is None
    assert len(ag.log_prob_sequences) == 1 and ag.log_prob_sequences[0] == []
    assert not np.array_equal(_flat(model.parameters()), before)


if __name__ == "__main__":      # the child of the ``host_traces`` fixture
    import sys

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    _record_host_traces(sys.argv[1])
