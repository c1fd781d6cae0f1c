"""TRPO, the part that needs no GPU: the constructor against the reference's recorded signature, the
host route against a trace of the reference (tests/golden/make_trpo_fixtures.py), and the closed
forms pfrl_trpo_gaussian_eval implements against autograd through torch.distributions in float64.
The helpers the device tests share (tests/test_trpo.py) live here."""
import json
import os
import random

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
OBS, ACT, N, UPDATE_INTERVAL, UPDATES = 5, 2, 4, 64, 2
NEW_ENTRY_POINTS = ("pfrl_trpo_gaussian_eval", "pfrl_cg_init", "pfrl_cg_step", "pfrl_cg_workgroup_reach",
                    "pfrl_trpo_scale_step", "pfrl_params_axpy")
SWITCHES = ("fused_gaussian_eval", "device_cg", "fused_param_step", "capture_vf_step")


def _exp2(x):
    return torch.exp(2 * x)


def _trace():
    return np.load(os.path.join(GOLDEN, "agent_trace_trpo.npz"))


def _hyper(g):
    h = dict(zip([str(k) for k in g["hyper_names"]], [float(v) for v in g["hyper_values"]]))
    for k in ("update_interval", "vf_epochs", "vf_batch_size"):
        h[k] = int(h[k])
    return h


def _models(obs=OBS, act=ACT, hidden=16):
    import pfrl_amd as pfrl

    nn = torch.nn
    policy = nn.Sequential(
        nn.Linear(obs, hidden), nn.Tanh(), nn.Linear(hidden, act),
        pfrl.policies.GaussianHeadWithStateIndependentCovariance(
            action_size=act, var_type="diagonal", var_func=_exp2, var_param_init=0))
    vf = nn.Sequential(nn.Linear(obs, hidden), nn.Tanh(), nn.Linear(hidden, 1))
    return policy, vf


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


def _agent(g, prefix, gpu, **kw):
    """The fixture's agent (its models at their recorded initial parameters)."""
    import pfrl_amd as pfrl
    from pfrl_amd import agents

    policy, vf = _models()
    _load_flat(policy.parameters(), g[prefix + "init_policy"])
    _load_flat(vf.parameters(), g[prefix + "init_vf"])
    norm = pfrl.nn.EmpiricalNormalization(OBS, clip_threshold=5) if prefix == "norm_" else None
    args = _hyper(g)
    args.update(kw)
    return agents.TRPO(policy, vf, torch.optim.Adam(vf.parameters(), lr=1e-2), obs_normalizer=norm,
                       gpu=gpu, **args)


def _run_trace(ag, steps, n_env=N, seed=5, after_update=None):
    """The fixture's loop; returns the actions and, per update, (step size, KL, policy, vf).
    ``after_update(k, agent)`` runs after update ``k`` has been recorded."""
    import pfrl_amd as pfrl
    from pfrl_amd.envs.synthetic import HostSyntheticVectorObsEnv

    pfrl.utils.set_random_seed(0)
    torch.manual_seed(8642)
    random.seed(11)
    env = HostSyntheticVectorObsEnv(n_env, obs_dim=OBS, act_dim=ACT, seed=seed, p_done=0.05)
    actions, updates = [], []
    obs = env.reset()
    for _ in range(steps):
        a = ag.batch_act(obs)
        actions.append(np.asarray(a).copy())
        obs, r, done, _ = env.step(a)
        seen = len(ag.policy_step_size_record)
        ag.batch_observe(obs, r, done, [False] * n_env)
        if len(ag.policy_step_size_record) > seen:
            updates.append((ag.policy_step_size_record[-1], ag.kl_record[-1] if ag.kl_record else None,
                            _flat(ag.policy.parameters()), _flat(ag.vf.parameters())))
            if after_update is not None:
                after_update(len(updates) - 1, ag)
        obs = env.reset(~done)
    return np.asarray(actions), updates


def test_library_exports_the_trpo_entry_points():
    from pfrl_amd import _native

    if not _native.available():
        _native.build()
    lib = _native.lib()
    for name in NEW_ENTRY_POINTS:
        assert name in _native.EXPORTS, name
        assert hasattr(lib, name), "library does not export %s" % name
    assert lib.pfrl_cg_workgroup_reach() >= 4096


def test_trpo_signature_is_the_references():
    """Parameter for parameter -- names, order, kinds, literal defaults -- then this package's
    keyword switches, each with a default; the methods and ``saved_attributes`` too."""
    from _api_surface import describe_signature
    from pfrl_amd import agents

    want = json.load(open(os.path.join(GOLDEN, "api_signatures_trpo.json")))
    got = describe_signature(agents.TRPO)
    ref = want["agents.TRPO"]
    assert got[:len(ref)] == ref
    extra = got[len(ref):]
    assert [e[0] for e in extra][:len(SWITCHES)] == list(SWITCHES)
    assert all(e[2] != "<required>" for e in extra)
    for key, sig in want.items():
        parts = key.split(".")
        if len(parts) == 3 and parts[2] != "saved_attributes":
            assert describe_signature(getattr(agents.TRPO, parts[2])) == sig, key
    assert list(agents.TRPO.saved_attributes) == want["agents.TRPO.saved_attributes"]
    names = [name for name, _ in _agent(_trace(), "plain_", None).get_statistics()]
    assert names == ["average_value", "average_entropy", "average_kl", "average_policy_step_size",
                     "explained_variance"]


def _pinned_environment(g):
    """The settings the fixture was recorded under (stored in it): one CPU code path of torch and of
    its BLAS / vector-math library on every processor, one thread."""
    return dict(zip([str(k) for k in g["pinned_env_names"]], [str(v) for v in g["pinned_env_values"]]))


def _record_host_traces(path):
    """Child process: the host route on the fixture's two configurations, written to ``path``."""
    g = _trace()
    for name, value in _pinned_environment(g).items():
        assert os.environ.get(name) == value, name
    assert torch.backends.cpu.get_cpu_capability() == "DEFAULT" and torch.get_num_threads() == 1
    out = {}
    for prefix in ("plain_", "norm_"):
        ag = _agent(g, prefix, None)
        actions, updates = _run_trace(ag, UPDATES * UPDATE_INTERVAL // N)
        assert len(updates) == UPDATES
        out[prefix + "actions"] = actions
        for k, (step, kl, policy, vf) in enumerate(updates):
            key = "%su%d_" % (prefix, k)
            out[key + "step_size"], out[key + "kl"] = np.asarray(step), np.asarray(kl)
            out[key + "policy_after"], out[key + "vf_after"] = policy, vf
        stats = dict(ag.get_statistics())
        out[prefix + "average_kl"] = np.asarray(stats["average_kl"])
        out[prefix + "average_policy_step_size"] = np.asarray(stats["average_policy_step_size"])
    np.savez(path, **out)


@pytest.fixture(scope="module")
def host_traces(tmp_path_factory):
    """Both configurations in ONE fresh interpreter under the fixture's pinned settings.  Which
    vector code torch's CPU kernels and its math library run is chosen per processor when the
    process starts (the library's tanh alone moves 1 unit in the last place in 2 of 128 actions
    between two processors), and "bit for bit" is only defined on one code path: the settings select
    the portable one, for the recording of the reference and for this run alike."""
    import subprocess
    import sys

    path = str(tmp_path_factory.mktemp("trpo") / "host_traces.npz")
    env = dict(os.environ)
    env.update(_pinned_environment(_trace()))
    subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, check=True, timeout=600)
    return np.load(path)


@pytest.mark.parametrize("prefix", ["plain_", "norm_"])
def test_host_route_follows_the_reference_trace(host_traces, prefix):
    """gpu=None: the reference's algorithm.  Before the first update the draws are the same torch CPU
    generator's and the parameters the same, so the actions equal the reference's bit for bit.  After
    each update the accepted step size and the KL equal the reference's, and so do ``average_kl`` and
    ``average_policy_step_size``; the policy / value-function parameters agree within the fixture's
    measured tolerance (ten times the reference's own float32 - float64 difference).

    Measured: on the recording machine (Intel Xeon, AVX-512) every figure is bit-equal.  On an AMD EPYC
    9575F, under the same pinned settings, the actions (0 of 128 differ), the step sizes and the policy
    after the first update are bit-equal too, but the float32 KL of the accepted trial is not
    (plain: 0.005932393483817577 against 0.005932400934398174; second update 0.007510151714086533
    against 0.007510174997150898; norm: first update equal, second 0.007570919115096331 against
    0.007570911198854446; value function 1.5e-8 to 6e-8 off, policy after the second update 7e-7 to
    2.2e-6, tolerance 7.8e-6 / 8.7e-6), so the KL equalities below fail there: some CPU kernel behind
    the 256-row evaluation or NumPy's norm still depends on the processor with these settings, and
    which one is not found yet.  The equalities stay as the criterion."""
    g, got = _trace(), host_traces
    first = UPDATE_INTERVAL // N
    want_actions = g[prefix + "actions"]
    print(prefix, "actions differing before the first update:",
          int((got[prefix + "actions"][:first] != want_actions[:first]).sum()), "of", want_actions[:first].size)
    tol = float(g[prefix + "param_tol"])
    for k in range(UPDATES):
        key = "%su%d_" % (prefix, k)
        print(key, "step", float(got[key + "step_size"]), float(g[key + "step_size"]),
              "kl", repr(float(got[key + "kl"])), repr(float(g[key + "kl"])),
              "max policy diff", np.abs(got[key + "policy_after"] - g[key + "policy_after"]).max(),
              "max vf diff", np.abs(got[key + "vf_after"] - g[key + "vf_after"]).max(), "tol", tol)
    print(prefix, "average_kl", repr(float(got[prefix + "average_kl"])), repr(float(g[prefix + "average_kl"])))
    np.testing.assert_array_equal(got[prefix + "actions"][:first], want_actions[:first])
    assert 0 < tol < 1e-4
    for k in range(UPDATES):
        key = "%su%d_" % (prefix, k)
        assert float(got[key + "step_size"]) == float(g[key + "step_size"])
        assert float(got[key + "kl"]) == float(g[key + "kl"])
        np.testing.assert_allclose(got[key + "policy_after"], g[key + "policy_after"], rtol=0, atol=tol)
        np.testing.assert_allclose(got[key + "vf_after"], g[key + "vf_after"], rtol=0, atol=tol)
    assert float(got[prefix + "average_policy_step_size"]) == float(g[prefix + "average_policy_step_size"])
    assert float(got[prefix + "average_kl"]) == float(g[prefix + "average_kl"])


def _distribution(mean, scale):
    return torch.distributions.Independent(torch.distributions.Normal(mean, scale.expand_as(mean)), 1)


def test_closed_form_gain_gradient_equals_autograd_through_the_distribution():
    """float64 on the CPU, 1e-12: out3 and the gradient of the gain with respect to mean and scale."""
    from pfrl_amd import ops

    torch.manual_seed(21)
    M, A, coef = 96, 5, 0.03
    dt = torch.float64
    mean = torch.randn(M, A, dtype=dt, requires_grad=True)
    scale = torch.exp(0.3 * torch.randn(A, dtype=dt)).requires_grad_(True)
    mean_old = (mean + 0.1 * torch.randn(M, A, dtype=dt)).detach()
    scale_old = (scale * torch.exp(0.1 * torch.randn(A, dtype=dt))).detach()
    old = _distribution(mean_old, scale_old)
    action = old.sample()
    log_prob_old = old.log_prob(action)
    adv = torch.randn(M, dtype=dt)
    new = _distribution(mean, scale)
    gain = torch.mean(torch.exp(new.log_prob(action) - log_prob_old) * adv) + coef * new.entropy().mean()
    kl = torch.distributions.kl_divergence(old, new).mean()
    gain.backward()
    out3, dmean, dscale = ops.trpo_gaussian_eval_closed_form(
        mean.detach(), scale.detach(), mean_old, scale_old, action, adv, log_prob_old, coef)
    want3 = torch.stack([gain.detach(), kl.detach(), new.entropy().mean().detach()])
    np.testing.assert_allclose(out3.numpy(), want3.numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(dmean.numpy(), mean.grad.numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(dscale.numpy(), scale.grad.numpy(), rtol=1e-12, atol=1e-12)


def test_fisher_metric_of_the_gaussian_is_the_hessian_of_the_kl():
    """At old = new the Hessian of KL(old || new) with respect to (mean_j, log scale_j) is
    diag(1 / s_j^2, 2): in (mean, scale) coordinates diag(1 / s^2, 2 / s^2), the metric a fused
    Fisher-vector product would apply per row (float64, autograd, 1e-10)."""
    torch.manual_seed(22)
    A = 4
    dt = torch.float64
    m0 = torch.randn(A, dtype=dt)
    s0 = torch.exp(0.4 * torch.randn(A, dtype=dt))

    def kl(theta):
        new = torch.distributions.Normal(theta[:A], theta[A:])
        return torch.distributions.kl_divergence(torch.distributions.Normal(m0, s0), new).sum()

    H = torch.autograd.functional.hessian(kl, torch.cat([m0, s0]))
    want = torch.diag(torch.cat([1 / s0 ** 2, 2 / s0 ** 2]))
    np.testing.assert_allclose(H.numpy(), want.numpy(), rtol=1e-10, atol=1e-10)


def test_recurrent_policy_takes_the_host_route_and_steps_inside_the_trust_region():
    """``recurrent=True``: the list-of-dicts rollout and the reference's sequence update.  One update
    of 32 transitions: the accepted step size is a power of one half with a KL inside ``max_kl`` and
    moved parameters, or 0 with the parameters restored bit for bit; the value function was fitted
    either way."""
    import pfrl_amd as pfrl
    from pfrl_amd import agents

    torch.manual_seed(3)
    nn = torch.nn
    pi = pfrl.nn.RecurrentSequential(
        nn.LSTM(num_layers=1, input_size=OBS, hidden_size=8), nn.Linear(8, ACT),
        pfrl.policies.GaussianHeadWithStateIndependentCovariance(
            action_size=ACT, var_type="diagonal", var_func=_exp2, var_param_init=0))
    v = pfrl.nn.RecurrentSequential(nn.LSTM(num_layers=1, input_size=OBS, hidden_size=8),
                                    nn.Linear(8, 1))
    ag = agents.TRPO(pi, v, torch.optim.Adam(v.parameters(), lr=1e-2), gpu=-1, recurrent=True,
                     update_interval=32, vf_batch_size=16, max_grad_norm=1.0)
    assert ag._host is not None and ag.rollout is None
    assert isinstance(ag.model, pfrl.nn.RecurrentBranched)
    before, vf_before = _flat(pi.parameters()), _flat(v.parameters())
    _, updates = _run_trace(ag, 8)
    assert len(updates) == 1 and ag.n_updates == 1
    step, kl, after, vf_after = updates[0]
    assert np.isfinite(after).all() and np.isfinite(vf_after).all()
    assert step in [0.0] + [0.5 ** i for i in range(ag.line_search_max_backtrack + 1)]
    if step == 0.0:
        assert np.array_equal(after, before) and len(ag.kl_record) == 0
    else:
        assert not np.array_equal(after, before)
        assert 0.0 <= kl <= ag.max_kl
    assert not np.array_equal(vf_after, vf_before)


if __name__ == "__main__":      # the child of the ``host_traces`` fixture
    import sys

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    _record_host_traces(sys.argv[1])
