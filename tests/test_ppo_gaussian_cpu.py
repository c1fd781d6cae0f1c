"""Gaussian-policy PPO on the device path, the part that needs no GPU: the three entry points are
exported, the closed-form gradients pfrl_ppo_gaussian_loss implements equal autograd through
``Independent(Normal)`` + ``PPO._lossfun`` in float64, ``_ActGraph._gaussian_split`` recognises
the two model shapes in use and nothing else, and one update on the reference's own recorded state
through the host path (its device twin, and the helpers both share, live here / in
test_ppo_gaussian.py)."""
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
OBS, ACT = 17, 6
NEW_ENTRY_POINTS = ("pfrl_ppo_gaussian_act", "pfrl_ppo_gaussian_loss", "pfrl_ppo_minibatch_f32act")


def test_library_exports_the_gaussian_ppo_entry_points():
    from pfrl_amd import _native

    if not _native.available():
        _native.build()
    lib = _native.lib()
    for name in NEW_ENTRY_POINTS:
        assert name in _native.EXPORTS, name
        assert hasattr(lib, name), "library does not export %s" % name


def _exp2(x):
    return torch.exp(2 * x)


def _cpu_agent(model, **kw):
    from pfrl_amd import agents

    opt = torch.optim.Adam(model.parameters(), lr=3e-4, eps=1e-5)
    return agents.PPO(model, opt, gpu=None, update_interval=64, minibatch_size=16, epochs=1, **kw)


@pytest.mark.parametrize("clip_eps_vf", [None, 0.15])
@pytest.mark.parametrize("var_type", ["spherical", "diagonal"])
def test_closed_form_gradients_equal_autograd_through_the_distribution(var_type, clip_eps_vf):
    """float64 on the CPU, 1e-12: out4 and the gradients with respect to mean, value and the scale
    vector (for a spherical variance: the sum over the expanded entries)."""
    import pfrl_amd as pfrl
    from pfrl_amd import ops

    torch.manual_seed(11 if var_type == "spherical" else 12)
    M, A = 96, 5
    dt = torch.float64
    head = pfrl.policies.GaussianHeadWithStateIndependentCovariance(
        action_size=A, var_type=var_type, var_func=_exp2, var_param_init=0).to(dt)
    with torch.no_grad():
        head.var_param.copy_(0.3 * torch.randn_like(head.var_param))
    ag = _cpu_agent(torch.nn.Sequential(torch.nn.Linear(3, A), head), clip_eps=0.2,
                    clip_eps_vf=clip_eps_vf, value_func_coef=0.7, entropy_coef=0.03)
    mean = torch.randn(M, A, dtype=dt, requires_grad=True)
    value = torch.randn(M, 1, dtype=dt, requires_grad=True)
    distrib = head(mean)
    scale = distrib.base_dist.scale          # [M, A], a broadcast of the scale vector
    action = (mean + 0.8 * torch.randn(M, A, dtype=dt) * scale).detach()
    # ratios on both sides of the clip range, a third of the rows exactly at ratio 1, some zero
    # advantages; old values on both sides of the value clip range
    lp_now = distrib.log_prob(action).detach()
    log_prob_old = lp_now + 0.5 * torch.randn(M, dtype=dt)
    log_prob_old[::3] = lp_now[::3]
    adv = torch.randn(M, dtype=dt)
    adv[1::7] = 0
    v_old = value.detach().reshape(-1) + 0.3 * torch.randn(M, dtype=dt)
    v_teacher = torch.randn(M, dtype=dt)
    records = {}
    loss = ag._lossfun(distrib.entropy(), value, distrib.log_prob(action),
                       vs_pred_old=v_old[:, None], log_probs_old=log_prob_old, advs=adv,
                       vs_teacher=v_teacher[:, None], records=records)
    loss.backward()
    scale_vec = torch.sqrt(_exp2(head.var_param.detach())).expand(A)
    out4, dmean, dvalue, dscale = ops.gaussian_ppo_loss_closed_form(
        mean.detach(), scale_vec, value.detach(), action, adv, log_prob_old, v_old, v_teacher,
        ag.clip_eps, ag.clip_eps_vf, ag.value_func_coef, ag.entropy_coef)
    want4 = torch.stack([loss.detach(), records["policy_loss"].detach(),
                         records["value_loss"].detach(), distrib.entropy().mean().detach()])
    np.testing.assert_allclose(out4.numpy(), want4.numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(dmean.numpy(), mean.grad.numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(dvalue.numpy(), value.grad.numpy(), rtol=1e-12, atol=1e-12)
    # chain through scale = sqrt(var_func(var_param)) by autograd, as the agent does
    p = head.var_param.detach().clone().requires_grad_(True)
    torch.sqrt(_exp2(p)).expand(A).backward(dscale)
    np.testing.assert_allclose(p.grad.numpy(), head.var_param.grad.numpy(), rtol=1e-12, atol=1e-12)


def _plain_example_model(obs=17, act=6, head=None):
    import pfrl_amd as pfrl

    nn = torch.nn
    head = head or pfrl.policies.GaussianHeadWithStateIndependentCovariance(
        action_size=act, var_type="diagonal", var_func=_exp2, var_param_init=0)
    policy = nn.Sequential(nn.Linear(obs, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(),
                           nn.Linear(64, act), head)
    vf = nn.Sequential(nn.Linear(obs, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 1))
    return pfrl.nn.Branched(policy, vf)


def _fixture_model(obs=11, act=3, head=None, out=None):
    import pfrl_amd as pfrl

    nn = torch.nn
    head = head or pfrl.policies.GaussianHeadWithStateIndependentCovariance(
        action_size=act, var_type="spherical", var_param_init=0.5)
    return nn.Sequential(
        nn.Linear(obs, 16), nn.Tanh(),
        pfrl.nn.Branched(nn.Sequential(nn.Linear(16, out or act), head), nn.Linear(16, 1)))


def _split_of(agent):
    from pfrl_amd.agents.ppo import _ActGraph

    return _ActGraph(agent)._gaussian_split()


@pytest.mark.parametrize("shape", ["example", "fixture", "fixed"])
def test_gaussian_split_recognises_the_model_shapes_in_use(shape):
    import pfrl_amd as pfrl

    torch.manual_seed(5)
    if shape == "example":
        model, obs, act = _plain_example_model(), 17, 6
    elif shape == "fixture":
        model, obs, act = _fixture_model(), 11, 3
    else:
        model, obs, act = _plain_example_model(
            head=pfrl.policies.GaussianHeadWithFixedCovariance(scale=0.4)), 17, 6
    ag = _cpu_agent(model)
    params = [p.data_ptr() for p in model.parameters()]
    split = _split_of(ag)
    assert split is not None
    view, head = split
    assert type(view) is type(model)
    # a view: the model keeps its head, the same parameters sit behind both
    assert isinstance(model(torch.zeros(2, obs))[0], torch.distributions.Distribution)
    assert [p.data_ptr() for p in model.parameters()] == params
    assert {p.data_ptr() for p in view.parameters()} <= set(params)
    x = torch.randn(7, obs)
    mean, value = view(x)
    distrib, want_value = model(x)
    assert tuple(mean.shape) == (7, act) and tuple(value.shape) == (7, 1)
    assert torch.equal(mean, distrib.base_dist.loc) and torch.equal(value, want_value)
    from pfrl_amd.agents.ppo import _ActGraph

    g = _ActGraph(ag)
    g._gaussian_split()
    scale = g.gaussian_scale(head, act)
    assert tuple(scale.shape) == (act,)
    assert torch.equal(scale.expand(7, act), distrib.base_dist.scale.expand(7, act))


def test_gaussian_split_refuses_everything_else():
    import pfrl_amd as pfrl
    from pfrl_amd import agents

    torch.manual_seed(6)
    # state-dependent variance
    assert _split_of(_cpu_agent(_fixture_model(
        head=pfrl.policies.GaussianHeadWithDiagonalCovariance(), out=6))) is None
    # more than 32 action dimensions
    assert _split_of(_cpu_agent(_plain_example_model(act=33))) is None
    assert _split_of(_cpu_agent(_plain_example_model(act=32))) is not None
    # a categorical policy
    cat = torch.nn.Sequential(
        torch.nn.Linear(11, 16), torch.nn.Tanh(),
        pfrl.nn.Branched(torch.nn.Sequential(torch.nn.Linear(16, 4),
                                             pfrl.policies.SoftmaxCategoricalHead()),
                         torch.nn.Linear(16, 1)))
    assert _split_of(_cpu_agent(cat)) is None
    # parameters that are not float32
    assert _split_of(_cpu_agent(_plain_example_model().double())) is None
    # a subclass of the head (its forward may be anything)
    class MyHead(pfrl.policies.GaussianHeadWithStateIndependentCovariance):
        pass

    assert _split_of(_cpu_agent(_plain_example_model(head=MyHead(action_size=6)))) is None
    # _sample_action / _lossfun patched on the instance, or overridden in a subclass
    ag = _cpu_agent(_plain_example_model())
    assert _split_of(ag) is not None
    ag._sample_action = lambda distrib: distrib.sample()
    assert _split_of(ag) is None
    ag = _cpu_agent(_plain_example_model())
    ag._lossfun = ag._lossfun
    assert _split_of(ag) is None

    class MyPPO(agents.PPO):
        def _lossfun(self, *a, **kw):
            return super()._lossfun(*a, **kw)

    model = _plain_example_model()
    ag = MyPPO(model, torch.optim.Adam(model.parameters()), gpu=None)
    assert _split_of(ag) is None
    # a recurrent model
    rec = pfrl.nn.RecurrentSequential(
        torch.nn.LSTM(num_layers=1, input_size=11, hidden_size=16),
        pfrl.nn.Branched(torch.nn.Sequential(
            torch.nn.Linear(16, 3),
            pfrl.policies.GaussianHeadWithStateIndependentCovariance(action_size=3)),
            torch.nn.Linear(16, 1)))
    ag = agents.PPO(rec, torch.optim.Adam(rec.parameters()), gpu=None, recurrent=True)
    assert _split_of(ag) is None


# -- one update on the reference's own state ----------------------------------------------------------
def _example_model(head=None, out=ACT):
    import pfrl_amd as pfrl

    nn = torch.nn
    head = head or pfrl.policies.GaussianHeadWithStateIndependentCovariance(
        action_size=ACT, var_type="diagonal", var_func=_exp2, var_param_init=0)
    policy = nn.Sequential(nn.Linear(OBS, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(),
                           nn.Linear(64, out), head)
    vf = nn.Sequential(nn.Linear(OBS, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 1))
    for layer, gain in ((policy[0], 1), (policy[2], 1), (policy[4], 1e-2), (vf[0], 1), (vf[2], 1),
                        (vf[4], 1)):
        nn.init.orthogonal_(layer.weight, gain=gain)
        nn.init.zeros_(layer.bias)
    return pfrl.nn.Branched(policy, vf)


def _agent(gpu, model=None, standardize_advantages=True, **kw):
    import pfrl_amd as pfrl
    from pfrl_amd import agents

    model = model or _example_model()
    normalizer = pfrl.nn.EmpiricalNormalization(OBS, clip_threshold=5)
    opt = torch.optim.Adam(model.parameters(), lr=3e-4, eps=1e-5)
    args = dict(update_interval=256, minibatch_size=64, epochs=2, clip_eps_vf=None, entropy_coef=0,
                gamma=0.995, lambd=0.97)
    args.update(kw)
    return agents.PPO(model, opt, obs_normalizer=normalizer, gpu=gpu,
                      standardize_advantages=standardize_advantages, **args)


def _load_flat(tensors, flat):
    off = 0
    with torch.no_grad():
        for p in tensors:
            n = p.numel()
            p.copy_(torch.as_tensor(flat[off:off + n]).view_as(p))
            off += n
    assert off == len(flat)


def _teacher_forced_state(ag, g, k):
    """Parameters, Adam state and normaliser statistics of the reference before update k."""
    params = list(ag.model.parameters())
    _load_flat(params, g["u%d_params" % k])
    step = float(g["u%d_step" % k])
    if step > 0:
        for p in params:
            ag.optimizer.state[p] = dict(step=torch.tensor(step), exp_avg=torch.zeros_like(p),
                                         exp_avg_sq=torch.zeros_like(p))
        _load_flat([ag.optimizer.state[p]["exp_avg"] for p in params], g["u%d_exp_avg" % k])
        _load_flat([ag.optimizer.state[p]["exp_avg_sq"] for p in params], g["u%d_exp_avg_sq" % k])
    n = ag.obs_normalizer
    with torch.no_grad():
        n._mean.copy_(torch.as_tensor(g["u%d_norm_mean" % k]))
        n._var.copy_(torch.as_tensor(g["u%d_norm_var" % k]))
        n.count.fill_(int(g["u%d_norm_count" % k]))
    n._cached_std_inverse = None


def _check_teacher_forced(got_losses, ag, g, k):
    want = g["u%d_losses" % k]
    for a, b, what in zip(got_losses, want, ("loss", "value loss", "policy loss")):
        assert abs(a - b) <= 1e-5 * max(1.0, abs(b)), (int(k), what, a, float(b))
    after = np.concatenate([p.detach().cpu().numpy().ravel() for p in ag.model.parameters()])
    np.testing.assert_allclose(after, g["u%d_params_after" % k], rtol=1e-5, atol=1e-6)
    assert not np.array_equal(after, g["u%d_params" % k])


def test_teacher_forced_gaussian_ppo_update_on_the_host_path():
    """The same three updates through the list-of-dicts path (``gpu=None``): torch.distributions,
    autograd, stock Adam.  Its device twin is in test_ppo_gaussian.py."""
    from pfrl_amd.agents import ppo_host

    g = np.load(os.path.join(GOLDEN, "teacher_forced_ppo_gaussian.npz"))
    for k in g["updates"]:
        torch.manual_seed(1)
        ag = _agent(None, standardize_advantages=False, clip_eps=float(g["hyper"][0]))
        _teacher_forced_state(ag, g, k)
        G = lambda name: g["u%d_%s" % (k, name)]   # noqa: E731
        transitions = [dict(state=G("states")[i], action=G("actions")[i], adv=float(G("advs")[i]),
                            v_pred=float(G("vs_pred_old").reshape(-1)[i]),
                            log_prob=float(G("log_probs_old")[i]),
                            v_teacher=float(G("vs_teacher").reshape(-1)[i]))
                       for i in range(len(G("states")))]
        seen = []
        orig = ag._lossfun

        def spy(*a, **kw):
            loss = orig(*a, **kw)
            seen.append(float(loss.detach()))
            return loss

        ag._lossfun = spy
        distribs, vs_pred = ag.model(ppo_host._states(transitions, "state", ag.batch_states, ag.device,
                                                      ag.phi, ag.obs_normalizer))
        ag._host._step(transitions, distribs, vs_pred, None, None)
        _check_teacher_forced([seen[0], float(ag.value_loss_record.values()[-1]),
                               float(ag.policy_loss_record.values()[-1])], ag, g, k)
