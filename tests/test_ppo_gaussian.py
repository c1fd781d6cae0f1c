"""PPO with a Gaussian policy on the fused, captured device path (csrc/ppo_gaussian.hip,
agents/ppo.py): the three launches against the torch expressions they replace, one teacher-forced
update on the reference's own state, and the whole agent against itself with every switch off."""
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SWITCHES = ("PFRL_PPO_FUSED_LOSS", "PFRL_PPO_UPDATE_GRAPH", "PFRL_PPO_ACT_GRAPH", "PFRL_PPO_ACT_HEAD")



@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from pfrl_amd import _native

    _native.lib()  # fail loudly if the HIP library is missing
    return torch.device("cuda:0")


def _distribution(mean, scale):
    return torch.distributions.Independent(
        torch.distributions.Normal(mean, scale.expand_as(mean)), 1)


@pytest.mark.parametrize("clip_eps_vf", [None, 0.2])
@pytest.mark.parametrize("A", [1, 3, 6, 17, 32])
@pytest.mark.parametrize("M", [1, 37, 64, 2048, 4099])
def test_gaussian_ppo_loss_matches_the_reference_expression_and_its_autograd(dev, M, A, clip_eps_vf):
    """pfrl_ppo_gaussian_loss against PPO._lossfun (pfrl/agents/ppo.py:634-671) on
    ``Independent(Normal(mean, scale))`` with autograd: out4, dmean, dvalue, dscale, every row
    included -- rows clipped from either side, zero advantages, a third of the rows with
    ``log_prob_old`` exactly the current one.  Rows whose ratio (value) sits within 1e-4 of a clip
    bound could fall on either side of it in two f32 evaluations: the inputs keep 1e-3 away from
    the bounds by construction, and the test asserts that from the torch side."""
    from pfrl_amd import ops
    from pfrl_amd.agents.ppo import PPO

    clip_eps = 0.2
    torch.manual_seed(M * 41 + A)
    mean = torch.randn(M, A, device=dev).requires_grad_(True)
    scale = torch.exp(0.3 * torch.randn(A, device=dev)).requires_grad_(True)
    value = torch.randn(M, 1, device=dev).requires_grad_(True)
    with torch.no_grad():
        action = mean + 0.9 * scale * torch.randn(M, A, device=dev)
        lp_now = _distribution(mean, scale).log_prob(action)
    # log-ratios: N(0, 0.3) (ratios ~0.5 .. ~2), moved out of a 1e-3 band around both clip bounds
    shift = torch.randn(M, device=dev) * 0.3
    for bound in (1 - clip_eps, 1 + clip_eps):
        near = (torch.exp(shift) - bound).abs() < 1e-3
        shift = torch.where(near, shift + 0.01, shift)
    shift[::3] = 0.0
    logp_old = lp_now - shift
    adv = torch.randn(M, device=dev)
    adv[::7] = 0.0
    dv = torch.randn(M, device=dev) * 0.3
    if clip_eps_vf is not None:
        dv = torch.where((dv.abs() - clip_eps_vf).abs() < 1e-3, dv * 1.05, dv)
    v_old = value.detach().reshape(-1) + dv
    v_teacher = torch.randn(M, device=dev)

    class _A:
        value_func_coef, entropy_coef = 0.7, 0.02
        value_loss_record = policy_loss_record = None

    _A.clip_eps, _A.clip_eps_vf = clip_eps, clip_eps_vf
    rec = {}
    d = _distribution(mean, scale)
    lp = d.log_prob(action)
    # the precondition, from the torch side
    ratio = torch.exp(lp.detach() - logp_old)
    assert float(torch.min((ratio - (1 - clip_eps)).abs().min(),
                           (ratio - (1 + clip_eps)).abs().min())) > 1e-4
    if clip_eps_vf is not None:
        gap = ((value.detach().reshape(-1) - v_old).abs() - clip_eps_vf).abs()
        assert float(gap.min()) > 1e-4
    if M >= 37:
        assert bool((ratio > 1 + clip_eps).any()) and bool((ratio < 1 - clip_eps).any())
    want = PPO._lossfun(_A, d.entropy(), value, lp, vs_pred_old=v_old[:, None],
                        log_probs_old=logp_old, advs=adv, vs_teacher=v_teacher[:, None], records=rec)
    want.backward()
    out4, dmean, dvalue, dscale = ops.ppo_gaussian_loss(
        mean, scale, value, action, adv, logp_old, v_old, v_teacher, clip_eps, clip_eps_vf,
        _A.value_func_coef, _A.entropy_coef)
    want4 = torch.stack([want.detach(), rec["policy_loss"].detach(), rec["value_loss"].detach(),
                         d.entropy().mean().detach()])
    print("out4", out4.tolist(), "want", want4.tolist(),
          "max |dmean|", float((dmean - mean.grad).abs().max()),
          "max |dvalue|", float((dvalue - value.grad).abs().max()),
          "max |dscale|", float((dscale - scale.grad).abs().max()))
    for i in range(4):
        assert torch.allclose(out4[i], want4[i], rtol=1e-5, atol=1e-6), (i, out4.tolist(), want4.tolist())
    tol = dict(rtol=2e-5, atol=2e-7)
    assert dvalue.shape == value.shape and dscale.shape == scale.shape
    assert torch.allclose(dvalue, value.grad, **tol), float((dvalue - value.grad).abs().max())
    assert torch.allclose(dmean, mean.grad, **tol), float((dmean - mean.grad).abs().max())
    assert torch.allclose(dscale, scale.grad, **tol), (dscale.tolist(), scale.grad.tolist())


@pytest.mark.parametrize("N,A", [(1, 6), (4, 6), (64, 6), (2048, 6), (64, 1), (64, 32), (2048, 17)])
def test_gaussian_act_draws_what_the_distribution_draws(dev, N, A):
    """With the same generator state the action is ``sample()``'s bit for bit; entropy and
    log_prob(given action) against the distribution."""
    from pfrl_amd import ops

    torch.manual_seed(1000 + N + A)
    mean = torch.randn(N, A, device=dev) * 2
    scale = torch.exp(0.5 * torch.randn(A, device=dev))
    d = _distribution(mean, scale)
    torch.manual_seed(77)
    want = d.sample()
    torch.manual_seed(77)
    z = torch.randn((N, A), dtype=torch.float32, device=dev)
    action, entropy = ops.ppo_gaussian_act(mean, scale, z=z)
    assert torch.equal(action, want)
    assert torch.allclose(entropy, d.entropy(), rtol=1e-5, atol=1e-6)
    given = mean + 1.5 * scale * torch.randn(N, A, device=dev)
    logp = ops.ppo_gaussian_act(mean, scale, given_action=given)
    assert torch.allclose(logp, d.log_prob(given), rtol=1e-5, atol=1e-6), \
        float((logp - d.log_prob(given)).abs().max())
    column = torch.zeros(N + 3, device=dev)
    ops.ppo_gaussian_act(mean, scale, given_action=given, out_log_prob=column[2:N + 2])
    assert torch.equal(column[2:N + 2], logp) and float(column[:2].abs().sum() + column[N + 2:].abs().sum()) == 0


@pytest.mark.parametrize("A", [1, 6, 17])
def test_ppo_minibatch_with_a_float_action_column(dev, A):
    from pfrl_amd import ops

    g = torch.Generator().manual_seed(3 + A)
    D, M, k = 4096, 1000, 1
    T = lambda t: t.to(dev)     # noqa: E731
    adv, lp, v, vt = (T(torch.randn(D, generator=g)) for _ in range(4))
    act = T(torch.randn(D, A, generator=g))
    refs = T(torch.randint(0, 9999, (D, k), generator=g, dtype=torch.int32))
    idx = T(torch.randint(0, D, (M,), generator=g))
    ms = ops.adv_stats(adv)
    out = ops.ppo_minibatch(idx, adv, ms, False, lp, v, vt, act, refs)
    assert out["action"].dtype == torch.float32 and tuple(out["action"].shape) == (M, A)
    for name, col in (("adv", adv), ("log_prob", lp), ("v_pred", v), ("v_teacher", vt),
                      ("action", act), ("refs", refs)):
        assert torch.equal(out[name], col[idx]), name
    out = ops.ppo_minibatch(idx, adv, ms, True, lp, v, vt, act, refs)
    ms_h = ms.cpu().numpy()
    want = (adv.cpu().numpy()[idx.cpu().numpy()] - ms_h[0]) / (ms_h[1] + np.float32(1e-8))
    np.testing.assert_array_equal(out["adv"].cpu().numpy(), want.astype(np.float32))
    assert torch.equal(out["action"], act[idx])


# -- the agent -------------------------------------------------------------------------------------
from test_ppo_gaussian_cpu import (ACT, GOLDEN, OBS, _agent, _check_teacher_forced,  # noqa: E402
                                   _example_model, _teacher_forced_state)


def test_teacher_forced_gaussian_ppo_update_on_the_device_path():
    """The first, a middle and the last minibatch update of the reference's run
    (tests/golden/make_teacher_forced_ppo_gaussian.py) on its own parameters, Adam state, normaliser
    statistics and minibatch, through the fused loss inside the captured update: the three loss
    terms at 1e-5, the parameters after the Adam step at rtol 1e-5 / atol 1e-6."""
    g = np.load(os.path.join(GOLDEN, "teacher_forced_ppo_gaussian.npz"))
    for k in g["updates"]:
        torch.manual_seed(1)
        ag = _agent(0, standardize_advantages=False, clip_eps=float(g["hyper"][0]))
        dev = ag.device
        _teacher_forced_state(ag, g, k)
        T = lambda name: torch.as_tensor(g["u%d_%s" % (k, name)]).to(dev)   # noqa: E731
        states = g["u%d_states" % k]
        refs, batch = ag._refs_of(list(states))
        ag._sample_obs = batch[0]
        s_refs = torch.from_numpy(refs).to(dev)
        M = len(states)
        assert M == ag.minibatch_size
        assert ag._captured_update_ok(M, T("actions"))
        cols = ag._static_columns(T("advs"), torch.zeros(2, device=dev), T("log_probs_old"),
                                  T("vs_pred_old").reshape(-1), T("vs_teacher").reshape(-1),
                                  T("actions"), s_refs)
        cols["idx"].copy_(torch.arange(M, device=dev))
        out = ag._update_graph.run({"idx": cols["idx"]}, baked=ag._baked_hyperparameters())
        assert len(ag._update_graph.graphs) == 1
        _check_teacher_forced([float(out["loss"]), float(out["value_loss"]),
                               float(out["policy_loss"])], ag, g, k)


def _run_two_rollouts(monkeypatch, switches_off, model=None, patch=None, n_env=4):
    """Two rollouts of the example model on the synthetic vector-observation env; returns (agent,
    actions per step, (loss, value loss, policy loss) per update, final parameters, ops calls)."""
    import pfrl_amd as pfrl
    from pfrl_amd import ops
    from pfrl_amd.envs.synthetic import HostSyntheticVectorObsEnv

    for name in SWITCHES:
        if switches_off:
            monkeypatch.setenv(name, "0")
        else:
            monkeypatch.delenv(name, raising=False)
    pfrl.utils.set_random_seed(0)
    torch.manual_seed(2468)
    random.seed(5)
    env = HostSyntheticVectorObsEnv(n_env, obs_dim=OBS, act_dim=ACT, seed=3, p_done=0.02)
    ag = _agent(0, model=model)
    if patch is not None:
        patch(ag)
    calls = {"loss": 0, "act": 0}
    orig_loss, orig_act = ops.ppo_gaussian_loss, ops.ppo_gaussian_act

    def spy_loss(*a, **kw):
        calls["loss"] += 1
        return orig_loss(*a, **kw)

    def spy_act(*a, **kw):
        calls["act"] += 1
        return orig_act(*a, **kw)

    monkeypatch.setattr(ops, "ppo_gaussian_loss", spy_loss)
    monkeypatch.setattr(ops, "ppo_gaussian_act", spy_act)
    actions = []
    obs = env.reset()
    steps = 2 * ag.update_interval // n_env
    for t in range(steps):
        a = ag.batch_act(obs)
        actions.append(np.asarray(a).copy())
        obs, r, done, _ = env.step(a)
        ag.batch_observe(obs, r, done, [False] * n_env)
        obs = env.reset(~done)
    vl, pl = ag.value_loss_record.values(), ag.policy_loss_record.values()
    params = np.concatenate([p.detach().cpu().numpy().ravel() for p in ag.model.parameters()])
    monkeypatch.setattr(ops, "ppo_gaussian_loss", orig_loss)
    monkeypatch.setattr(ops, "ppo_gaussian_act", orig_act)
    return ag, np.asarray(actions), np.stack([vl, pl], axis=1), params, calls


def test_gaussian_ppo_agent_fused_and_captured_against_every_switch_off(monkeypatch):
    """The example model, two rollouts of 256 steps (8 minibatch updates each): the fused + captured
    agent against the same agent with the four switches at 0.  Rollout 1: the same actions bit for
    bit (same parameters, same generator offsets, torch.normal's roundings).  Rollout 2: parameters
    differ by f32 rounding -- actions at 1e-4.  Every value / policy loss and the final parameters at
    rtol 1e-5, atol 1e-6."""
    ag, act, losses, params, calls = _run_two_rollouts(monkeypatch, switches_off=False)
    per_rollout = ag.update_interval // 4
    n_updates = 2 * ag.epochs * ag.update_interval // ag.minibatch_size
    assert ag.n_updates == n_updates and len(losses) == n_updates
    # captured: the update graph exists, holds ONE graph, and python ran the fused loss only while
    # capturing it (2 warm-ups + 1 capture), not once per update
    assert ag._update_graph is not None and len(ag._update_graph.graphs) == 1
    assert calls["loss"] == 3
    # acting: one graph for the one batch shape, replayed; python ran the fused head 3 times for the
    # capture and then only in the two value passes
    assert len(ag._act_graph.entries) == 1
    assert calls["act"] == 3 + 2
    ref, ref_act, ref_losses, ref_params, ref_calls = _run_two_rollouts(monkeypatch, switches_off=True)
    assert ref._update_graph is None and ref_calls == {"loss": 0, "act": 0}
    assert ref._act_graph is None or len(ref._act_graph.entries) == 0
    assert ref.n_updates == n_updates
    assert act.dtype == np.float32 and act.shape == (2 * per_rollout, 4, ACT)
    np.testing.assert_array_equal(act[:per_rollout], ref_act[:per_rollout])
    np.testing.assert_allclose(act[per_rollout:], ref_act[per_rollout:], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(losses, ref_losses, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(params, ref_params, rtol=1e-5, atol=1e-6)


def test_unrecognised_gaussian_agents_take_the_eager_path(monkeypatch):
    """A state-dependent variance, and ``_sample_action`` patched on the instance: they run, and
    neither fused launch is used."""
    import pfrl_amd as pfrl

    torch.manual_seed(31)
    model = _example_model(head=pfrl.policies.GaussianHeadWithDiagonalCovariance(), out=2 * ACT)
    ag, act, losses, _, calls = _run_two_rollouts(monkeypatch, switches_off=False, model=model)
    assert calls == {"loss": 0, "act": 0} and ag._update_graph is None
    assert ag.n_updates == 16 and np.isfinite(losses).all() and np.isfinite(act).all()

    def patch(agent):
        agent._sample_action = lambda distrib: distrib.sample()

    ag, act, losses, _, calls = _run_two_rollouts(monkeypatch, switches_off=False, patch=patch)
    assert calls == {"loss": 0, "act": 0} and ag._update_graph is None
    assert ag.n_updates == 16 and np.isfinite(losses).all() and np.isfinite(act).all()
