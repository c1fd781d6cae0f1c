"""TRPO on the device route (csrc/trpo.hip, agents/trpo.py): each kernel against its closed form or
bit for bit, the agent with every switch on against every switch off, one teacher-forced policy
update on the reference's recorded state, and a line search that is made to fail."""
import random

import numpy as np
import pytest
import torch

from test_trpo_cpu import (ACT, OBS, SWITCHES, _agent, _distribution, _flat, _load_flat, _run_trace,
                           _trace)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from pfrl_amd import _native

    _native.lib()  # fail loudly if the HIP library is missing
    return torch.device("cuda:0")


def _close(got, want, rtol=1e-5, atol=1e-7):
    """The project's teacher-forced tolerance: 1e-5 relative with an absolute floor of 1e-7."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err = np.abs(got - want)
    bound = np.maximum(rtol * np.abs(want), atol)
    assert np.all(err <= bound), (float(err.max()), float((err / bound).max()))


# -- pfrl_trpo_gaussian_eval ---------------------------------------------------------------------------
def _eval_inputs(dev, M, A, spread=1.0, positive_adv=False):
    g = torch.Generator().manual_seed(M * 131 + A)
    r = lambda *s: torch.randn(*s, generator=g)     # noqa: E731
    mean = r(M, A)
    scale = torch.exp(0.3 * r(A))
    mean_old = mean + 0.05 * r(M, A)
    scale_old = scale * torch.exp(0.05 * r(A))
    action = mean_old + spread * scale_old * r(M, A)
    log_prob_old = _distribution(mean_old.double(), scale_old.double()).log_prob(action.double()).float()
    adv = r(M).abs() + 0.5 if positive_adv else r(M)
    return [t.to(dev) for t in (mean, scale, mean_old, scale_old, action, adv, log_prob_old)]


@pytest.mark.parametrize("A", [1, 3, 17])
@pytest.mark.parametrize("M", [1, 63, 64, 65, 2053])
def test_gaussian_eval_matches_the_torch_expression_in_float64(dev, M, A):
    """out3 and the gradient of the gain against torch.distributions + autograd in float64 on the same
    float32 operands; two calls are bit-identical.

    The kernel keeps log pi(a | s) in float32, summed in the acting launch's order (an unchanged
    policy must give ratio exactly 1), so every row term carries the relative error of that sum,
    ~2^-24 |log pi| c: 2e-6 at A = 17.  A sum over rows can then be held to 1e-5 relative only where
    it does not cancel: the inputs are positive advantages and actions drawn 1.5 scales wide
    (E[(d / s)^2 - 1] = 1.25 instead of 0), and the test asserts from the float64 side that every
    checked sum has sum |terms| / |sum| < 8 (the row errors are independent: the sum's relative error
    stays well below that factor times 2e-6).  Zero-mean and NaN advantages: the two tests below."""
    from pfrl_amd import ops

    coef = 0.02
    mean, scale, mean_old, scale_old, action, adv, lpo = _eval_inputs(dev, M, A, spread=1.5,
                                                                      positive_adv=True)
    m64 = mean.double().cpu().requires_grad_(True)
    s64 = scale.double().cpu().requires_grad_(True)
    new = _distribution(m64, s64)
    old = _distribution(mean_old.double().cpu(), scale_old.double().cpu())
    gain = (torch.exp(new.log_prob(action.double().cpu()) - lpo.double().cpu()) * adv.double().cpu()).mean() \
        + coef * new.entropy().mean()
    kl = torch.distributions.kl_divergence(old, new).mean()
    gain.backward()
    with torch.no_grad():       # the precondition, from the torch side
        g_row = torch.exp(new.log_prob(action.double().cpu()) - lpo.double().cpu()) * adv.double().cpu() / M
        d = action.double().cpu() - m64
        terms = g_row[:, None] * (d * d / s64 ** 3 - 1 / s64)
        cond = terms.abs().sum(0) / terms.sum(0).abs()
        assert float(cond.max()) < 8.0, cond.tolist()
    out3, dmean, dscale = ops.trpo_gaussian_eval(mean, scale, mean_old, scale_old, action, adv, lpo, coef,
                                                 want_grad=True)
    want3 = [float(gain), float(kl), float(new.entropy().mean())]
    print("out3", out3.tolist(), "want", want3,
          "max |dmean|", float((dmean.cpu().double() - m64.grad).abs().max()),
          "max |dscale|", float((dscale.cpu().double() - s64.grad).abs().max()))
    _close(out3.cpu().numpy(), want3)
    _close(dmean.cpu().numpy(), m64.grad.numpy())
    _close(dscale.cpu().numpy(), s64.grad.numpy())
    again, dmean2, dscale2 = ops.trpo_gaussian_eval(mean, scale, mean_old, scale_old, action, adv, lpo,
                                                    coef, want_grad=True)
    assert torch.equal(out3, again) and torch.equal(dmean, dmean2) and torch.equal(dscale, dscale2)
    plain = ops.trpo_gaussian_eval(mean, scale, mean_old, scale_old, action, adv, lpo, coef)
    assert torch.equal(plain, out3)


@pytest.mark.parametrize("A", [1, 3, 17])
@pytest.mark.parametrize("M", [1, 63, 64, 65, 2053])
def test_gaussian_eval_with_standardised_advantages_within_its_forward_error_bound(dev, M, A):
    """Zero-mean advantages, as the agent's standardised ones are: the gain and the scale gradient are
    sums that cancel, so a relative tolerance on the result means nothing and the bound comes from
    the terms instead (as tests/test_conv_geometry.py does), U = 2^-24:

    row m   log pi is a float32 sum of A elements x_j = -q_j - log s_j - log sqrt(2 pi), q_j =
            d_j^2 / (2 s_j^2): at most 5 roundings on q_j, 2 U on log s_j, one per subtraction -- 7 U
            on l_j = q_j + |log s_j| + log sqrt(2 pi) -- then a tree of D + 1 additions, D =
            ceil(log2 A).  So |error of log pi| <= (8 + D) U L_m, L_m = sum_j l_j, which is the relative
            error of ratio = exp(log pi - log pi_old); expf (2 U), the subtraction, the product with
            the advantage and the division by M add 5 U: e_m = (8 + D) U L_m + 5 U.
    gain    rows are added in float64: |error| <= sum_m |g_m| e_m + U (|sum| + 2 |coef H|), g_m =
            ratio_m adv_m / M.
    dmean   g_m d_j / s_j^2, four more roundings: |error| <= |dmean_mj| (e_m + 4 U).
    dscale  sum_m g_m (d^2 / s^3 - 1 / s) in float64 from the float32 g_m and d^2 (3 U):
            |error| <= sum_m |g_m| ((e_m + 3 U) d^2 / s^3 + e_m / s) + U |dscale_j|.
    Asserted at twice these first-order bounds, computed from the float64 side only."""
    from pfrl_amd import ops

    coef = 0.02
    U = 2.0 ** -24
    mean, scale, mean_old, scale_old, action, adv, lpo = _eval_inputs(dev, M, A)
    if M > 1:
        adv = (adv - adv.mean()) / (adv.std(unbiased=False) + 1e-8)
    m64 = mean.double().cpu().requires_grad_(True)
    s64 = scale.double().cpu().requires_grad_(True)
    a64, adv64, lpo64 = action.double().cpu(), adv.double().cpu(), lpo.double().cpu()
    new = _distribution(m64, s64)
    surrogate = (torch.exp(new.log_prob(a64) - lpo64) * adv64).mean()
    bonus = coef * new.entropy().mean()
    (surrogate + bonus).backward()
    with torch.no_grad():
        d = a64 - m64
        L = (d * d / (2 * s64 * s64) + s64.log().abs() + 0.9189385332046727).sum(1)
        D = int(np.ceil(np.log2(A))) if A > 1 else 0
        e = (8 + D) * U * L + 5 * U
        g_row = (torch.exp(new.log_prob(a64) - lpo64) * adv64 / M).abs()
        gain_bound = 2 * ((g_row * e).sum() + U * (surrogate.abs() + 2 * bonus.abs()))
        dmean_bound = 2 * m64.grad.abs() * (e[:, None] + 4 * U)
        dscale_bound = 2 * ((g_row[:, None] * ((e[:, None] + 3 * U) * d * d / s64 ** 3
                                               + e[:, None] / s64)).sum(0) + U * s64.grad.abs())
    out3, dmean, dscale = ops.trpo_gaussian_eval(mean, scale, mean_old, scale_old, action, adv, lpo, coef,
                                                 want_grad=True)
    gain_err = abs(float(out3[0]) - float(surrogate + bonus))
    dmean_err = (dmean.cpu().double() - m64.grad).abs()
    dscale_err = (dscale.cpu().double() - s64.grad).abs()
    print("gain", float(out3[0]), "want", float(surrogate + bonus), "err / bound", gain_err / float(gain_bound),
          "dmean", float((dmean_err / dmean_bound.clamp(min=1e-300)).max()),
          "dscale", float((dscale_err / dscale_bound).max()), "bounds", float(gain_bound),
          float(dscale_bound.max()))
    assert gain_err <= float(gain_bound)
    assert bool((dmean_err <= dmean_bound).all())
    assert bool((dscale_err <= dscale_bound).all())


@pytest.mark.parametrize("M,A", [(1, 1), (65, 3), (2053, 17)])
def test_gaussian_eval_of_an_unchanged_policy_and_of_a_nan_advantage(dev, M, A):
    """old = new: the KL is exactly 0, and with the log-probability the acting launch recorded the
    ratio is exactly 1 (gain = mean advantage + bonus).  A NaN advantage makes the gain NaN."""
    from pfrl_amd import ops

    mean, scale, _, _, action, adv, _ = _eval_inputs(dev, M, A)
    lp = ops.ppo_gaussian_act(mean, scale, given_action=action)
    out3 = ops.trpo_gaussian_eval(mean, scale, mean, scale, action, adv, lp, 0.0)
    assert float(out3[1]) == 0.0
    _close(float(out3[0]), float(adv.double().mean()), rtol=1e-6)
    adv[M // 2] = float("nan")
    out3 = ops.trpo_gaussian_eval(mean, scale, mean, scale, action, adv, lp, 0.0)
    assert np.isnan(float(out3[0])) and float(out3[1]) == 0.0


# -- conjugate gradient ----------------------------------------------------------------------------------
def _reference_cg(A_product_func, b, tol=1e-10, max_iter=10):
    from pfrl_amd.utils.conjugate_gradient import conjugate_gradient

    return conjugate_gradient(A_product_func, b, tol=tol, max_iter=max_iter)


def _spd(n, seed):
    """Q^T D Q + 0.01 I, float64 on the CPU: D log-uniform in [1, 500] (condition number <= 1e3 with
    the shift), Q a product of two Householder reflections, so the dense matrix costs O(n^2)."""
    g = torch.Generator().manual_seed(seed)
    d = torch.exp(torch.rand(n, generator=g, dtype=torch.float64) * np.log(500.0))
    A = torch.diag(d)
    for _ in range(2):
        v = torch.randn(n, generator=g, dtype=torch.float64)
        v /= v.norm()
        Av = A @ v
        c = float(v @ Av)
        A.addr_(v, Av, alpha=-2.0).addr_(Av, v, alpha=-2.0).addr_(v, v, alpha=4.0 * c)
    A.diagonal().add_(0.01)
    return A, torch.randn(n, generator=g, dtype=torch.float64)


def _cg_sizes():
    from pfrl_amd import _native

    reach = 8192
    if _native.available():
        reach = int(_native.lib().pfrl_cg_workgroup_reach())
    return [1, 255, 256, 257, reach - 1, reach, reach + 1]


@pytest.mark.parametrize("n", _cg_sizes())
def test_device_cg_against_the_reference_loop(dev, n):
    """Ten steps on a random SPD system applied as a torch matvec, against the host-driven loop in
    float64 on the CPU.  Tolerance: ten times the distance between that run and the same loop in
    float32 on the CPU -- computed here from those two runs, never from the kernel."""
    from pfrl_amd import ops

    A64, b64 = _spd(n, seed=n)
    want = _reference_cg(lambda v: A64 @ v, b64)
    A32, b32 = A64.float(), b64.float()
    cpu32 = _reference_cg(lambda v: A32 @ v, b32)
    tol = 10.0 * float((cpu32.double() - want).abs().max())
    A_dev, b_dev = A32.to(dev), b32.to(dev)
    x = ops.conjugate_gradient_device(lambda v: torch.mv(A_dev, v), b_dev, max_iter=10)
    err = float((x.cpu().double() - want).abs().max())
    print("n", n, "err", err, "tol", tol, "|x|", float(want.abs().max()))
    assert tol > 0 or n == 1
    assert err <= tol, (err, tol)
    x2 = ops.conjugate_gradient_device(lambda v: torch.mv(A_dev, v), b_dev, max_iter=10)
    assert torch.equal(x, x2)


@pytest.mark.parametrize("n", _cg_sizes())
def test_device_cg_stops_changing_once_converged(dev, n):
    """A = I: the reference returns after one iteration.  ``done`` is set by step 1, and x, r, p after
    ten steps are what they were after one, bit for bit."""
    from pfrl_amd import ops

    b = torch.randn(n, generator=torch.Generator().manual_seed(n + 7)).to(dev)
    cg = ops.DeviceCG(b)
    assert cg.state.tolist()[3] == 0.0
    cg.step(cg.p.clone())
    assert cg.state.tolist()[3] == 1.0
    first = [t.clone() for t in (cg.x, cg.r, cg.p)]
    state = cg.state.clone()
    for _ in range(9):
        cg.step(cg.p.clone())
    assert all(torch.equal(a, b_) for a, b_ in zip(first, (cg.x, cg.r, cg.p)))
    assert torch.equal(state, cg.state)
    assert torch.equal(cg.x, b) and float(cg.r.abs().max()) == 0.0


# -- parameter step and KL scale -----------------------------------------------------------------------
@pytest.mark.parametrize("step_size", [1.0, 0.5, 2.0 ** -10, 0.0])
@pytest.mark.parametrize("sizes", [[(4097,)], [(1,), (3, 5), (4097,), (7,), (64, 65), (1, 1), (4096,)]])
def test_params_axpy_is_the_torch_expression_bit_for_bit(dev, sizes, step_size):
    from pfrl_amd import ops

    g = torch.Generator().manual_seed(len(sizes))
    params = [torch.zeros(s, device=dev) for s in sizes]
    total = sum(p.numel() for p in params)
    base = torch.randn(total, generator=g).to(dev)
    full_step = (torch.randn(total, generator=g) * 3).to(dev)
    ops.params_axpy(params, base, full_step, step_size)
    want = base + step_size * full_step
    pieces = torch.split(want, [p.numel() for p in params])
    for p, w in zip(params, pieces):
        assert torch.equal(p, w.reshape(p.shape))
    if step_size == 0.0:
        assert torch.equal(torch.cat([p.reshape(-1) for p in params]), base)


@pytest.mark.parametrize("n", [1, 257, 4097, 9001])
def test_scale_step_against_the_python_expression(dev, n):
    from pfrl_amd import ops

    g = torch.Generator().manual_seed(n)
    d = torch.randn(n, generator=g)
    Fd = d * torch.exp(torch.randn(n, generator=g))
    max_kl = 0.01
    dId = float(d.double().dot(Fd.double()))
    scale = (2.0 * max_kl / (dId + 1e-8)) ** 0.5
    full_step, out = ops.trpo_scale_step(d.to(dev), Fd.to(dev), max_kl)
    np.testing.assert_allclose(out.cpu().numpy(), [scale, dId], rtol=1e-6)
    np.testing.assert_allclose(full_step.cpu().numpy(), scale * d.numpy().astype(np.float64), rtol=1e-6)


# -- the agent -------------------------------------------------------------------------------------------
def _device_run(switches_on, updates=3, n_env=8, update_interval=128, **kw):
    g = _trace()
    after_update = kw.pop("after_update", None)
    args = {name: switches_on for name in SWITCHES}
    args.update(kw)
    ag = _agent(g, "norm_", 0, update_interval=update_interval, **args)
    actions, ups = _run_trace(ag, updates * update_interval // n_env, n_env=n_env,
                              after_update=after_update)
    assert len(ups) == updates
    return ag, actions, ups


def _learning_state(ag):
    """Copies of everything an update writes: policy, value function, the optimizer's state."""
    opt = [{k: (v.detach().clone() if torch.is_tensor(v) else v)
            for k, v in ag.vf_optimizer.state.get(p, {}).items()} for p in ag.vf.parameters()]
    return ([p.detach().clone() for p in ag.policy.parameters()],
            [p.detach().clone() for p in ag.vf.parameters()], opt)


def _load_learning_state(ag, state):
    policy, vf, opt = state
    with torch.no_grad():
        for p, q in zip(list(ag.policy.parameters()) + list(ag.vf.parameters()), policy + vf):
            p.copy_(q)
        for p, theirs in zip(ag.vf.parameters(), opt):
            mine = ag.vf_optimizer.state[p]
            assert set(mine) == set(theirs)
            for k, v in theirs.items():
                if torch.is_tensor(mine[k]):
                    mine[k].copy_(v)
                else:
                    mine[k] = v


def test_agent_with_every_switch_on_against_every_switch_off(monkeypatch):
    """8 envs, update_interval 128, three updates, Gaussian policy with a normaliser.

    Free-running, both settings: the chosen step sizes are equal; KL and parameters agree within the
    CPU fixture's measured tolerance after every update.  The switches select how an update is
    computed, not how an action is drawn, and the two updates round differently (float64 row sums in
    the kernels, float32 reductions in eager torch), so from the second rollout on the free-running
    actions differ where the parameters do.  That sampling is unchanged is therefore checked exactly:
    a third run with the switches off is handed, after each of its updates, what the switches-on run
    had learned at that point (policy, value function, optimizer state).  It consumes the same random
    streams, so every action of all three rollouts must equal the switches-on run's, bit for bit --
    and each of its updates, now starting from the very state the switches-on update started from,
    must land within the same tolerance of it."""
    from pfrl_amd import ops

    calls = {"eval": 0, "axpy": 0, "cg": 0}
    orig = ops.trpo_gaussian_eval, ops.params_axpy, ops.conjugate_gradient_device
    monkeypatch.setattr(ops, "trpo_gaussian_eval",
                        lambda *a, **k: (calls.__setitem__("eval", calls["eval"] + 1), orig[0](*a, **k))[1])
    monkeypatch.setattr(ops, "params_axpy",
                        lambda *a, **k: (calls.__setitem__("axpy", calls["axpy"] + 1), orig[1](*a, **k))[1])
    monkeypatch.setattr(ops, "conjugate_gradient_device",
                        lambda *a, **k: (calls.__setitem__("cg", calls["cg"] + 1), orig[2](*a, **k))[1])
    learned = []
    on, act_on, ups_on = _device_run(True, after_update=lambda k, ag: learned.append(_learning_state(ag)))
    assert calls["cg"] == 3 and calls["eval"] >= 6 and calls["axpy"] >= 3
    assert on._vf_graph is not None and len(on._vf_graph.graphs) == 1
    seen = dict(calls)
    off, act_off, ups_off = _device_run(False)
    assert calls == seen and off._vf_graph is None
    tol = float(_trace()["norm_param_tol"])
    per = 128 // 8
    np.testing.assert_array_equal(act_on[:per], act_off[:per])
    # (an update is recorded before the hand-over: ups_fed holds what the run computed itself)
    _, act_fed, ups_fed = _device_run(False, after_update=lambda k, ag: _load_learning_state(ag, learned[k]))
    assert calls == seen
    print("actions differing, free-running:", int((act_on != act_off).sum()), "of", act_on.size,
          "max", float(np.abs(act_on - act_off).max()),
          " handed over:", int((act_on != act_fed).sum()))
    np.testing.assert_array_equal(act_on, act_fed)
    for name, ups in (("free", ups_off), ("fed", ups_fed)):
        for k, (a, b) in enumerate(zip(ups_on, ups)):
            print(name, "update", k, "step", a[0], b[0], "kl", a[1], b[1], "policy diff",
                  np.abs(a[2] - b[2]).max(), "vf diff", np.abs(a[3] - b[3]).max(), "tol", tol)
            assert a[0] == b[0] and a[0] > 0
            assert abs(a[1] - b[1]) <= tol
            np.testing.assert_allclose(a[2], b[2], rtol=0, atol=tol)
            np.testing.assert_allclose(a[3], b[3], rtol=0, atol=tol)


@pytest.mark.parametrize("prefix", ["plain_", "norm_"])
def test_teacher_forced_policy_update_on_the_device_route(dev, prefix):
    """The reference's first policy update on its own parameters, normaliser statistics and dataset,
    through the fused device step: accepted step size and KL as recorded, parameters within the
    fixture's tolerance."""
    g = _trace()
    ag = _agent(g, prefix, 0)
    key = prefix + "u0_"
    _load_flat(ag.policy.parameters(), g[key + "policy_before"])
    T = lambda name, dt=torch.float32: torch.as_tensor(g[key + name]).to(dt).to(dev)   # noqa: E731
    states = T("states")
    if ag.obs_normalizer is not None:
        n = ag.obs_normalizer
        with torch.no_grad():
            n._mean.copy_(T("norm_mean").view_as(n._mean))
            n._var.copy_(T("norm_var").view_as(n._var))
            n.count.fill_(int(g[key + "norm_count"]))
        n._cached_std_inverse = None
        states = n(states, update=False)
    advs = ag._standardized(T("advs"))
    assert ag._gaussian_policy_split() is not None
    ag._update_policy_device(states, T("actions"), advs, T("log_probs"))
    tol = float(g[prefix + "param_tol"])
    after = _flat(ag.policy.parameters())
    print(key, "step", ag.policy_step_size_record[-1], "kl", ag.kl_record[-1], float(g[key + "kl"]),
          "policy diff", np.abs(after - g[key + "policy_after"]).max(), "tol", tol)
    assert ag.policy_step_size_record[-1] == float(g[key + "step_size"])
    assert abs(ag.kl_record[-1] - float(g[key + "kl"])) <= tol
    np.testing.assert_allclose(after, g[key + "policy_after"], rtol=0, atol=tol)


def test_a_line_search_that_fails_restores_the_parameters(dev):
    """max_kl = 1e-12 and one NaN advantage: no trial is accepted; the parameters are bit-equal to
    before and the recorded step size is 0.  (max_kl = 1e-12 alone does not make the search fail: the
    full step is scaled to the bound, and on this dataset the reference's own algorithm accepts step
    size 1.0 at KL 7.1e-14.  The NaN row makes every trial's gain NaN -- the case the restore exists
    for, with a step that is not finite either.)"""
    g = _trace()
    ag = _agent(g, "plain_", 0, max_kl=1e-12)
    before = [p.detach().clone() for p in ag.policy.parameters()]
    key = "plain_u0_"
    T = lambda name: torch.as_tensor(g[key + name]).float().to(dev)   # noqa: E731
    advs = ag._standardized(T("advs"))
    advs[5] = float("nan")
    ag._update_policy_device(T("states"), T("actions"), advs, T("log_probs"))
    assert ag.policy_step_size_record[-1] == 0.0 and len(ag.kl_record) == 0
    assert all(torch.equal(a, b) for a, b in zip(before, ag.policy.parameters()))


def test_a_finite_step_that_fails_the_line_search_is_taken_back(dev, monkeypatch):
    """max_kl = 1e-12 with a finite step: ``line_search_max_backtrack = 0`` leaves one trial, and that
    trial's evaluation is made to report a gain 1.0 below the truth, so the search sees no
    improvement.  pfrl_params_axpy wrote base + 1.0 * full_step (finite, not zero) for the trial and
    base + 0.0 * full_step afterwards: the parameters are bit-equal to before, the recorded step size
    is 0 and no KL is recorded."""
    from pfrl_amd import ops

    g = _trace()
    ag = _agent(g, "plain_", 0, max_kl=1e-12, line_search_max_backtrack=0)
    before = [p.detach().clone() for p in ag.policy.parameters()]
    evaluate, axpy = ops.trpo_gaussian_eval, ops.params_axpy
    written = []

    def pessimistic(*a, **k):
        out = evaluate(*a, **k)
        if not k.get("want_grad"):
            out = out.clone()
            out[0] -= 1.0
        return out

    def recorded(params, base, full_step, step_size):
        axpy(params, base, full_step, step_size)
        written.append((step_size, full_step.clone(), [p.detach().clone() for p in params]))

    monkeypatch.setattr(ops, "trpo_gaussian_eval", pessimistic)
    monkeypatch.setattr(ops, "params_axpy", recorded)
    key = "plain_u0_"
    T = lambda name: torch.as_tensor(g[key + name]).float().to(dev)   # noqa: E731
    ag._update_policy_device(T("states"), T("actions"), ag._standardized(T("advs")), T("log_probs"))
    assert [w[0] for w in written] == [1.0, 0.0]
    full_step = written[0][1]
    assert bool(torch.isfinite(full_step).all()) and float(full_step.abs().max()) > 0
    assert any(not torch.equal(a, b) for a, b in zip(before, written[0][2]))     # the trial moved them
    assert ag.policy_step_size_record[-1] == 0.0 and len(ag.kl_record) == 0
    assert all(torch.equal(a, b) for a, b in zip(before, ag.policy.parameters()))


def test_a_softmax_policy_takes_the_device_route_with_torch_expressions(dev):
    """Not a recognised Gaussian head: gain / KL / entropy stay torch.distributions, the conjugate
    gradient and the parameter step still run on the device; nothing goes to the host route."""
    import pfrl_amd as pfrl
    from pfrl_amd import agents
    from pfrl_amd.envs.synthetic import HostSyntheticVectorObsEnv

    torch.manual_seed(4)
    random.seed(4)
    nn = torch.nn
    pi = nn.Sequential(nn.Linear(OBS, 16), nn.Tanh(), nn.Linear(16, 3), pfrl.policies.SoftmaxCategoricalHead())
    vf = nn.Sequential(nn.Linear(OBS, 16), nn.Tanh(), nn.Linear(16, 1))
    ag = agents.TRPO(pi, vf, torch.optim.Adam(vf.parameters(), lr=1e-2), gpu=0, update_interval=64,
                     vf_batch_size=32)
    assert ag._host is None
    env = HostSyntheticVectorObsEnv(4, obs_dim=OBS, act_dim=ACT, seed=1, p_done=0.05)
    obs = env.reset()
    for _ in range(16):
        a = ag.batch_act(obs)
        obs, r, done, _ = env.step(a)
        ag.batch_observe(obs, r, done, [False] * 4)
        obs = env.reset(~done)
    assert len(ag.policy_step_size_record) == 1 and ag._gaussian_policy_split() is None
    assert np.isfinite(_flat(pi.parameters())).all()
