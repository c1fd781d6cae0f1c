"""TD3 and DDPG with the launches of ``csrc/td3.hip`` (``fused_loss=True``, the default on a GPU) against
the torch expressions they replace (``fused_loss=False``: the code as it stood) and the reference:

* teacher-forced on ``teacher_forced_td3.npz`` / ``teacher_forced_ddpg.npz`` through ``_check_td3`` /
  ``_check_ddpg`` of tests/test_teacher_forced_loss.py (losses at 1e-5), with ``agents.TD3`` /
  ``agents.DDPG`` replaced by a factory that fixes ``fused_loss``, keeps the agents and records every
  module's gradient right after its backward, next to that of a float64 CPU replica;
* the rollouts of ``agent_trace_td3.npz`` / ``agent_trace_ddpg.npz`` through ``_run_det_agent`` on both
  routes;
* the default smoothing function: the value target bit for bit and the device generator's state equal
  between the routes, eager and captured.

A recording proxy in front of the library counts the calls of the entry points (tests/test_a2c_agent.py).

The fixtures' critics are ``Linear(27, 32) - ReLU - Linear(32, 1)``: one hidden layer.
``nn.twin_mlp.twin_plan`` admits two hidden layers only, so on the fixtures the two critics run one
after the other (asserted: ``twin_plan`` returns None, ``pfrl_linear_fwd_twin`` is never called) and the
twin route is exercised on critics of the admitted shape in
``test_admitted_critics_run_twinned_and_match_the_composite_route``.

The gradient condition (COVERAGE rows a26-a29): for every parameter tensor, with ref the float64 replica's
gradient,  max |fused - ref| <= max(4 max |composite - ref|, 8 u max |ref|),  u = 2^-24.
"""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pfrl_amd import _native
from test_a2c_agent import _RecordingLib, _assert_gradient_condition
from test_teacher_forced_loss import GOLDEN, TOL, _check_ddpg, _check_td3, _load_flat  # noqa: F401

gpu = pytest.mark.gpu
CRITIC, BWD, NEG, SMOOTH, TWIN = ("pfrl_td3_critic_loss", "pfrl_td3_critic_loss_bwd", "pfrl_neg_mean",
                                  "pfrl_td3_smooth_action", "pfrl_linear_fwd_twin")
LAUNCHES = (CRITIC, BWD, NEG, SMOOTH)


@pytest.fixture
def recorder(monkeypatch):
    if not _native.available():
        _native.build()
    rec = _RecordingLib(_native.lib())
    monkeypatch.setattr(_native, "_lib", rec)
    return rec


def _none_of(recorder, names=LAUNCHES):
    return not [c for c in recorder.calls if c in names]


# ------------------------------------------------------------------ float64 replicas
def _f64(m):
    m = copy.deepcopy(m).cpu().double()
    for p in m.parameters():
        p.grad = None
        p.requires_grad_(True)
    return m


def _b64(batch):
    return {k: v.detach().cpu().double() for k, v in batch.items() if torch.is_tensor(v)}


def _replica_td3(ag, batch, which):
    """The gradient of the reference's expression (pfrl/agents/td3.py:191-211, 238-242) from float64 CPU
    copies of the networks as they are when ``which``'s backward has just run."""
    b = _b64(batch)
    if which == "policy":
        pol, q1 = _f64(ag.policy), _f64(ag.q_func1)
        (-torch.mean(q1((b["state"], pol(b["state"]).rsample())))).backward()
        return [p.grad.clone() for p in pol.parameters()]
    tp, t1, t2 = _f64(ag.target_policy), _f64(ag.target_q_func1), _f64(ag.target_q_func2)
    with torch.no_grad():
        na = ag.target_policy_smoothing_func(tp(b["next_state"]).sample())
        nq = torch.min(t1((b["next_state"], na)), t2((b["next_state"], na)))
        target = b["reward"] + b["discount"] * (1.0 - b["is_state_terminal"]) * torch.flatten(nq)
    q = _f64(ag.q_func1 if which == "q1" else ag.q_func2)
    F.mse_loss(target, torch.flatten(q((b["state"], b["action"])))).backward()
    return [p.grad.clone() for p in q.parameters()]


def _replica_ddpg(ag, batch, which):
    b = _b64(batch)
    n = b["reward"].shape[0]
    if which == "policy":
        pol, q = _f64(ag.policy), _f64(ag.q_function)
        (-q((b["state"], pol(b["state"]).rsample())).mean()).backward()
        return [p.grad.clone() for p in pol.parameters()]
    tp, tq = _f64(ag.target_policy), _f64(ag.target_q_function)
    with torch.no_grad():
        nq = tq((b["next_state"], tp(b["next_state"]).sample()))
        target = b["reward"] + ag.gamma * (1.0 - b["is_state_terminal"]) * nq.reshape((n,))
    q = _f64(ag.q_function)
    F.mse_loss(target, q((b["state"], b["action"])).reshape((n,))).backward()
    return [p.grad.clone() for p in q.parameters()]


def _watch(ag, seen, modules, replica):
    """Every reducer's ``all_reduce`` runs right after its module's backward and before clipping and the
    optimizer step on both routes: record the float32 gradient there, next to the replica's."""
    cur = {}
    orig_impl = ag._update_impl

    def impl(batch, *a, **k):
        cur["batch"] = batch
        return orig_impl(batch, *a, **k)

    ag._update_impl = impl
    for which, module in modules.items():
        red = ag._reducers[module]

        def all_reduce(_orig=red.all_reduce, _which=which, _module=module):
            _orig()
            got = [p.grad.detach().cpu().double() for p in _module.parameters()]
            seen.append((got, replica(ag, cur["batch"], _which)))

        red.all_reduce = all_reduce
    return ag


def _factory(monkeypatch, kind, state):
    from pfrl_amd import agents

    real = getattr(agents, kind)

    def make(*a, **k):
        k.update(state.get("kw", {}))
        ag = real(*a, **k)
        if state.get("cls") is not None:
            ag.__class__ = state["cls"]
        if kind == "TD3":
            mods = {"q1": ag.q_func1, "q2": ag.q_func2, "policy": ag.policy}
            _watch(ag, state["seen"], mods, _replica_td3)
        else:
            _watch(ag, state["seen"], {"q": ag.q_function, "policy": ag.policy}, _replica_ddpg)
        state["made"].append(ag)
        return ag

    monkeypatch.setattr(agents, kind, make)


def _errors(seen):
    return [[(float((g - r).abs().max()), float(r.abs().max())) for g, r in zip(got, ref)]
            for got, ref in seen]


def _fixture_batch(kind, k, dev):
    g = np.load(os.path.join(GOLDEN, "teacher_forced_%s.npz" % kind))
    return {key: torch.as_tensor(g["u%d_%s" % (k, key)]).to(dev)
            for key in ("state", "action", "reward", "next_state", "is_state_terminal", "discount")}


# ================================================================== teacher-forced
@gpu
def test_teacher_forced_td3_update_on_both_routes(monkeypatch, recorder):
    from pfrl_amd.nn.twin_mlp import twin_plan

    g = np.load(os.path.join(GOLDEN, "teacher_forced_td3.npz"))
    n_updates = len(g["updates"])
    n_policy = sum(int(g["u%d_with_policy" % k]) for k in g["updates"])
    runs, state = {}, {}
    _factory(monkeypatch, "TD3", state)
    for fused in (True, False):
        state.update(kw={"fused_loss": fused}, made=[], seen=[], cls=None)
        before = list(recorder.calls)
        _check_td3(0, use_graphs=False)                     # (asserts 1e-5 against the fixture)
        calls = recorder.calls[len(before):]
        count = lambda name: sum(1 for c in calls if c == name)
        assert count(CRITIC) == (n_updates if fused else 0), "one critic launch per update when fused"
        assert count(NEG) == (n_policy if fused else 0), "one actor-loss launch per policy update"
        assert count(SMOOTH) == 0, "the fixture's smoothing function is not the default one"
        assert count(BWD) == 0, "the unit gradient came from the forward launch"
        (ag,) = state["made"]
        assert ag.fused_loss is fused and len(state["seen"]) == 2 * n_updates + n_policy
        # the fixture's critics have ONE hidden layer: outside twin_plan (module docstring)
        b = _fixture_batch("td3", int(g["updates"][0]), ag.device)
        assert twin_plan(ag.q_func1, ag.q_func2, (b["state"], b["action"])) is None
        assert count(TWIN) == 0
        runs[fused] = _errors(state["seen"])
    _assert_gradient_condition("td3", runs[True], runs[False])


@gpu
def test_teacher_forced_ddpg_update_on_both_routes(monkeypatch, recorder):
    g = np.load(os.path.join(GOLDEN, "teacher_forced_ddpg.npz"))
    n_updates = len(g["updates"])
    runs, state = {}, {}
    _factory(monkeypatch, "DDPG", state)
    for fused in (True, False):
        state.update(kw={"fused_loss": fused}, made=[], seen=[], cls=None)
        before = len(recorder.calls)
        _check_ddpg(0, use_graphs=False)
        calls = recorder.calls[before:]
        count = lambda name: sum(1 for c in calls if c == name)
        assert count(CRITIC) == (n_updates if fused else 0) and count(NEG) == (n_updates if fused else 0)
        assert count(SMOOTH) == 0 and count(BWD) == 0
        assert len(state["seen"]) == 2 * n_updates
        runs[fused] = _errors(state["seen"])
    _assert_gradient_condition("ddpg", runs[True], runs[False])


def test_host_agents_never_reach_the_launches(monkeypatch, recorder):
    for kind, check in (("TD3", _check_td3), ("DDPG", _check_ddpg)):
        state = {"kw": {"fused_loss": True}, "made": [], "seen": [], "cls": None}
        _factory(monkeypatch, kind, state)
        check(-1)
        assert state["made"][0].fused_loss and state["made"][0].device.type == "cpu"
    assert _none_of(recorder)


@gpu
def test_subclasses_that_override_a_method_keep_its_torch_expression(monkeypatch, recorder):
    from pfrl_amd import agents

    real_td3, real_ddpg = agents.TD3, agents.DDPG

    class QMine(real_td3):
        def update_q_func(self, batch):
            return real_td3.update_q_func(self, batch)

    class BothMine(QMine):
        def update_policy(self, batch):
            return real_td3.update_policy(self, batch)

    class Plain(real_td3):
        pass

    class CriticMine(real_ddpg):
        def compute_critic_loss(self, batch):
            return real_ddpg.compute_critic_loss(self, batch)

    class DBothMine(CriticMine):
        def compute_actor_loss(self, batch):
            return real_ddpg.compute_actor_loss(self, batch)

    class DPlain(real_ddpg):
        pass

    for kind, check, cases in (
            ("TD3", _check_td3, ((QMine, {NEG}), (BothMine, set()), (Plain, {CRITIC, NEG}))),
            ("DDPG", _check_ddpg, ((CriticMine, {NEG}), (DBothMine, set()), (DPlain, {CRITIC, NEG})))):
        for cls, expected in cases:
            state = {"kw": {"fused_loss": True}, "made": [], "seen": [], "cls": cls}
            with monkeypatch.context() as mp:
                _factory(mp, kind, state)
                before = len(recorder.calls)
                check(0, use_graphs=False)
            assert type(state["made"][0]) is cls
            assert {c for c in recorder.calls[before:] if c in LAUNCHES} == expected, cls.__name__


@gpu
def test_float64_parameters_keep_the_torch_expressions(recorder):
    ag = _small_td3(True, default_smoothing=True)
    for m in ag._graph_modules():
        m.double()
    batch = {k: v.double() for k, v in _small_batch(ag.device).items()}
    ag._update_impl(batch, True)
    torch.cuda.synchronize()
    assert _none_of(recorder)
    assert all(p.dtype == torch.float64 and bool(torch.isfinite(p).all()) for p in ag.q_func1.parameters())


# ================================================================== small agents of the admitted shape
OBS, ACT, MB = 24, 3, 16


def _small_td3(fused, default_smoothing, use_graphs=False, seed=11, twin=True, adam=False):
    import pfrl_amd as pfrl
    from pfrl_amd import agents, explorers, replay_buffers
    from pfrl_amd.agents.td3 import default_target_policy_smoothing_func
    from test_agent_parity import _shifted_smoothing

    torch.manual_seed(seed)
    policy = torch.nn.Sequential(
        torch.nn.Linear(OBS, 32), torch.nn.ReLU(), torch.nn.Linear(32, ACT),
        pfrl.nn.BoundByTanh(low=-np.ones(ACT, dtype=np.float32), high=np.ones(ACT, dtype=np.float32)),
        pfrl.policies.DeterministicHead())

    def q():
        layers = [pfrl.nn.ConcatObsAndAction(), torch.nn.Linear(OBS + ACT, 32), torch.nn.ReLU()]
        if twin:
            layers += [torch.nn.Linear(32, 32), torch.nn.ReLU()]
        return torch.nn.Sequential(*layers, torch.nn.Linear(32, 1))

    q1, q2 = q(), q()
    if adam:
        from pfrl_amd.optimizers import FusedAdam

        opts = [FusedAdam(m.parameters(), lr=1e-3) for m in (policy, q1, q2)]
    else:
        opts = [torch.optim.SGD(m.parameters(), lr=1e-2) for m in (policy, q1, q2)]
    smoothing = default_target_policy_smoothing_func if default_smoothing else _shifted_smoothing
    return agents.TD3(policy, q1, q2, opts[0], opts[1], opts[2], replay_buffers.ReplayBuffer(500),
                      gamma=0.99, explorer=explorers.AdditiveGaussian(scale=0.1, low=-1.0, high=1.0),
                      gpu=0, replay_start_size=40, minibatch_size=MB, update_interval=1,
                      soft_update_tau=5e-3, policy_update_delay=2, target_policy_smoothing_func=smoothing,
                      use_graphs=use_graphs, fused_loss=fused)


def _small_batch(dev, seed=3):
    g = torch.Generator().manual_seed(seed)
    b = {"state": torch.randn(MB, OBS, generator=g), "action": torch.rand(MB, ACT, generator=g) * 2 - 1,
         "reward": torch.randn(MB, generator=g), "next_state": torch.randn(MB, OBS, generator=g),
         "is_state_terminal": (torch.rand(MB, generator=g) < 0.2).float(),
         "discount": torch.full((MB,), 0.99) ** torch.randint(1, 4, (MB,), generator=g).float()}
    return {k: v.to(dev) for k, v in b.items()}


def _flat(*modules):
    return np.concatenate([p.detach().cpu().numpy().ravel() for m in modules for p in m.parameters()])


def _losses_of(ag):
    seen = {}
    orig = ag._record_stats

    def spy(st):
        orig(st)
        for k, v in st.items():
            if "loss" in k:
                seen.setdefault(k, []).extend(float(x) for x in v.detach().reshape(-1).cpu())

    ag._record_stats = spy
    return seen


@gpu
@pytest.mark.parametrize("adam", [False, True])
def test_admitted_critics_run_twinned_and_match_the_composite_route(recorder, adam):
    from pfrl_amd.nn.twin_mlp import twin_plan

    out = {}
    for fused in (True, False):
        ag = _small_td3(fused, default_smoothing=False, adam=adam)
        b = _small_batch(ag.device)
        assert twin_plan(ag.q_func1, ag.q_func2, (b["state"], b["action"])) is not None
        assert twin_plan(ag.target_q_func1, ag.target_q_func2, (b["next_state"], b["action"])) is not None
        seen = _losses_of(ag)
        before = len(recorder.calls)
        for step in range(4):
            ag._update_impl(_small_batch(ag.device, seed=step), step % 2 == 1)
        calls = recorder.calls[before:]
        # two twinned passes (target pair, online pair) of two wide layers each per update
        assert sum(1 for c in calls if c == TWIN) == (4 * 2 * 2 if fused else 0)
        assert sum(1 for c in calls if c == CRITIC) == (4 if fused else 0)
        assert sum(1 for c in calls if c == NEG) == (2 if fused else 0)
        out[fused] = (seen, _flat(ag.policy, ag.q_func1, ag.q_func2, ag.target_q_func1))
    for k in out[True][0]:
        np.testing.assert_allclose(out[True][0][k], out[False][0][k], rtol=TOL, atol=TOL)
    np.testing.assert_allclose(out[True][1], out[False][1], rtol=1e-4 if adam else TOL, atol=TOL)


# ================================================================== the default smoothing function
def _hooked_targets(monkeypatch, ag, sink):
    """The value target of every ``update_q_func``: what ``critic_losses`` computes on the fused route,
    what ``F.mse_loss`` receives first on the composite one."""
    from pfrl_amd.agents import _td3_losses

    orig_cl, orig_mse = _td3_losses.critic_losses, F.mse_loss

    def critic_losses(*a, **k):
        losses, target = orig_cl(*a, with_target=True, **k)
        sink.append(("fused", target))
        return losses

    def mse_loss(inp, tgt, *a, **k):
        if not sink or sink[-1][0] != "composite-first":
            sink.append(("composite-first", inp))
        else:
            sink[-1] = ("composite", sink[-1][1])
        return orig_mse(inp, tgt, *a, **k)

    monkeypatch.setattr(_td3_losses, "critic_losses", critic_losses)
    monkeypatch.setattr(F, "mse_loss", mse_loss)


@gpu
@pytest.mark.parametrize("use_graphs", [False, True])
def test_default_smoothing_gives_the_same_target_bits_and_generator_state(monkeypatch, recorder, use_graphs):
    from pfrl_amd.agents.graphed_update import CapturedStep

    dev = torch.device("cuda:0")
    results = {}
    for fused in (True, False):
        # (one-hidden-layer critics: both routes evaluate the target critics one after the other, so
        # the target depends on the route through the smoothing and the target arithmetic only)
        ag = _small_td3(fused, default_smoothing=True, use_graphs=use_graphs, twin=False)
        sink, targets, states = [], [], []
        with monkeypatch.context() as mp:
            _hooked_targets(mp, ag, sink)
            batch = _small_batch(dev)
            if use_graphs:
                step = CapturedStep(ag._update_core, ag._graph_modules(), ag._graph_optimizers(), dev)
            for k in range(3):
                torch.cuda.manual_seed(1234 + k)
                before = len(recorder.calls)
                if use_graphs:
                    step.run(batch, False)          # k = 0 captures; sink[-1] is the graph's own tensor
                    torch.cuda.synchronize()
                    if k == 0:                      # the launch is seen while the graph is captured
                        assert (SMOOTH in recorder.calls[before:]) == fused
                else:
                    ag.update_q_func(batch)
                    assert sum(1 for c in recorder.calls[before:] if c == SMOOTH) == (1 if fused else 0)
                targets.append(sink[-1][1].detach().clone())
                states.append(torch.cuda.get_rng_state(dev).clone())
        assert all(t.shape == (MB,) for t in targets)
        assert not torch.equal(targets[0], targets[1]), "the seed does not reach the draw"
        results[fused] = (targets, states, _flat(ag.q_func1, ag.q_func2))
    (tf, sf, pf), (tc, sc, pc) = results[True], results[False]
    assert len(tf) == len(tc)
    for a, b in zip(tf, tc):
        assert torch.equal(a, b), "target_q differs between the routes"
    assert all(torch.equal(a, b) for a, b in zip(sf, sc)), "the device generator advanced differently"
    np.testing.assert_allclose(pf, pc, rtol=TOL, atol=TOL)


# ================================================================== recorded rollouts
@gpu
@pytest.mark.parametrize("kind", ["td3", "ddpg"])
def test_recorded_rollout_on_both_routes(kind, recorder):
    from test_agent_parity import _run_det_agent

    a = _run_det_agent(kind, 0, use_graphs=False, fused_loss=True)
    n_critic = recorder.count(CRITIC)
    b = _run_det_agent(kind, 0, use_graphs=False, fused_loss=False)
    assert n_critic == len(a["losses"]) > 0 and recorder.count(CRITIC) == n_critic
    assert np.array_equal(a["actions"], b["actions"])
    print("largest loss difference between the routes", np.abs(a["losses"] - b["losses"]).max())
    np.testing.assert_allclose(a["losses"], b["losses"], rtol=TOL, atol=TOL)
    np.testing.assert_allclose(a["stats"], b["stats"], rtol=TOL, atol=TOL)


# ================================================================== captured against eager
@gpu
@pytest.mark.parametrize("kind", ["td3", "ddpg"])
def test_captured_fused_update_matches_the_eager_one(kind, recorder):
    from test_agent_parity import _run_det_agent

    eager = _run_det_agent(kind, 0, use_graphs=False, fused_loss=True)
    before = len(recorder.calls)
    graph = _run_det_agent(kind, 0, use_graphs=True, fused_loss=True)
    ag = graph["agent"]
    assert ag.use_graphs and ag._captured is not None
    assert len(ag._captured.graphs) >= (2 if kind == "td3" else 1)         # both TD3 step shapes
    seen = set(recorder.calls[before:])
    assert CRITIC in seen and NEG in seen, "the kernels are launched while the graphs are captured"
    assert np.array_equal(graph["actions"], eager["actions"])
    np.testing.assert_allclose(graph["losses"], eager["losses"], rtol=TOL, atol=TOL)
    for k in ("policy_params", "critic_params", "target_critic_params"):
        np.testing.assert_allclose(graph[k], eager[k], rtol=TOL, atol=TOL)


# ================================================================== save / load
@gpu
def test_save_load_round_trip_and_the_next_update(tmp_path):
    ag = _small_td3(True, default_smoothing=True, adam=True)
    dev = ag.device
    torch.cuda.manual_seed(5)
    ag._update_impl(_small_batch(dev, 0), True)
    ag.save(str(tmp_path / "agent"))
    other = _small_td3(True, default_smoothing=True, adam=True, seed=99)
    other.load(str(tmp_path / "agent"))
    mods = lambda a: (a.policy, a.q_func1, a.q_func2, a.target_policy, a.target_q_func1, a.target_q_func2)
    assert np.array_equal(_flat(*mods(other)), _flat(*mods(ag)))
    for a in (ag, other):
        torch.cuda.manual_seed(6)
        a._update_impl(_small_batch(dev, 1), True)
    assert np.array_equal(_flat(*mods(other)), _flat(*mods(ag)))


def test_constructors_take_fused_loss_after_use_graphs():
    import inspect

    from pfrl_amd import agents

    for cls in (agents.TD3, agents.DDPG):
        names = list(inspect.signature(cls.__init__).parameters)
        assert names[-2:] == ["use_graphs", "fused_loss"]
        assert inspect.signature(cls.__init__).parameters["fused_loss"].default is True
