"""``explorers.Boltzmann`` on the device step of the DQN family (agents/_dqn_device_step.py), on the
agent ``bench.py`` builds at 32 envs with updates running, following
``test_dqn_act_graph_and_fused_head_equal_the_eager_act_path`` of tests/test_bench_path_parity.py:
the captured graph with the fused head, the two-launch form (``PFRL_DQN_ACT_HEAD=0``) and the eager
launches (``PFRL_DQN_ACT_GRAPH=0``) are one computation -- actions of every step, parameters and
the final NumPy state are identical -- and the per-env branch of ``DQN.batch_act`` (the reference's
loop: a softmax, a device-to-host read and one ``np.random.choice`` per env) picks the same actions
from the same stream positions.
"""
import argparse
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

N = 32
SEED = 0


def _bench_args(**kw):
    d = dict(gpus=1, algo="dqn", host_env=False, steps=1, warmup=0, num_envs=N, capacity=3000,
             minibatch=32, update_interval=4, seed=SEED, prefill=None, no_cpu_baseline=True,
             cpu_baseline_seconds=0.0, cpu_baseline_threads=1, cudnn_benchmark=False,
             channels_last=True, blas="default", chunks=None, torch_optimizer=False,
             replay_start=128, frame_slots=12288, slack=512, priority_pow="device")
    d.update(kw)
    return argparse.Namespace(**d)


def _same_rng_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def _run(monkeypatch, steps, schedule, graph=True, head=True, device_step=True, spy=None):
    """``steps`` batched steps of the bench agent; ``schedule(step, agent, state)`` sets the
    explorer before each step.  Returns actions per step, parameters, the final NumPy state, the
    act graph, the steps at which a graph was captured and the number of updates.  (A fresh agent
    captures at steps 0 AND 1: the frame store's output layout, part of the graph's key, is routed
    to the network's inside the first capture.)"""
    import bench
    from pfrl_amd.agents import _dqn_device_step as ds

    monkeypatch.setenv("PFRL_DQN_ACT_GRAPH", "1" if graph else "0")
    monkeypatch.setenv("PFRL_DQN_ACT_HEAD", "1" if head else "0")
    captures, now = [], [None]
    orig_capture = ds.ActGraph._capture

    def counting_capture(self, *a, **kw):
        captures.append(now[0])
        return orig_capture(self, *a, **kw)

    with monkeypatch.context() as patch:        # (undone per leg: a later leg must not count here)
        patch.setattr(ds.ActGraph, "_capture", counting_capture)
        return _steps(bench, steps, schedule, device_step, spy, captures, now)


def _steps(bench, steps, schedule, device_step, spy, captures, now):
    agent, env, _ = bench.build_agent(_bench_args(), torch.device("cuda:0"), 0)
    agent.device_step = bool(device_step)
    state = {"eps": agent.explorer}
    obss = env.reset()
    acts = []
    for step in range(steps):
        now[0] = step
        schedule(step, agent, state)
        if spy is not None:
            spy(agent)
        a = agent.batch_act(obss)
        acts.append(np.asarray(a).astype(np.int64).copy())
        obss2, rs, dones, _ = env.step(a)
        agent.batch_observe(obss2, rs, dones, np.zeros(N, dtype=bool))
        obss = env.reset(~np.asarray(dones))
    agent.get_statistics()                      # (looks at the status words still in flight)
    torch.cuda.synchronize()
    params = [p.detach().cpu().clone() for p in agent.model.parameters()]
    return dict(acts=acts, params=params, rng=np.random.get_state(), graph=agent.__dict__.get("_act_graph"),
                captures=captures, updates=agent.optim_t, device_actions=agent._last_actions_dev is not None)


def _boltzmann(T):
    from pfrl_amd import explorers

    def schedule(step, agent, state):
        if step == 0:
            agent.explorer = explorers.Boltzmann(T)

    return schedule


def test_graph_fused_head_two_launch_and_eager_forms_are_one_computation(monkeypatch):
    steps = 24
    full = _run(monkeypatch, steps, _boltzmann(1.0))
    two = _run(monkeypatch, steps, _boltzmann(1.0), head=False)
    eager = _run(monkeypatch, steps, _boltzmann(1.0), graph=False)
    assert full["graph"] is not None and full["graph"].entries and full["captures"], \
        "the graph path was not taken"
    assert set(full["captures"]) <= {0, 1}, "a later step captured again"
    assert two["graph"] is None and eager["graph"] is None and not two["captures"] and not eager["captures"]
    assert full["updates"] > 100
    for leg in (full, two, eager):
        assert leg["device_actions"], "the actions did not stay on the device"
    # (every action is one of the six, and Boltzmann at T = 1 on a fresh network uses them all)
    allacts = np.concatenate(full["acts"])
    assert allacts.min() >= 0 and allacts.max() <= 5 and len(np.unique(allacts)) == 6
    for other in (two, eager):
        assert other["updates"] == full["updates"]
        for t, (x, y) in enumerate(zip(full["acts"], other["acts"])):
            np.testing.assert_array_equal(x, y, err_msg="step %d" % t)
        assert _same_rng_state(full["rng"], other["rng"])
        for x, y in zip(full["params"], other["params"]):
            assert torch.equal(x, y)


def test_device_step_picks_the_actions_of_the_per_env_branch(monkeypatch):
    """Against ``DQN.batch_act``'s own per-env branch (``device_step`` off), with updates running.
    That branch divides and exponentiates with torch's kernels, so its float32 probabilities differ
    from the device step's in the last bits; the test therefore first checks on that branch's OWN
    action values and draws that no draw lies within 1e-5 of a boundary of the float64 cdf (a
    condition on the inputs -- the seed was picked so that it holds -- not a tolerance on the
    result), then asks for equal actions at every step and the same stream position behind every
    step.

    Both branches act on the SAME agent: at every step the per-env branch runs first from a saved
    NumPy state, the state is put back and the device step takes the step for real.  Two separate
    runs do not serve: with ``device_step`` off the appends and updates take the Python path instead
    of the native planner's, the parameters of the two runs part ways (measured on this set-up:
    1.5e-8 after the first updates, 2e-4 from step 15 on, action values 1e-2 apart at step 16, the
    first different action at step 17) and the legs then sample from different action values --
    whatever the explorer."""
    import bench
    from pfrl_amd import explorers

    steps, T = 24, 1.0
    agent, env, _ = bench.build_agent(_bench_args(), torch.device("cuda:0"), 0)
    ex = agent.explorer = explorers.Boltzmann(T)
    seen, pairs = [], []

    def spying(t, greedy_action_func, action_value=None):
        st = np.random.get_state()
        u = np.random.random_sample()           # the draw choice() is about to make
        np.random.set_state(st)
        seen.append((action_value.q_values.detach().double().cpu().numpy().ravel(), u))
        return explorers.Boltzmann.select_action(ex, t, greedy_action_func, action_value=action_value)

    obss = env.reset()
    for step in range(steps):
        s0 = np.random.get_state()
        agent.device_step, ex.select_action = False, spying
        want = np.asarray(agent.batch_act(obss)).astype(np.int64)
        assert agent._last_actions_dev is None
        s_ref = np.random.get_state()
        np.random.set_state(s0)
        agent.device_step = True
        del ex.select_action
        a = agent.batch_act(obss)
        assert agent._last_actions_dev is not None, "the device step was not taken"
        pairs.append((want, np.asarray(a).astype(np.int64).copy()))
        assert _same_rng_state(np.random.get_state(), s_ref), "step %d" % step
        obss2, rs, dones, _ = env.step(a)
        agent.batch_observe(obss2, rs, dones, np.zeros(N, dtype=bool))
        obss = env.reset(~np.asarray(dones))
    agent.get_statistics()
    assert agent.optim_t > 100 and agent.__dict__["_act_graph"].entries and len(seen) == steps * N
    q = np.stack([s[0] for s in seen])
    u = np.array([s[1] for s in seen])
    z = q / T
    e = np.exp(z - z.max(axis=1, keepdims=True))
    cdf = np.cumsum(e / e.sum(axis=1, keepdims=True), axis=1)[:, :-1]
    gap = np.abs(cdf - u[:, None]).min()
    print("closest draw to a cdf boundary: %.3e" % gap)
    assert gap > 1e-5, "a draw lies within 1e-5 of a cdf boundary (%.3e): pick another seed" % gap
    for step, (want, got) in enumerate(pairs):
        np.testing.assert_array_equal(got, want, err_msg="step %d" % step)


@pytest.mark.parametrize("graph", [True, False])
def test_nan_probabilities_raise_the_reference_error_late(monkeypatch, graph):
    """A NaN action value: ``np.random.choice`` raises ``ValueError("probabilities contain NaN")``
    on the spot, the device step when the step's event is waited for -- on ``get_statistics`` /
    ``stop_episode`` / ``save``, or in the run-ahead loop at most RUN_AHEAD steps later."""
    import bench
    from pfrl_amd import explorers
    from pfrl_amd.agents import _dqn_device_step as ds

    monkeypatch.setenv("PFRL_DQN_ACT_GRAPH", "1" if graph else "0")
    agent, env, _ = bench.build_agent(_bench_args(), torch.device("cuda:0"), 0)
    agent.explorer = explorers.Boltzmann(1.0)
    obss = env.reset()
    a = np.asarray(agent.batch_act(obss))
    assert a.min() >= 0
    agent.get_statistics()                              # nothing pending is wrong
    with torch.no_grad():
        agent.model[len(agent.model) - 2].bias[2] = float("nan")
    for check in (agent.get_statistics, agent.stop_episode):
        a = np.asarray(agent.batch_act(obss))           # (returns: the status word is read later)
        assert (a == -1).all()
        with pytest.raises(ValueError, match="probabilities contain NaN"):
            check()
        check()                                         # reported once
    with pytest.raises(ValueError, match="probabilities contain NaN"):
        for _ in range(ds.RUN_AHEAD + 1):
            agent.batch_act(obss)
    with torch.no_grad():
        agent.model[len(agent.model) - 2].bias[2] = 0.0
    agent.__dict__["_step_events"].clear()              # (the poisoned steps still in flight)
    torch.cuda.synchronize()
    agent._act_status.zero_()
    assert np.asarray(agent.batch_act(obss)).min() >= 0
    agent.get_statistics()


def test_temperature_change_and_explorer_swap_replay_the_right_graphs(monkeypatch):
    """``explorer.T`` changed between steps reaches the captured graph through the staging block
    (no new capture); epsilon-greedy on the live agent is a second graph, and going back to
    Boltzmann replays the first.  The eager launches under the same schedule are the yardstick."""
    from pfrl_amd import explorers

    steps = 16

    def schedule(step, agent, state):
        if step == 0:
            state["boltzmann"] = agent.explorer = explorers.Boltzmann(1.0)
        elif step == 4:
            agent.explorer.T = 0.02
        elif step == 8:
            agent.explorer = state["eps"]
        elif step == 12:
            agent.explorer = state["boltzmann"]

    graph = _run(monkeypatch, steps, schedule)
    eager = _run(monkeypatch, steps, schedule, graph=False)
    control = _run(monkeypatch, 8, _boltzmann(1.0))
    # (captures: the Boltzmann form on the fresh agent, the epsilon-greedy form at step 8 -- none
    # for the new temperature at step 4, none for the way back at step 12)
    assert set(graph["captures"]) <= {0, 1, 8} and 0 in graph["captures"] and 8 in graph["captures"]
    assert eager["graph"] is None and set(control["captures"]) <= {0, 1}
    for t, (x, y) in enumerate(zip(graph["acts"], eager["acts"])):
        np.testing.assert_array_equal(x, y, err_msg="step %d" % t)
    assert _same_rng_state(graph["rng"], eager["rng"])
    for x, y in zip(graph["params"], eager["params"]):
        assert torch.equal(x, y)
    for t in range(4):
        np.testing.assert_array_equal(graph["acts"][t], control["acts"][t])
    assert any(not np.array_equal(graph["acts"][t], control["acts"][t]) for t in range(4, 8)), \
        "the new temperature did not reach the graph"
