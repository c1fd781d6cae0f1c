"""ops.lstm_sequence against nn.LSTM in float64, and who reaches it: containers only inside nn.recurrent.first_order_sequences,
which the DQN family's and PPO's recurrent updates enter and TRPO does not.  Yardstick as test_lstm_sequence.py: nn.LSTM in float32
on the CPU against nn.LSTM in float64; the route may err twice as much."""
import copy
import tempfile

import numpy as np
import pytest
import torch
from test_lstm_route import _container
from torch import nn
from torch.nn.utils.rnn import PackedSequence, pack_sequence

import pfrl_amd
from pfrl_amd import agents, experiments, explorers, ops
from pfrl_amd.nn.recurrent import first_order_sequences

pytestmark = pytest.mark.gpu
NAMES = ("Y", "hn", "cn", "dX", "dh0", "dW_ih", "dW_hh", "db_ih", "db_hh")


@pytest.fixture
def calls(monkeypatch):
    seen, orig = [], ops.lstm_sequence
    monkeypatch.setattr(ops, "lstm_sequence", lambda *a, **k: seen.append(list(a[1])) or orig(*a, **k))
    return seen


@pytest.mark.parametrize("sizes,I,H", [([5, 3, 3, 1], 6, 4), ([17, 16, 1], 36, 20)])
def test_lstm_sequence_against_nn_lstm_in_float64(sizes, I, H):
    torch.manual_seed(H)
    ref, (R, n0) = nn.LSTM(I, H), (sum(sizes), sizes[0])
    x, h0, c0, wy, wh, wc = (torch.randn(s) for s in ((R, I), (n0, H), (n0, H), (R, H), (n0, H), (n0, H)))
    res = []
    for dtype, dev in ((torch.float64, "cpu"), (torch.float32, "cpu"), (torch.float32, "cuda")):
        m = copy.deepcopy(ref).to(dev, dtype)
        xl, hl, c = x.to(dev, dtype).requires_grad_(), h0.to(dev, dtype).requires_grad_(), c0.to(dev, dtype)
        if dev == "cuda":
            y, hn, cn = ops.lstm_sequence(xl, sizes, hl, c, m.weight_ih_l0, m.weight_hh_l0, m.bias_ih_l0, m.bias_hh_l0)
        else:
            out, (hn, cn) = m(PackedSequence(xl, torch.tensor(sizes)), (hl[None], c[None]))
            y, hn, cn = out.data, hn[0], cn[0]
        obj = (y * wy.to(y)).sum() + (hn * wh.to(y)).sum() + (cn * wc.to(y)).sum()
        grads = torch.autograd.grad(obj, [xl, hl] + list(m.parameters()))      # (weight_ih, weight_hh, bias_ih, bias_hh)
        res.append([t.detach().cpu().double() for t in (y, hn, cn, *grads)])
    for name, want, f32, got in zip(NAMES, *res):
        yard, err = float((f32 - want).abs().max()), float((got - want).abs().max())
        print("LSTM sequence route %s %s nn.LSTM_f32_max_err %.3e route_max_err %.3e" % (sizes, name, yard, err))
        assert err <= 2 * yard, (name, err, yard)


def test_a_second_backward_raises():
    m, x = nn.LSTM(4, 4).cuda(), torch.randn(3, 4, device="cuda", requires_grad=True)
    y, _, _ = ops.lstm_sequence(x, [2, 1], None, None, *m.parameters())
    (g,) = torch.autograd.grad(y.sum(), x, create_graph=True)
    with pytest.raises(RuntimeError):
        torch.autograd.grad(g.sum(), x)


@pytest.mark.parametrize("lens", [[3, 2, 2], [1] * 4], ids=["sequences", "one-step-with-gradients"])
def test_a_container_takes_the_route_only_inside_the_context(lens, calls, monkeypatch):
    net = _container().cuda()
    packed = pack_sequence([torch.randn(n, 6, device="cuda") for n in lens])
    net(packed, None)
    assert not calls
    with first_order_sequences():
        net(packed, None)
        monkeypatch.setenv("PFRL_LSTM_SEQ", "0")
        net(packed, None)
    assert calls == [packed.batch_sizes.tolist()]


def test_a_drqn_update_makes_three_calls_and_matches_the_library_update(calls, monkeypatch):
    """Bound: rtol 1e-4, atol 1e-6 on the loss and every parameter after the step, the tolerance at which test_episodic_recurrent.py
    holds this agent's update to a trace recorded with another (CPU) LSTM implementation: both sides here are f32 LSTMs of that accuracy."""
    def agent():
        q = _container(tail=[pfrl_amd.q_functions.DiscreteActionValueHead()])
        return agents.DoubleDQN(q, torch.optim.SGD(q.parameters(), lr=0.1), pfrl_amd.replay_buffers.EpisodicReplayBuffer(1000), 0.9,
                                explorers.ConstantEpsilonGreedy(0.1, lambda: 0), gpu=0, recurrent=True, replay_start_size=500)
    ag = agent()
    for t in range(12):     # three environments, one episode boundary: a few short episodes with stored states
        obs = [np.full(6, 0.1 * (t + i), np.float32) for i in range(3)]
        ag.batch_act(obs)
        ag.batch_observe(obs, [float(t % 3)] * 3, [t == 5, t == 10, t == 8], [False] * 3)
    episodes = ag.replay_buffer.sample_episodes(3, max_len=4)
    out = []
    for env, n_calls in (("1", 3), ("0", 0)):
        monkeypatch.setenv("PFRL_LSTM_SEQ", env)
        ag, before = agent(), len(calls)
        ag.update_from_episodes(list(episodes))
        assert len(calls) - before == n_calls
        out.append(np.concatenate([[float(ag.loss_record.values()[-1])]] + [p.detach().cpu().numpy().ravel() for p in ag.model.parameters()]))
    print("DRQN update: route against library, max abs difference of loss and parameters %.3e" % np.abs(out[0] - out[1]).max())
    np.testing.assert_allclose(out[0], out[1], rtol=1e-4, atol=1e-6)


def test_a_recurrent_ppo_update_enters_the_route(calls):
    from pfrl_amd.envs.synthetic import HostSyntheticAtariVectorEnv
    torch.manual_seed(1)
    model = pfrl_amd.nn.RecurrentSequential(
        nn.Flatten(), nn.Linear(4 * 144, 32), nn.ReLU(), nn.LSTM(32, 16),
        pfrl_amd.nn.Branched(nn.Sequential(nn.Linear(16, 6), pfrl_amd.policies.SoftmaxCategoricalHead()), nn.Linear(16, 1)))
    ag = agents.PPO(model, torch.optim.SGD(model.parameters(), lr=1e-2), gpu=0, phi=lambda x: np.asarray(x, np.float32) / 255,
                    update_interval=16, minibatch_size=16, epochs=1, recurrent=True)
    env = HostSyntheticAtariVectorEnv(4, seed=5, frame_shape=(12, 12), p_done=0.0)
    experiments.train_agent_batch(ag, env, 6 * 4, tempfile.mkdtemp())
    assert ag.n_updates == 1 and calls == [[4] * 4] * 3     # two value passes over the rollout, one minibatch of four 4-step sequences


def test_a_recurrent_trpo_update_never_enters_the_context(monkeypatch):
    """On the CPU (the library's LSTM has no double backward on the device): none of the update's container calls is inside the context."""
    from test_trpo_cpu import ACT, OBS, _exp2, _run_trace
    from pfrl_amd.nn import recurrent
    inside, orig = [], recurrent.lstm_sequence_or_none
    monkeypatch.setattr(recurrent, "lstm_sequence_or_none", lambda *a: inside.append(getattr(recurrent._route, "sequences", False)) or orig(*a))
    torch.manual_seed(3)
    pi = pfrl_amd.nn.RecurrentSequential(nn.LSTM(OBS, 8), nn.Linear(8, ACT), pfrl_amd.policies.GaussianHeadWithStateIndependentCovariance(
        action_size=ACT, var_type="diagonal", var_func=_exp2, var_param_init=0))
    v = pfrl_amd.nn.RecurrentSequential(nn.LSTM(OBS, 8), nn.Linear(8, 1))
    ag = agents.TRPO(pi, v, torch.optim.Adam(v.parameters(), lr=1e-2), gpu=-1, recurrent=True, update_interval=32, vf_batch_size=16)
    _, updates = _run_trace(ag, 8)
    assert len(updates) == 1 and len(inside) > 16 and not any(inside)
