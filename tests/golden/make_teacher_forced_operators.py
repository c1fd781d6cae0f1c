#!/usr/bin/env python
"""Teacher-forced loss fixtures of the six operator agents (AL, PAL, DoublePAL, DPP, DPPL,
DPPGreedy), recorded by running the REFERENCE (pfnet/pfrl) itself.

    python tests/golden/make_teacher_forced_operators.py   (build container only: needs the reference)

The method of make_teacher_forced.py (whose helpers this script imports): the six runs of
``make_golden.DQN_FAMILY`` again -- same seeds, same environment, the losses asserted equal to the
committed ``agent_trace_*.npz`` -- recording for updates {1, 50, 140} the online and target
parameters BEFORE the update, the ``exp_batch`` handed to ``_compute_loss`` and the loss the
reference computed.  States are stored as the u8 frames they came from (``phi`` is /255, exact).

Output: tests/golden/teacher_forced_{al,pal,double_pal,dpp,dppl,dpp_greedy}.npz
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_golden as mg  # noqa: E402  (puts the reference and the gym shim on sys.path)
import make_teacher_forced as mtf  # noqa: E402


def family(name, agent_cls, agent_kw, steps=640, N=4):
    """make_golden.agent_trace(name, False, 1, False, agent_cls=..., **agent_kw) with the recorder
    of make_teacher_forced on ``_compute_loss``."""
    import tempfile

    import pfrl
    from pfrl import agents, explorers, experiments, replay_buffers
    from pfrl.q_functions import DiscreteActionValueHead

    sys.path.insert(0, os.path.join(HERE, "..", ".."))
    from pfrl_amd.envs.synthetic import HostSyntheticAtariVectorEnv

    pfrl.utils.set_random_seed(0)
    env = HostSyntheticAtariVectorEnv(N, seed=3, frame_shape=(12, 12), p_done=0.04)

    def phi(x):
        return np.asarray(x, dtype=np.float32) / 255

    q = mg.make_q_function(4 * 144, 6, DiscreteActionValueHead())
    opt = torch.optim.RMSprop(q.parameters(), lr=2.5e-4, alpha=0.95, eps=1e-2)
    rbuf = replay_buffers.ReplayBuffer(200, num_steps=1)
    ex = explorers.LinearDecayEpsilonGreedy(1.0, 0.1, 400, lambda: np.random.randint(6))
    cls = getattr(agents, agent_cls, None) or getattr(agents.dpp, agent_cls)
    ag = cls(q, opt, rbuf, 0.99, ex, gpu=-1, replay_start_size=40, minibatch_size=8,
             update_interval=4, target_update_interval=60, phi=phi, batch_accumulator="sum",
             **agent_kw)
    out = {}
    mtf.record(ag, out)
    losses = []
    orig_update = ag.update

    def spy_update(exps, errors_out=None):
        orig_update(exps, errors_out)
        losses.append(ag.loss_record[-1])

    ag.replay_updater.update_func = spy_update
    experiments.train_agent_batch(ag, env, steps, tempfile.mkdtemp())
    for k in mtf.UPDATES:
        for key in ("state", "next_state"):
            out["u%d_%s" % (k, key)] = mtf._as_u8(out["u%d_%s" % (k, key)])
    mtf.finish(name, out, losses)      # asserts: the run of agent_trace_<name>.npz, bit for bit
    size = os.path.getsize(os.path.join(HERE, "teacher_forced_%s.npz" % name))
    assert size <= os.path.getsize(os.path.join(HERE, "teacher_forced_dqn_uniform_n1.npz")), size


if __name__ == "__main__":
    wanted = sys.argv[1:]
    for name, agent_cls, agent_kw in mg.DQN_FAMILY:
        if not wanted or name in wanted:
            family(name, agent_cls, agent_kw)
