#!/usr/bin/env python
"""DDPG with Ornstein-Uhlenbeck exploration on the host-side synthetic vector-observation env, `pfrl`
replaced by `pfrl_amd`: the agent of the reference's examples/mujoco/reproduction/ddpg/train_ddpg.py
(400-300 MLPs, `BoundByTanh`, `AdditiveOU(sigma=0.2)`, Adam, soft target updates) at Humanoid's shape
(376 floats in, 17 action dimensions).

On the GPU a batched acting step is one pinned transfer -- the observations and the explorer's noise rows,
drawn on the host exactly as the reference's per-env `select_action` loop draws them -- one captured
graph that ends in one launch for the policy's last layer, `BoundByTanh` and the noise
(`pfrl_deterministic_head_act`, agents/_actor_device_step.py), and one copy back.  ``--no-device-act``
keeps the agent's own acting code (`PFRL_ACTOR_ACT_HEAD=0`).

``--time-acts K`` does not train: it times K batched acting steps (after a warm-up), five repeats, and
prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pfrl_amd as pfrl  # noqa: E402
from pfrl_amd import agents, explorers, replay_buffers, utils  # noqa: E402

OBS, ACT = 376, 17


def parse_args(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("--no-device-act", action="store_true", default=False)
    parser.add_argument("--gpu", type=int, default=0)
    parser.add_argument("--num-envs", type=int, default=16)
    parser.add_argument("--minibatch-size", type=int, default=100)
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--steps", type=int, default=2 * 10 ** 4)
    parser.add_argument("--replay-start-size", type=int, default=1000)
    parser.add_argument("--time-acts", type=int, default=0)
    return parser.parse_args(argv)


def make_agent(args):
    from pfrl_amd.optimizers import FusedAdam

    policy = nn.Sequential(nn.Linear(OBS, 400), nn.ReLU(), nn.Linear(400, 300), nn.ReLU(), nn.Linear(300, ACT),
                           pfrl.nn.BoundByTanh(low=-np.ones(ACT, dtype=np.float32),
                                               high=np.ones(ACT, dtype=np.float32)),
                           pfrl.policies.DeterministicHead())
    q = nn.Sequential(pfrl.nn.ConcatObsAndAction(), nn.Linear(OBS + ACT, 400), nn.ReLU(), nn.Linear(400, 300),
                      nn.ReLU(), nn.Linear(300, 1))
    Adam = (lambda ps: FusedAdam(ps, lr=3e-4)) if args.gpu >= 0 else (lambda ps: torch.optim.Adam(ps, lr=3e-4))
    return agents.DDPG(policy, q, Adam(policy.parameters()), Adam(q.parameters()),
                       replay_buffers.ReplayBuffer(10 ** 5), gamma=0.99, explorer=explorers.AdditiveOU(sigma=0.2),
                       gpu=args.gpu, replay_start_size=args.replay_start_size,
                       minibatch_size=args.minibatch_size, update_interval=1, target_update_interval=1,
                       target_update_method="soft", soft_update_tau=5e-3)


def time_acts(agent, args, repeats=5, warmup=30):
    from pfrl_amd.agents import _actor_device_step

    rs = np.random.RandomState(args.seed)
    obs = [rs.standard_normal(OBS).astype(np.float32) for _ in range(args.num_envs)]
    for _ in range(warmup):
        agent.batch_act(obs)
    us = []
    calls0 = _actor_device_step.calls
    for _ in range(repeats):
        if args.gpu >= 0:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.time_acts):
            agent.batch_act(obs)
        us.append(1e6 * (time.perf_counter() - t0) / args.time_acts)
    print(json.dumps(dict(agent="ddpg", explorer=repr(agent.explorer), envs=args.num_envs, acts=args.time_acts,
                          device_act_steps=_actor_device_step.calls - calls0,
                          us_per_act=[round(u, 2) for u in us], median_us=round(float(np.median(us)), 2))))


def main():
    args = parse_args()
    if args.no_device_act:
        os.environ["PFRL_ACTOR_ACT_HEAD"] = "0"
    utils.set_random_seed(args.seed)
    agent = make_agent(args)
    if args.time_acts:
        time_acts(agent, args)
        return
    import tempfile

    from pfrl_amd.envs.synthetic import HostSyntheticVectorObsEnv

    env = HostSyntheticVectorObsEnv(args.num_envs, obs_dim=OBS, act_dim=ACT, seed=args.seed)
    pfrl.experiments.train_agent_batch(agent, env, args.steps, tempfile.mkdtemp(prefix="ddpg_ou_"),
                                       log_interval=10 ** 9)
    print("env steps %d  %s" % (args.steps, agent.get_statistics()))


if __name__ == "__main__":
    main()
