#!/usr/bin/env python
"""DQN / DoubleDQN with a NAF Q-function and Ornstein-Uhlenbeck exploration on the continuous A-B-C
chain, `pfrl` replaced by `pfrl_amd`: the continuous-action half of the reference's
examples/gym/train_dqn_gym.py (`FCQuadraticStateQFunction`, `AdditiveOU`, Adam) on the toy problem of
the reference's agent tests (`envs.ABC(discrete=False)`).

On the GPU an update ends in ONE launch for everything behind the four `Linear` heads of the online
and the target network -- tanh and scale, exp, the triangular factor, the quadratic forms, the greedy
action in the box, the TD target, the Huber loss and the gradients (`pfrl_naf_td_loss`,
agents/_naf_split.py) -- inside the captured update.  ``--composite`` keeps the stock torch expression
(`PFRL_NAF_FUSED=0`).

``--time-updates K`` does not train: it fills the replay buffer, then times K updates of one minibatch
(after a warm-up), five repeats, and prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pfrl_amd as pfrl  # noqa: E402
from pfrl_amd import agents, explorers, replay_buffers, utils  # noqa: E402


def parse_args(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("--composite", action="store_true", default=False)
    parser.add_argument("--double", action="store_true", default=False)
    parser.add_argument("--gpu", type=int, default=0)
    parser.add_argument("--size", type=int, default=3, help="chain length = action dimensions")
    parser.add_argument("--num-envs", type=int, default=4)
    parser.add_argument("--minibatch-size", type=int, default=32)
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--steps", type=int, default=2 * 10 ** 4)
    parser.add_argument("--replay-start-size", type=int, default=500)
    parser.add_argument("--time-updates", type=int, default=0)
    return parser.parse_args(argv)


def make_env(args):
    return pfrl.envs.SerialVectorEnv([pfrl.envs.ABC(size=args.size, discrete=False)
                                      for _ in range(args.num_envs)])


def make_agent(args, env):
    obs = env.observation_space.shape[0]
    q = pfrl.q_functions.FCQuadraticStateQFunction(obs, args.size, 64, 2, env.action_space)
    opt = torch.optim.Adam(q.parameters(), lr=1e-3)
    cls = agents.DoubleDQN if args.double else agents.DQN
    return cls(q, opt, replay_buffers.ReplayBuffer(10 ** 5), 0.9, explorers.AdditiveOU(sigma=0.3),
               gpu=args.gpu, replay_start_size=args.replay_start_size,
               minibatch_size=args.minibatch_size, update_interval=1, target_update_interval=100)


def time_updates(agent, env, args, repeats=5, warmup=30):
    obs = env.reset()
    agent.replay_updater.replay_start_size = 10 ** 9        # (fill only)
    while len(agent.replay_buffer) < 4 * args.minibatch_size:
        actions = agent.batch_act(obs)
        obs, rewards, dones, _ = env.step(actions)
        agent.batch_observe(obs, rewards, dones, [False] * args.num_envs)
        obs = env.reset(np.logical_not(dones))
    sync = torch.cuda.synchronize if args.gpu >= 0 else (lambda: None)
    batch = agent.replay_buffer.sample(args.minibatch_size)
    for _ in range(warmup):
        agent.update(batch)
    us = []
    for _ in range(repeats):
        sync()
        t0 = time.perf_counter()
        for _ in range(args.time_updates):
            agent.update(batch)
        sync()
        us.append(1e6 * (time.perf_counter() - t0) / args.time_updates)
    print(json.dumps(dict(agent=type(agent).__name__, fused=bool(agent._fused_td_loss_applicable()
                                     and agent._naf_split() is not None),
                          graphs=bool(agent.use_graphs), minibatch=args.minibatch_size,
                          updates=args.time_updates, timed_updates=repeats * args.time_updates,
                          all_updates=warmup + repeats * args.time_updates,
                          us_per_update=[round(u, 2) for u in us],
                          median_us=round(float(np.median(us)), 2))))


def main():
    args = parse_args()
    if args.composite:
        os.environ["PFRL_NAF_FUSED"] = "0"
    utils.set_random_seed(args.seed)
    env = make_env(args)
    agent = make_agent(args, env)
    if args.time_updates:
        time_updates(agent, env, args)
        return
    import tempfile

    pfrl.experiments.train_agent_batch(agent, env, args.steps, tempfile.mkdtemp(prefix="dqn_naf_"),
                                       log_interval=10 ** 9)
    print("env steps %d  %s" % (args.steps, agent.get_statistics()))


if __name__ == "__main__":
    main()
