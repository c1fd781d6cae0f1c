#!/usr/bin/env python
"""Dynamic policy programming (DPP, DPPL) -- or any agent of the DQN family -- with Boltzmann
exploration on synthetic Atari-shaped envs: the configuration of
examples/train_al_family_batch_synthetic.py with ``explorers.Boltzmann(T)`` instead of
epsilon-greedy, run through the batched driver with `pfrl` replaced by `pfrl_amd`.  On the GPU the
step never visits the host: the N uniforms of the reference's N ``np.random.choice`` calls are
drawn up front from the same stream positions, softmax, cdf and search run behind the Q head in
one launch (pfrl_dqn_act_head_boltzmann), and the actions stay in HBM for the replay append.
``--per-env`` keeps the reference's loop (one softmax, device-to-host read and ``choice`` per env).

``--time-steps K`` does not train to the end: it fills the replay buffer to ``--replay-start-size``,
runs ``--warmup`` batched steps and then times K steps (acting, env, appends and updates) with a
host clock around a device synchronise, five repeats, and prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pfrl_amd import agents, experiments, explorers  # noqa: E402
from pfrl_amd import nn as pnn  # noqa: E402
from pfrl_amd import replay_buffers, utils  # noqa: E402
from pfrl_amd.initializers import init_chainer_default  # noqa: E402
from pfrl_amd.q_functions import DiscreteActionValueHead  # noqa: E402

AGENTS = ("DPP", "DPPL", "DPPGreedy", "DQN", "DoubleDQN", "AL", "PAL", "DoublePAL")


def parse_args(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("--agent", type=str, default="DPP", choices=AGENTS)
    parser.add_argument("--temperature", type=float, default=1.0)
    parser.add_argument("--per-env", action="store_true", default=False)
    parser.add_argument("--eta", type=float, default=1.0)
    parser.add_argument("--alpha", type=float, default=0.9)
    parser.add_argument("--gpu", type=int, default=0)
    parser.add_argument("--num-envs", type=int, default=256)
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--outdir", type=str, default="results")
    parser.add_argument("--steps", type=int, default=10 ** 6)
    parser.add_argument("--replay-start-size", type=int, default=5 * 10 ** 4)
    parser.add_argument("--capacity", type=int, default=10 ** 6)
    parser.add_argument("--target-update-interval", type=int, default=3 * 10 ** 4)
    parser.add_argument("--update-interval", type=int, default=4)
    parser.add_argument("--batch-size", type=int, default=32)
    parser.add_argument("--eval-interval", type=int, default=10 ** 5)
    parser.add_argument("--eval-n-runs", type=int, default=10)
    parser.add_argument("--lr", type=float, default=2.5e-4)
    parser.add_argument("--time-steps", type=int, default=0)
    parser.add_argument("--warmup", type=int, default=20)
    return parser.parse_args(argv)


def make_agent(args, n_actions=6, **agent_kw):
    q_func = nn.Sequential(pnn.LargeAtariCNN(), init_chainer_default(nn.Linear(512, n_actions)),
                           DiscreteActionValueHead())
    opt = torch.optim.RMSprop(q_func.parameters(), lr=args.lr, alpha=0.95, momentum=0.0, eps=1e-2,
                              centered=True)
    rbuf = replay_buffers.ReplayBuffer(args.capacity)

    def phi(x):
        return np.asarray(x, dtype=np.float32) / 255

    if args.agent in ("AL", "PAL", "DoublePAL"):
        agent_kw["alpha"] = args.alpha
    elif args.agent in ("DPP", "DPPL"):
        agent_kw["eta"] = args.eta
    agent = getattr(agents, args.agent)(
        q_func, opt, rbuf, gpu=args.gpu, gamma=0.99, explorer=explorers.Boltzmann(args.temperature),
        replay_start_size=args.replay_start_size,
        target_update_interval=args.target_update_interval, clip_delta=True,
        update_interval=args.update_interval, batch_accumulator="sum", phi=phi,
        minibatch_size=args.batch_size, **agent_kw)
    if args.per_env:
        agent.device_step = False
    return agent


def make_batch_env(args, test):
    from pfrl_amd.device_store import DeviceFrameStore
    from pfrl_amd.envs import SyntheticAtariVectorEnv

    device = torch.device("cuda", args.gpu)
    slots = (args.capacity if not test else 0) + args.num_envs * 32 + 8192
    store = DeviceFrameStore(slots, (84, 84), torch.uint8, device, stack=4)
    return SyntheticAtariVectorEnv(args.num_envs, store=store,
                                   seed=args.seed + (10 ** 6 if test else 0))


def time_steps(agent, args, repeats=5):
    env = make_batch_env(args, False)
    N = args.num_envs
    obss = env.reset()
    resets = np.zeros(N, dtype=bool)

    def step(obss):
        actions = agent.batch_act(obss)
        obss, rs, dones, _ = env.step(actions)
        agent.batch_observe(obss, rs, dones, resets)
        return env.reset(np.logical_not(dones))

    while len(agent.replay_buffer) < args.replay_start_size:
        obss = step(obss)
    for _ in range(args.warmup):
        obss = step(obss)
    rates = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.time_steps):
            obss = step(obss)
        torch.cuda.synchronize()
        rates.append(N * args.time_steps / (time.perf_counter() - t0))
    agent.get_statistics()
    print(json.dumps(dict(agent=args.agent, explorer=repr(agent.explorer), num_envs=N,
                          device_step=bool(agent.device_step and agent._last_actions_dev is not None),
                          act_graph=bool(getattr(agent.__dict__.get("_act_graph"), "entries", None)),
                          steps=args.time_steps, updates=agent.optim_t,
                          env_steps_per_s=[round(r, 1) for r in rates],
                          median_env_steps_per_s=round(float(np.median(rates)), 1))))


def main():
    args = parse_args()
    import logging

    logging.basicConfig(level=logging.INFO)
    utils.set_random_seed(args.seed)
    agent = make_agent(args)
    if args.time_steps:
        time_steps(agent, args)
        return
    os.makedirs(args.outdir, exist_ok=True)
    experiments.train_agent_batch_with_evaluation(
        agent=agent, env=make_batch_env(args, test=False), eval_env=make_batch_env(args, test=True),
        steps=args.steps, eval_n_steps=None, eval_n_episodes=args.eval_n_runs,
        eval_interval=args.eval_interval, outdir=args.outdir, save_best_so_far_agent=False,
        log_interval=10 ** 4)
    print(agent.get_statistics())


if __name__ == "__main__":
    main()
