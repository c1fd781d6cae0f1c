#!/usr/bin/env python
"""Advantage learning (AL, PAL, DoublePAL) and dynamic policy programming (DPP, DPPL,
DPPGreedy) on synthetic Atari-shaped envs -- the DQN configuration of
examples/train_dqn_batch_synthetic.py (Nature network, RMSprop, uniform replay) with the agent
class chosen by ``--agent``, run through the batched driver with `pfrl` replaced by `pfrl_amd`.
On the GPU everything behind the network passes is one launch (pfrl_dqn_operator_td_loss);
``--no-fused`` keeps the stock-PyTorch composite loss.

``--time-updates N`` does not train to the end: it fills the replay buffer, gathers one
minibatch and times N captured updates on it with device events (after a warm-up), five
repeats, and prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pfrl_amd import agents, experiments, explorers  # noqa: E402
from pfrl_amd import nn as pnn  # noqa: E402
from pfrl_amd import replay_buffers, utils  # noqa: E402
from pfrl_amd.initializers import init_chainer_default  # noqa: E402
from pfrl_amd.q_functions import DiscreteActionValueHead  # noqa: E402

AGENTS = ("AL", "PAL", "DoublePAL", "DPP", "DPPL", "DPPGreedy")


def parse_args(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("--agent", type=str, default="AL", choices=AGENTS)
    parser.add_argument("--no-fused", action="store_true", default=False)
    parser.add_argument("--alpha", type=float, default=0.9)
    parser.add_argument("--eta", type=float, default=1.0)
    parser.add_argument("--gpu", type=int, default=0)
    parser.add_argument("--num-envs", type=int, default=256)
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--outdir", type=str, default="results")
    parser.add_argument("--steps", type=int, default=10 ** 6)
    parser.add_argument("--replay-start-size", type=int, default=5 * 10 ** 4)
    parser.add_argument("--capacity", type=int, default=10 ** 6)
    parser.add_argument("--final-exploration-frames", type=int, default=10 ** 6)
    parser.add_argument("--final-epsilon", type=float, default=0.01)
    parser.add_argument("--target-update-interval", type=int, default=3 * 10 ** 4)
    parser.add_argument("--update-interval", type=int, default=4)
    parser.add_argument("--batch-size", type=int, default=32)
    parser.add_argument("--eval-interval", type=int, default=10 ** 5)
    parser.add_argument("--eval-n-runs", type=int, default=10)
    parser.add_argument("--lr", type=float, default=2.5e-4)
    parser.add_argument("--time-updates", type=int, default=0)
    return parser.parse_args(argv)


def make_agent(args, n_actions=6, **agent_kw):
    q_func = nn.Sequential(pnn.LargeAtariCNN(), init_chainer_default(nn.Linear(512, n_actions)),
                           DiscreteActionValueHead())
    opt = torch.optim.RMSprop(q_func.parameters(), lr=args.lr, alpha=0.95, momentum=0.0, eps=1e-2,
                              centered=True)
    rbuf = replay_buffers.ReplayBuffer(args.capacity)
    explorer = explorers.LinearDecayEpsilonGreedy(
        1.0, args.final_epsilon, args.final_exploration_frames,
        lambda: np.random.randint(n_actions))

    def phi(x):
        return np.asarray(x, dtype=np.float32) / 255

    if args.agent in ("AL", "PAL", "DoublePAL"):
        agent_kw["alpha"] = args.alpha
    elif args.agent in ("DPP", "DPPL"):
        agent_kw["eta"] = args.eta
    return getattr(agents, args.agent)(
        q_func, opt, rbuf, gpu=args.gpu, gamma=0.99, explorer=explorer,
        replay_start_size=args.replay_start_size,
        target_update_interval=args.target_update_interval, clip_delta=True,
        update_interval=args.update_interval, batch_accumulator="sum", phi=phi,
        minibatch_size=args.batch_size, fused_td_loss=not args.no_fused, **agent_kw)


def make_batch_env(args, test):
    from pfrl_amd.device_store import DeviceFrameStore
    from pfrl_amd.envs import SyntheticAtariVectorEnv

    device = torch.device("cuda", args.gpu)
    slots = (args.capacity if not test else 0) + args.num_envs * 32 + 8192
    store = DeviceFrameStore(slots, (84, 84), torch.uint8, device, stack=4)
    return SyntheticAtariVectorEnv(args.num_envs, store=store,
                                   seed=args.seed + (10 ** 6 if test else 0))


def gather_minibatch(agent, args):
    """One minibatch of the filled replay buffer, as ``update`` hands it to the loss."""
    from pfrl_amd.replay_buffer import batch_experiences

    return batch_experiences(agent.replay_buffer.sample(args.batch_size), device=agent.device,
                             phi=agent.phi, gamma=agent.gamma, batch_states=agent.batch_states)


def time_updates(agent, args, repeats=5, warmup=50):
    exp_batch = gather_minibatch(agent, args)
    for _ in range(warmup):
        agent._update_from_batch(exp_batch)
    torch.cuda.synchronize()
    us = []
    for _ in range(repeats):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(args.time_updates):
            agent._update_from_batch(exp_batch)
        stop.record()
        stop.synchronize()
        us.append(1e3 * start.elapsed_time(stop) / args.time_updates)
    print(json.dumps(dict(agent=args.agent, fused=agent._fused_operator_loss_applicable(),
                          captured=bool(agent.use_graphs and agent._graphed is not None
                                        and agent._graphed.graphs),
                          batch_size=args.batch_size, updates=args.time_updates,
                          us_per_update=[round(u, 2) for u in us],
                          median_us=round(float(np.median(us)), 2))))


def main():
    args = parse_args()
    import logging

    logging.basicConfig(level=logging.INFO)
    utils.set_random_seed(args.seed)
    os.makedirs(args.outdir, exist_ok=True)
    agent = make_agent(args)
    if args.time_updates:
        experiments.train_agent_batch(agent, make_batch_env(args, False), steps=args.steps,
                                      outdir=args.outdir, log_interval=10 ** 9)
        time_updates(agent, args)
        return
    experiments.train_agent_batch_with_evaluation(
        agent=agent, env=make_batch_env(args, test=False), eval_env=make_batch_env(args, test=True),
        steps=args.steps, eval_n_steps=None, eval_n_episodes=args.eval_n_runs,
        eval_interval=args.eval_interval, outdir=args.outdir, save_best_so_far_agent=False,
        log_interval=10 ** 4)
    print(agent.get_statistics())


if __name__ == "__main__":
    main()
