#!/usr/bin/env python
"""IQN on synthetic Atari-shaped envs -- the configuration of the reference's
examples/atari/reproduction/iqn/train_iqn.py (ImplicitQuantileQFunction with the DQN trunk
as psi, a 64-cosine embedding as phi and Linear(3136, 512) / Linear(512, n_actions) as f;
N = N' = 64, K = 32; Adam(5e-5, eps 1e-2 / 32); uniform replay; mean accumulator) run through
the batched driver with `pfrl` replaced by `pfrl_amd`.  On the GPU the loss behind the three
network passes is one launch (pfrl_iqn_loss)."""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pfrl_amd import agents, experiments, explorers, replay_buffers, utils  # noqa: E402
from pfrl_amd.agents import iqn  # noqa: E402


def make_q_func(n_actions):
    return iqn.ImplicitQuantileQFunction(
        psi=nn.Sequential(nn.Conv2d(4, 32, 8, stride=4), nn.ReLU(),
                          nn.Conv2d(32, 64, 4, stride=2), nn.ReLU(),
                          nn.Conv2d(64, 64, 3, stride=1), nn.ReLU(), nn.Flatten()),
        phi=nn.Sequential(iqn.CosineBasisLinear(64, 3136), nn.ReLU()),
        f=nn.Sequential(nn.Linear(3136, 512), nn.ReLU(), nn.Linear(512, n_actions)))


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--gpu", type=int, default=0)
    parser.add_argument("--num-envs", type=int, default=256)
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--outdir", type=str, default="results")
    parser.add_argument("--steps", type=int, default=5 * 10 ** 7)
    parser.add_argument("--replay-start-size", type=int, default=5 * 10 ** 4)
    parser.add_argument("--capacity", type=int, default=10 ** 6)
    parser.add_argument("--final-exploration-frames", type=int, default=10 ** 6)
    parser.add_argument("--final-epsilon", type=float, default=0.01)
    parser.add_argument("--target-update-interval", type=int, default=10 ** 4)
    parser.add_argument("--update-interval", type=int, default=4)
    parser.add_argument("--batch-size", type=int, default=32)
    parser.add_argument("--eval-interval", type=int, default=250000)
    parser.add_argument("--eval-n-runs", type=int, default=10)
    parser.add_argument("--quantile-thresholds-N", type=int, default=64)
    parser.add_argument("--quantile-thresholds-N-prime", type=int, default=64)
    parser.add_argument("--quantile-thresholds-K", type=int, default=32)
    args = parser.parse_args()

    import logging

    logging.basicConfig(level=logging.INFO)
    utils.set_random_seed(args.seed)
    os.makedirs(args.outdir, exist_ok=True)
    device = torch.device("cuda", args.gpu)
    N = args.num_envs

    from pfrl_amd.device_store import DeviceFrameStore
    from pfrl_amd.envs import SyntheticAtariVectorEnv

    def make_batch_env(test):
        slots = (args.capacity if not test else 0) + N * 32 + 8192
        store = DeviceFrameStore(slots, (84, 84), torch.uint8, device, stack=4)
        return SyntheticAtariVectorEnv(N, store=store, seed=args.seed + (10 ** 6 if test else 0))

    n_actions = 6
    q_func = make_q_func(n_actions)
    opt = torch.optim.Adam(q_func.parameters(), lr=5e-5, eps=1e-2 / args.batch_size)
    rbuf = replay_buffers.ReplayBuffer(args.capacity)
    explorer = explorers.LinearDecayEpsilonGreedy(
        1.0, args.final_epsilon, args.final_exploration_frames,
        lambda: np.random.randint(n_actions))

    def phi(x):
        return np.asarray(x, dtype=np.float32) / 255

    agent = agents.IQN(
        q_func, opt, rbuf, gpu=args.gpu, gamma=0.99, explorer=explorer,
        replay_start_size=args.replay_start_size,
        target_update_interval=args.target_update_interval,
        update_interval=args.update_interval, batch_accumulator="mean", phi=phi,
        minibatch_size=args.batch_size,
        quantile_thresholds_N=args.quantile_thresholds_N,
        quantile_thresholds_N_prime=args.quantile_thresholds_N_prime,
        quantile_thresholds_K=args.quantile_thresholds_K)
    experiments.train_agent_batch_with_evaluation(
        agent=agent, env=make_batch_env(False), eval_env=make_batch_env(True), outdir=args.outdir,
        steps=args.steps, eval_n_steps=None, eval_n_episodes=args.eval_n_runs,
        eval_interval=args.eval_interval, log_interval=10 ** 5, save_best_so_far_agent=False)
    print(agent.get_statistics())


if __name__ == "__main__":
    main()
