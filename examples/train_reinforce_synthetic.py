#!/usr/bin/env python
"""REINFORCE on CartPole -- the agent of the reference's examples/gym/train_reinforce_gym.py (a
two-hidden-layer policy ending in a SoftmaxCategoricalHead, Adam, entropy bonus ``beta``, ``batchsize``
episodes per update) with `pfrl` replaced by `pfrl_amd` and the gym env by the package's own CartPole
(there is no gym in this image), driven by ``train_agent`` as the reference's script is.  On a GPU the
update is one batched forward over the stored steps, one fused loss launch and one backward
(``--recompute-forward off`` keeps the reference's per-step graphs on the same device).  Prints the
statistics, env-steps/s and, with --count-launches, the library launches of the run."""
import argparse
import collections
import os
import sys
import tempfile
import time

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pfrl_amd as pfrl  # noqa: E402
from pfrl_amd import experiments, utils  # noqa: E402
from pfrl_amd.agents import REINFORCE  # noqa: E402
from pfrl_amd.envs.cartpole import CartPoleEnv  # noqa: E402


def make_agent(obs_size, n_actions, gpu, batchsize=10, beta=1e-4, recompute_forward=True, hidden=200):
    model = nn.Sequential(
        nn.Linear(obs_size, hidden), nn.LeakyReLU(0.2), nn.Linear(hidden, hidden), nn.LeakyReLU(0.2),
        nn.Linear(hidden, n_actions), pfrl.policies.SoftmaxCategoricalHead())
    return REINFORCE(model, torch.optim.Adam(model.parameters(), lr=1e-3), gpu=gpu, beta=beta,
                     batchsize=batchsize, max_grad_norm=1.0, recompute_forward=recompute_forward)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--gpu", type=int, default=0)
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--steps", type=int, default=20000)
    parser.add_argument("--batchsize", type=int, default=10)
    parser.add_argument("--beta", type=float, default=1e-4)
    parser.add_argument("--recompute-forward", choices=["on", "off"], default="on")
    parser.add_argument("--count-launches", action="store_true",
                        help="also print how often each library entry point was called")
    args = parser.parse_args()

    utils.set_random_seed(args.seed)
    env = CartPoleEnv(seed=args.seed)
    agent = make_agent(env.observation_space.low.size, env.action_space.n, args.gpu, args.batchsize,
                       args.beta, args.recompute_forward == "on")
    outdir = tempfile.mkdtemp(prefix="reinforce_")

    def run():
        start = time.perf_counter()
        experiments.train_agent(agent, env, args.steps, outdir)
        if args.gpu >= 0:
            torch.cuda.synchronize()
        return time.perf_counter() - start

    if args.count_launches and args.gpu >= 0:
        from pfrl_amd import _native

        with _native.timed_calls() as rec:
            seconds = run()
        print("library calls:", dict(collections.Counter(name for name, _, _ in rec.calls)))
    else:
        seconds = run()
    print("steps %d  %s  env-steps/s %.1f  device route %s" % (
        args.steps, dict(agent.get_statistics()), args.steps / seconds, agent.device_route))


if __name__ == "__main__":
    main()
