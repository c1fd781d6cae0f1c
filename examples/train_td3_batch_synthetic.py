#!/usr/bin/env python
"""TD3 / DDPG on the host-side synthetic vector-observation env, `pfrl` replaced by `pfrl_amd`: the
agents of the reference's examples/mujoco/reproduction/{td3,ddpg} at Humanoid's shape (376 floats in,
17 action dimensions) with the 256-256 MLPs of benchkit/workloads.py::build_sac as policy and critics,
Adam(3e-4), uniform replay, minibatch ``--minibatch-size``.

On the GPU what lies between the network outputs and ``backward()`` is one launch per piece (target-policy
smoothing, critic target + losses + gradients, actor loss + gradient: csrc/td3.hip) and TD3's twin
critics run as one chain of launches; ``--no-fused-loss`` keeps the torch expressions.

``--time-updates K`` does not train: it captures the update on one synthetic minibatch (TD3: both step
shapes, replayed alternately as ``policy_update_delay=2`` makes them alternate), times K replays between
device synchronisations (after a warm-up), five repeats, counts the device kernels / copies of one eager
update with the profiler (TD3: the shape with the policy update) and prints one JSON line."""
import argparse
import inspect
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
    parser.add_argument("--agent", type=str, default="td3", choices=("td3", "ddpg"))
    parser.add_argument("--no-fused-loss", action="store_true", default=False)
    parser.add_argument("--gpu", type=int, default=0)
    parser.add_argument("--num-envs", type=int, default=16)
    parser.add_argument("--minibatch-size", type=int, default=100)
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--steps", type=int, default=2 * 10 ** 4)
    parser.add_argument("--replay-start-size", type=int, default=1000)
    parser.add_argument("--time-updates", type=int, default=0)
    return parser.parse_args(argv)


def make_agent(args):
    from pfrl_amd.optimizers import FusedAdam

    policy = nn.Sequential(nn.Linear(OBS, 256), nn.ReLU(), nn.Linear(256, 256), nn.ReLU(),
                           nn.Linear(256, ACT),
                           pfrl.nn.BoundByTanh(low=-np.ones(ACT, dtype=np.float32),
                                               high=np.ones(ACT, dtype=np.float32)),
                           pfrl.policies.DeterministicHead())

    def make_q():
        q = nn.Sequential(pfrl.nn.ConcatObsAndAction(), nn.Linear(OBS + ACT, 256), nn.ReLU(),
                          nn.Linear(256, 256), nn.ReLU(), nn.Linear(256, 1))
        for i in (1, 3, 5):
            nn.init.xavier_uniform_(q[i].weight)
        return q

    Adam = (lambda ps: FusedAdam(ps, lr=3e-4)) if args.gpu >= 0 else (lambda ps: torch.optim.Adam(ps, lr=3e-4))
    common = dict(gamma=0.99, explorer=explorers.AdditiveGaussian(scale=0.1, low=-1.0, high=1.0),
                  gpu=args.gpu, replay_start_size=args.replay_start_size,
                  minibatch_size=args.minibatch_size, update_interval=1,
                  burnin_action_func=lambda: np.random.uniform(-1, 1, size=ACT).astype(np.float32))
    cls = agents.TD3 if args.agent == "td3" else agents.DDPG
    if "fused_loss" in inspect.signature(cls.__init__).parameters:
        common["fused_loss"] = not args.no_fused_loss
    rbuf = replay_buffers.ReplayBuffer(10 ** 5)
    if args.agent == "td3":
        q1, q2 = make_q(), make_q()
        return agents.TD3(policy, q1, q2, Adam(policy.parameters()), Adam(q1.parameters()),
                          Adam(q2.parameters()), rbuf, soft_update_tau=5e-3, **common)
    q = make_q()
    return agents.DDPG(policy, q, Adam(policy.parameters()), Adam(q.parameters()), rbuf,
                       target_update_interval=1, target_update_method="soft", soft_update_tau=5e-3,
                       **common)


def synthetic_batch(args, device):
    g = torch.Generator().manual_seed(args.seed)
    B = args.minibatch_size
    b = {"state": torch.randn(B, OBS, generator=g), "next_state": torch.randn(B, OBS, generator=g),
         "action": torch.rand(B, ACT, generator=g) * 2 - 1, "reward": torch.randn(B, generator=g),
         "is_state_terminal": (torch.rand(B, generator=g) < 0.05).float(),
         "discount": torch.full((B,), 0.99)}
    return {k: v.to(device) for k, v in b.items()}


def count_launches(agent, batch, variant):
    """Device kernels and copies of ONE eager update, from the profiler's device events."""
    from torch.profiler import ProfilerActivity, profile

    agent._update_impl(batch, variant)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        agent._update_impl(batch, variant)
        torch.cuda.synchronize()
    kernels = copies = 0
    for ev in prof.events():
        if ev.device_type == torch.autograd.DeviceType.CUDA:
            if "memcpy" in ev.name.lower() or "memset" in ev.name.lower():
                copies += 1
            else:
                kernels += 1
    return kernels, copies


def time_updates(agent, args, repeats=5, warmup=30):
    from pfrl_amd.agents.graphed_update import CapturedStep

    batch = synthetic_batch(args, agent.device)
    variants = [False, True] if args.agent == "td3" else [None]
    step = CapturedStep(agent._update_core, agent._graph_modules(), agent._graph_optimizers(),
                        agent.device)
    for i in range(warmup):
        step.run(batch, variants[i % len(variants)])
    us = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(args.time_updates):
            step.run(batch, variants[i % len(variants)])
        torch.cuda.synchronize()
        us.append(1e6 * (time.perf_counter() - t0) / args.time_updates)
    kernels, copies = count_launches(agent, batch, variants[-1])
    print(json.dumps(dict(agent=args.agent, fused=bool(getattr(agent, "fused_loss", False)),
                          minibatch=args.minibatch_size, updates=args.time_updates,
                          us_per_update=[round(u, 2) for u in us], median_us=round(float(np.median(us)), 2),
                          device_kernels=kernels, device_copies=copies)))


def main():
    args = parse_args()
    utils.set_random_seed(args.seed)
    agent = make_agent(args)
    if args.time_updates:
        time_updates(agent, args)
        return
    import tempfile

    from pfrl_amd.envs.synthetic import HostSyntheticVectorObsEnv

    env = HostSyntheticVectorObsEnv(args.num_envs, obs_dim=OBS, act_dim=ACT, seed=args.seed)
    pfrl.experiments.train_agent_batch(agent, env, args.steps, tempfile.mkdtemp(prefix=args.agent + "_"),
                                       log_interval=10 ** 9)
    print("env steps %d  %s" % (args.steps, agent.get_statistics()))


if __name__ == "__main__":
    main()
