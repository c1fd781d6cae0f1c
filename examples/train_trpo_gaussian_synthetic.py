#!/usr/bin/env python
"""TRPO with a Gaussian policy on synthetic MuJoCo-shaped envs -- the models, optimizer and agent of
the reference's examples/mujoco/reproduction/trpo/train_trpo.py (two 64-64 tanh MLPs, a
state-independent diagonal covariance parameterised as log std, observation normalisation, Adam on
the value function, update_interval 5000, max_kl 0.01, 10 CG iterations, 5 value epochs) with `pfrl`
replaced by `pfrl_amd` and the gym env factory by the host-side synthetic VectorEnv (there is no
MuJoCo in this image).  Prints env-steps/s and, with --count-launches, the library launches of one
policy update.  --switches off keeps the whole update as eager torch on the device."""
import argparse
import collections
import os
import sys
import time

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pfrl_amd as pfrl  # noqa: E402
from pfrl_amd import utils  # noqa: E402
from pfrl_amd.agents import TRPO  # noqa: E402
from pfrl_amd.envs.synthetic import HostSyntheticVectorObsEnv  # noqa: E402


def make_models(obs_size, action_size):
    policy = nn.Sequential(
        nn.Linear(obs_size, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(),
        nn.Linear(64, action_size),
        pfrl.policies.GaussianHeadWithStateIndependentCovariance(
            action_size=action_size, var_type="diagonal",
            var_func=lambda x: torch.exp(2 * x),    # parameterise log std
            var_param_init=0))                      # log std = 0 => std = 1
    vf = nn.Sequential(nn.Linear(obs_size, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(),
                       nn.Linear(64, 1))
    for layer, gain in ((policy[0], 1), (policy[2], 1), (policy[4], 1e-2), (vf[0], 1), (vf[2], 1),
                        (vf[4], 1)):
        nn.init.orthogonal_(layer.weight, gain=gain)
        nn.init.zeros_(layer.bias)
    return policy, vf


def make_agent(obs_size, action_size, gpu, update_interval=5000, switches=True):
    policy, vf = make_models(obs_size, action_size)
    return TRPO(policy, vf, torch.optim.Adam(vf.parameters(), lr=1e-3),
                obs_normalizer=pfrl.nn.EmpiricalNormalization(obs_size, clip_threshold=5), gpu=gpu,
                update_interval=update_interval, max_kl=0.01, conjugate_gradient_max_iter=10,
                conjugate_gradient_damping=1e-1, gamma=0.995, lambd=0.97, vf_epochs=5, entropy_coef=0,
                **({} if switches is None else dict(
                    fused_gaussian_eval=switches, device_cg=switches, fused_param_step=switches,
                    capture_vf_step=switches)))


def run(agent, env, steps, on_update=None):
    """The batch training loop without evaluation or logging; ``on_update(env steps so far)`` is
    called after each completed update."""
    obs = env.reset()
    t, n_updates = 0, agent.n_updates
    while t < steps:
        actions = agent.batch_act(obs)
        obs, rewards, dones, infos = env.step(actions)
        t += env.num_envs
        agent.batch_observe(obs, rewards, dones, [False] * env.num_envs)
        if agent.n_updates != n_updates:
            n_updates = agent.n_updates
            if on_update is not None:
                on_update(t)
        obs = env.reset(~dones)
    return n_updates


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--gpu", type=int, default=0)
    parser.add_argument("--num-envs", type=int, default=1)
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--steps", type=int, default=8 * 5000)
    parser.add_argument("--warmup-updates", type=int, default=2,
                        help="updates before the timed region (captures, library warm-up)")
    parser.add_argument("--update-interval", type=int, default=5000)
    parser.add_argument("--switches", choices=["on", "off"], default="on")
    parser.add_argument("--count-launches", action="store_true",
                        help="also print the library launches of the last policy update")
    args = parser.parse_args()

    utils.set_random_seed(args.seed)
    obs_size, action_size = 17, 6
    env = HostSyntheticVectorObsEnv(args.num_envs, obs_dim=obs_size, act_dim=action_size,
                                    seed=args.seed)
    agent = make_agent(obs_size, action_size, args.gpu, args.update_interval, args.switches == "on")
    marks = []

    def on_update(t):
        if args.gpu >= 0:
            torch.cuda.synchronize()
        marks.append((t, time.perf_counter()))

    run(agent, env, args.steps, on_update)
    stats = dict(agent.get_statistics())
    print("updates %d  average_kl %.6g  average_policy_step_size %.4g  average_entropy %.6g" % (
        len(marks), stats["average_kl"], stats["average_policy_step_size"], stats["average_entropy"]))
    w = args.warmup_updates
    if len(marks) > w + 1:
        (t0, c0), (t1, c1) = marks[w], marks[-1]
        print("updates timed %d  env-steps/s %.1f  seconds/update-interval %.4f" % (
            len(marks) - 1 - w, (t1 - t0) / (c1 - c0), (c1 - c0) / (len(marks) - 1 - w)))
    else:
        print("too few updates to time (%d completed, %d warm-up)" % (len(marks), w))
    if args.count_launches and args.gpu >= 0:
        # one more policy update on the last dataset's shapes, with every library entry point counted
        from pfrl_amd import _native

        agent.update_interval = args.update_interval
        with _native.timed_calls() as rec:
            run(agent, env, args.update_interval)
        print("library calls of one rollout + update:",
              dict(collections.Counter(name for name, _, _ in rec.calls)))


if __name__ == "__main__":
    main()
