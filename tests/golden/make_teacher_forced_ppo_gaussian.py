#!/usr/bin/env python
"""Teacher-forced fixture for PPO with a Gaussian policy, recorded by running the REFERENCE
(pfnet/pfrl) itself.

    python tests/golden/make_teacher_forced_ppo_gaussian.py   (build container only: needs the reference checkout)

The reference's PPO (pfrl/agents/ppo.py) with the model, normaliser, optimizer and loss settings of
examples/mujoco/reproduction/ppo/train_ppo.py:146-206 (two 64-64 tanh MLPs under ``Branched``,
``GaussianHeadWithStateIndependentCovariance(diagonal, exp(2x))``, ``EmpiricalNormalization(clip 5)``,
Adam lr 3e-4 eps 1e-5, no value clipping, entropy_coef 0) runs three short rollouts on the synthetic
vector-observation env (obs 17, act 6).  For the first minibatch update, one in the middle and the
last one it records everything ONE update (ppo.py:480-532) depends on -- parameters and Adam state
before the step, the normaliser's statistics, the minibatch (raw states, actions, standardised
advantages, value targets, old values, old log-probabilities) -- and what it produced: the three
loss terms and the parameters after the Adam step.

Output: tests/golden/teacher_forced_ppo_gaussian.npz
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_golden as mg  # noqa: E402,F401  (puts the reference and the gym shim on sys.path)

OBS, ACT, N = 17, 6, 4
UPDATE_INTERVAL, MINIBATCH, EPOCHS, ROLLOUTS = 256, 64, 2, 3
UPDATES = (1, 12, 24)


def flat(tensors):
    return np.concatenate([t.detach().numpy().ravel() for t in tensors])


def main():
    import tempfile

    import pfrl
    from pfrl import agents, experiments
    from torch import nn

    sys.path.insert(0, os.path.join(HERE, "..", ".."))
    from pfrl_amd.envs.synthetic import HostSyntheticVectorObsEnv

    pfrl.utils.set_random_seed(0)
    torch.manual_seed(97531)
    env = HostSyntheticVectorObsEnv(N, obs_dim=OBS, act_dim=ACT, seed=9, p_done=0.02)
    policy = nn.Sequential(
        nn.Linear(OBS, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, ACT),
        pfrl.policies.GaussianHeadWithStateIndependentCovariance(
            action_size=ACT, var_type="diagonal", var_func=lambda x: torch.exp(2 * x),
            var_param_init=0))
    vf = nn.Sequential(nn.Linear(OBS, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 1))
    for layer, gain in ((policy[0], 1), (policy[2], 1), (policy[4], 1e-2), (vf[0], 1), (vf[2], 1),
                        (vf[4], 1)):
        nn.init.orthogonal_(layer.weight, gain=gain)
        nn.init.zeros_(layer.bias)
    model = pfrl.nn.Branched(policy, vf)
    normalizer = pfrl.nn.EmpiricalNormalization(OBS, clip_threshold=5)
    opt = torch.optim.Adam(model.parameters(), lr=3e-4, eps=1e-5)
    ag = agents.PPO(model, opt, obs_normalizer=normalizer, gpu=-1, update_interval=UPDATE_INTERVAL,
                    minibatch_size=MINIBATCH, epochs=EPOCHS, clip_eps_vf=None, entropy_coef=0,
                    standardize_advantages=True, gamma=0.995, lambd=0.97)
    out = {}
    count = [0]
    last = {}
    orig_norm = normalizer.forward

    def spy_norm(x, update=True):
        last["states"] = x
        return orig_norm(x, update=update)

    normalizer.forward = spy_norm
    orig_forward = model.forward

    def spy_forward(x):
        distrib, v = orig_forward(x)
        orig_lp = distrib.log_prob

        def log_prob(a):
            last["actions"] = a
            return orig_lp(a)

        distrib.log_prob = log_prob
        return distrib, v

    model.forward = spy_forward
    orig_loss = ag._lossfun
    params = list(model.parameters())

    def spy_loss(entropy, vs_pred, log_probs, vs_pred_old, log_probs_old, advs, vs_teacher):
        count[0] += 1
        k = count[0]
        loss = orig_loss(entropy, vs_pred, log_probs, vs_pred_old=vs_pred_old,
                         log_probs_old=log_probs_old, advs=advs, vs_teacher=vs_teacher)
        if k in UPDATES:
            out["u%d_params" % k] = flat(params)
            st = [opt.state.get(p, {}) for p in params]
            if all("exp_avg" in s for s in st):
                out["u%d_exp_avg" % k] = flat([s["exp_avg"] for s in st])
                out["u%d_exp_avg_sq" % k] = flat([s["exp_avg_sq"] for s in st])
                out["u%d_step" % k] = np.asarray(float(st[0]["step"]))
            else:
                out["u%d_step" % k] = np.asarray(0.0)
            out["u%d_norm_mean" % k] = normalizer._mean.numpy().copy()
            out["u%d_norm_var" % k] = normalizer._var.numpy().copy()
            out["u%d_norm_count" % k] = np.asarray(int(normalizer.count))
            out["u%d_states" % k] = last["states"].detach().numpy().copy()
            out["u%d_actions" % k] = last["actions"].detach().numpy().copy()
            for name, t in (("advs", advs), ("log_probs_old", log_probs_old),
                            ("vs_pred_old", vs_pred_old), ("vs_teacher", vs_teacher)):
                out["u%d_%s" % (k, name)] = t.detach().numpy().copy()
            out["u%d_losses" % k] = np.asarray(
                [float(loss), ag.value_loss_record[-1], ag.policy_loss_record[-1]])
            last["pending"] = k
        return loss

    ag._lossfun = spy_loss
    orig_step = opt.step

    def spy_step(*a, **kw):
        r = orig_step(*a, **kw)
        k = last.pop("pending", None)
        if k is not None:
            out["u%d_params_after" % k] = flat(params)
        return r

    opt.step = spy_step
    experiments.train_agent_batch(ag, env, ROLLOUTS * UPDATE_INTERVAL, tempfile.mkdtemp())
    assert count[0] == UPDATES[-1], count[0]
    assert all("u%d_params_after" % k in out for k in UPDATES)
    out["updates"] = np.asarray(UPDATES)
    # clip_eps, value_func_coef, entropy_coef, lr, Adam eps
    out["hyper"] = np.asarray([0.2, 1.0, 0.0, 3e-4, 1e-5])
    path = os.path.join(HERE, "teacher_forced_ppo_gaussian.npz")
    np.savez_compressed(path, **out)
    print("teacher_forced ppo gaussian", {k: out["u%d_losses" % k].tolist() for k in UPDATES},
          os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
