#!/usr/bin/env python
"""Teacher-forced A2C fixture for a Gaussian policy, recorded by running the REFERENCE (pfnet/pfrl)
itself on the CPU.

    python tests/golden/make_a2c_gaussian_fixture.py      (needs the reference, which make_golden.py finds)

The categorical fixture (teacher_forced_a2c.npz, make_teacher_forced.py) has no continuous counterpart.
This script drives the reference's A2C with a small MLP on 8-float observations behind a
``GaussianHeadWithStateIndependentCovariance`` (A = 3), T = 5 steps of N = 4 environments, through
three updates for both ``use_gae`` settings, and records for every update what ONE ``update``
(pfrl/agents/a2c.py:169-213) depends on and produces, under the keys of the categorical fixture:
``gae{0,1}_u{k}_{params, states, actions, rewards, masks, value_preds, losses, returns, params_after}``
and ``gae{0,1}_updates``.  Observations, rewards and episode ends come from a seeded NumPy generator
(no environment is needed: the agent only sees the four lists ``batch_observe`` takes); the loss terms
are read through the moving averages with their decay set to 0 for the update, as make_teacher_forced.py
does.  The whole run is repeated and asserted equal.

Output: tests/golden/teacher_forced_a2c_gaussian.npz (a few tens of kilobytes)
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_golden as mg  # noqa: E402,F401  (puts the reference and the gym shim on sys.path)

OBS, A, T, N, UPDATES = 8, 3, 5, 4, (1, 2, 3)


def make_model(nn_module, head):
    """Branched(policy MLP -> Linear(., A) -> head, value MLP): the shape of the reference's
    examples/mujoco/reproduction/ppo/train_ppo.py, small."""
    torch.manual_seed(97)
    policy = torch.nn.Sequential(torch.nn.Linear(OBS, 16), torch.nn.Tanh(), torch.nn.Linear(16, A), head)
    vf = torch.nn.Sequential(torch.nn.Linear(OBS, 16), torch.nn.Tanh(), torch.nn.Linear(16, 1))
    return nn_module.Branched(policy, vf)


def head_kwargs():
    return dict(action_size=A, var_type="diagonal", var_func=lambda x: torch.exp(2 * x),
                var_param_init=-0.25)


def record():
    import pfrl
    from pfrl import agents
    from pfrl.policies import GaussianHeadWithStateIndependentCovariance

    out = {}
    for use_gae in (True, False):
        pfrl.utils.set_random_seed(0)
        rng = np.random.RandomState(11 + int(use_gae))
        model = make_model(pfrl.nn, GaussianHeadWithStateIndependentCovariance(**head_kwargs()))
        opt = torch.optim.SGD(model.parameters(), lr=1e-2)
        ag = agents.A2C(model, opt, gamma=0.99, num_processes=N, gpu=-1, update_steps=T,
                        use_gae=use_gae, tau=0.95, max_grad_norm=0.5, entropy_coeff=0.01)
        flat = lambda: np.concatenate([p.detach().numpy().ravel() for p in model.parameters()])  # noqa: E731
        count = [0]
        orig = ag.update
        tag = "gae%d" % int(use_gae)

        def spy(_orig=orig, _ag=ag, _count=count, _tag=tag, _flat=flat):
            _count[0] += 1
            k = _count[0]
            if k not in UPDATES:
                return _orig()
            pre = "%s_u%d_" % (_tag, k)
            out[pre + "params"] = _flat()
            for key in ("states", "actions", "rewards", "masks", "value_preds"):
                out[pre + key] = getattr(_ag, key).detach().numpy().copy()
            saved = (_ag.average_actor_loss, _ag.average_value, _ag.average_entropy,
                     _ag.average_actor_loss_decay, _ag.average_value_decay, _ag.average_entropy_decay)
            _ag.average_actor_loss_decay = _ag.average_value_decay = _ag.average_entropy_decay = 0.0
            _ag.average_actor_loss = _ag.average_value = _ag.average_entropy = 0.0
            _orig()
            out[pre + "losses"] = np.asarray([_ag.average_value, _ag.average_actor_loss,
                                              _ag.average_entropy])        # value, action, entropy
            (_, _, _, _ag.average_actor_loss_decay, _ag.average_value_decay,
             _ag.average_entropy_decay) = saved
            _ag.average_actor_loss = saved[0] + (1 - saved[3]) * (out[pre + "losses"][1] - saved[0])
            _ag.average_value = saved[1] + (1 - saved[4]) * (out[pre + "losses"][0] - saved[1])
            _ag.average_entropy = saved[2] + (1 - saved[5]) * (out[pre + "losses"][2] - saved[2])
            out[pre + "returns"] = _ag.returns.numpy().copy()
            out[pre + "params_after"] = _flat()

        ag.update = spy
        obs = [rng.uniform(-1, 1, OBS).astype(np.float32) for _ in range(N)]
        for _ in range(T * max(UPDATES) + 1):
            actions = ag.batch_act(obs)
            assert actions.shape == (N, A)
            rewards = [float(np.float32(o[0] - 0.1 * np.abs(a).sum())) for o, a in zip(obs, actions)]
            dones = [bool(rng.rand() < 0.1) for _ in range(N)]
            obs = [rng.uniform(-1, 1, OBS).astype(np.float32) for _ in range(N)]
            ag.batch_observe(obs, rewards, dones, [False] * N)
        assert count[0] >= max(UPDATES), count
        out[tag + "_updates"] = np.asarray(UPDATES)
    return out


def main():
    out, again = record(), record()
    assert out.keys() == again.keys()
    for k in out:
        assert np.array_equal(out[k], again[k]), "not reproducible: %s" % k
    path = os.path.join(HERE, "teacher_forced_a2c_gaussian.npz")
    np.savez_compressed(path, **out)
    print("teacher_forced a2c gaussian", os.path.getsize(path), "bytes",
          {k: out[k].tolist() for k in out if k.endswith("losses")})


if __name__ == "__main__":
    main()
