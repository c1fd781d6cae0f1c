#!/usr/bin/env python
"""Teacher-forced fixture for DQN and DoubleDQN with a NAF Q-function, recorded by running the
REFERENCE (pfnet/pfrl) itself.

    python tests/golden/make_teacher_forced_naf.py   (build container only: needs the reference checkout)

The reference's DQN / DoubleDQN (pfrl/agents/dqn.py, double_dqn.py) with
``FCQuadraticStateQFunction(5, 3, 32, 2, action_space)`` and ``AdditiveOU`` act on the reference's own
``pfrl.envs.abc.ABC(size=3, discrete=False)`` (the continuous half of examples/gym/train_dqn_gym.py on the
toy problem of the reference's agent tests).  For updates 1, 20 and 60 of each agent it records what
ONE update depends on -- the online and target parameters before the step and the minibatch handed to
``_compute_loss`` -- and what it produced: the loss and the parameters after the Adam step (with the
Adam state before it, so that the step can be repeated).

The archive is written entry by entry with a fixed time stamp, so that the same run gives the same
bytes.

Output: tests/golden/teacher_forced_naf.npz
"""
import io
import os
import sys
import zipfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_golden as mg  # noqa: E402,F401  (puts the reference and the gym shim on sys.path)

OBS, ACT, HIDDEN, LAYERS = 5, 3, 32, 2
UPDATES = (1, 20, 60)
GAMMA, LR, MINIBATCH, START, TARGET_INTERVAL, SIGMA = 0.9, 1e-3, 32, 32, 25, 0.4
BATCH_KEYS = ("state", "next_state", "action", "reward", "discount", "is_state_terminal")


def flat(tensors):
    return np.concatenate([t.detach().numpy().ravel() for t in tensors])


def run(name, agent_cls, out):
    import pfrl
    from pfrl import explorers, replay_buffers
    from pfrl.envs.abc import ABC

    pfrl.utils.set_random_seed(0)
    torch.manual_seed(2468)
    env = ABC(size=ACT, discrete=False)
    q = pfrl.q_functions.FCQuadraticStateQFunction(OBS, ACT, HIDDEN, LAYERS, env.action_space)
    opt = torch.optim.Adam(q.parameters(), lr=LR)
    ag = agent_cls(q, opt, replay_buffers.ReplayBuffer(1000), GAMMA, explorers.AdditiveOU(sigma=SIGMA),
                   gpu=-1, replay_start_size=START, minibatch_size=MINIBATCH, update_interval=1,
                   target_update_interval=TARGET_INTERVAL)
    params = list(q.parameters())
    count = [0]
    pending = []
    orig_loss = ag._compute_loss

    def spy_loss(exp_batch, errors_out=None):
        count[0] += 1
        k = count[0]
        loss = orig_loss(exp_batch, errors_out=errors_out)
        if k in UPDATES:
            pre = "%s_u%d_" % (name, k)
            out[pre + "params"] = flat(params)
            out[pre + "target_params"] = flat(ag.target_model.parameters())
            for key in BATCH_KEYS:
                out[pre + key] = exp_batch[key].detach().numpy().astype(np.float32)
            st = [opt.state.get(p, {}) for p in params]
            if all("exp_avg" in s for s in st):
                out[pre + "exp_avg"] = flat([s["exp_avg"] for s in st])
                out[pre + "exp_avg_sq"] = flat([s["exp_avg_sq"] for s in st])
                out[pre + "step"] = np.asarray(float(st[0]["step"]))
            else:
                out[pre + "step"] = np.asarray(0.0)
            out[pre + "loss"] = np.asarray(float(loss.detach()), dtype=np.float64)
            pending.append(pre)
        return loss

    ag._compute_loss = spy_loss
    orig_step = opt.step

    def spy_step(*a, **kw):
        r = orig_step(*a, **kw)
        if pending:
            out[pending.pop() + "params_after"] = flat(params)
        return r

    opt.step = spy_step
    obs = env.reset()
    while count[0] < UPDATES[-1]:
        action = ag.act(obs)
        obs, reward, done, _ = env.step(action)
        ag.observe(obs, reward, done, False)
        if done:
            obs = env.reset()
    assert all("%s_u%d_params_after" % (name, k) in out for k in UPDATES)
    return {k: float(out["%s_u%d_loss" % (name, k)]) for k in UPDATES}


def save(path, arrays):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def main():
    from pfrl import agents

    out = {}
    losses = {name: run(name, cls, out) for name, cls in (("dqn", agents.DQN),
                                                          ("double_dqn", agents.DoubleDQN))}
    out["updates"] = np.asarray(UPDATES)
    # obs, action dim, hidden width, hidden layers, gamma, lr
    out["hyper"] = np.asarray([OBS, ACT, HIDDEN, LAYERS, GAMMA, LR])
    path = os.path.join(HERE, "teacher_forced_naf.npz")
    save(path, out)
    print("teacher_forced naf", losses, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
