"""What the policy-loss launches share by construction (csrc/softmax_rows.h, gaussian_rows.h,
row_reduce.h), pinned bit for bit on the same seeded operands.

PPO, A2C and REINFORCE call one categorical row (softmax_row / softmax_grad_row), the four Gaussian
launches one entropy (gaussian_entropy) and one gradient loop (gaussian_grad_columns), and all of
them one wave sum, one workgroup fold and one column fold.  So, with no tolerance:

  * the mean entropy of the same logits is the same float32 from pfrl_ppo_loss, pfrl_a2c_loss and
    pfrl_reinforce_loss: the rows' H are the same numbers, added in the same order;
  * the mean entropy of the three Gaussian losses IS the per-row entropy pfrl_ppo_gaussian_act
    stores: every row contributes the same float32 H, the f64 sum of M <= 2^29 copies of a float32 is
    exact, and so is its division by M;
  * with pi_coef = 1, value = 0, ent_coef = beta and inv_batchsize = fl(1 / M) A2C's row factors are
    gl = fl(fl(1 / M) (-R)) and ge = fl(beta fl(1 / M)), which is what REINFORCE computes (R - 0 is
    R): dlogits and dmean are equal.  dscale is equal where M fl(1 / M) = 1 exactly (M a power of
    two) or beta = 0: REINFORCE's finish subtracts beta M inv_b / s_j in f64, A2C's ent_coef / s_j,
    and for other M the two differ in the f64 factor M fl(1 / M) by design of the two agents
    (batchsize is not M there), so no equality is claimed for those;
  * the log-probability pfrl_ppo_gaussian_act records, fed to pfrl_trpo_gaussian_eval as
    log_prob_old with adv = 1 and entropy_coef = 0, gives ratio 1 in every row and gain
    fl(M / M) = 1 exactly, for every M (tests/test_trpo.py asserts it to 1e-6 only).

M: one block with a tail (1, 65) and two blocks (257); A: the narrowest, an even, an odd and the
widest instantiation.
"""
import functools

import numpy as np
import pytest
import torch

from pfrl_amd import _native
from pfrl_amd.nn import mfma_trunk as mt
from test_actor_critic_envelope import F64, _cd, _dev, _f, _Guarded, _p, _same, _stream

gpu = pytest.mark.gpu

M_LIST = [1, 65, 257]
SOFTMAX_A = [1, 2, 9, 31]
GAUSSIAN_A = [1, 3, 32]
BETA = _f(0.01)
V_COEF = 0.5
DECAY = (0.999, 0.999, 0.999)


def _inv(M):
    return float(np.float32(1) / np.float32(M))


def _done(out):
    torch.cuda.synchronize()
    return {k: t.done(k).cpu() for k, t in out.items()}


@functools.lru_cache(maxsize=None)
def _softmax_operands(M, A):
    g = torch.Generator().manual_seed(7919 * M + A)
    action = torch.randint(0, A, (M,), generator=g)
    return {"z": 2 * torch.randn(M, A, generator=g), "action": action, "action_f32": action.float(),
            "ret": 2 * torch.randn(M, generator=g), "adv": torch.randn(M, generator=g),
            "lpo": -torch.rand(M, generator=g), "vt": torch.randn(M, generator=g),
            "value": torch.randn(M, generator=g), "zero": torch.zeros(M)}


@functools.lru_cache(maxsize=None)
def _gaussian_operands(M, A):
    g = torch.Generator().manual_seed(104723 * M + A)
    mean = torch.randn(M, A, generator=g)
    scale = torch.exp(0.3 * torch.randn(A, generator=g))
    o = _softmax_operands(M, 1)
    return {"mean": mean, "scale": scale, "noise": torch.randn(M, A, generator=g),
            "action": mean + scale * torch.randn(M, A, generator=g), "ret": o["ret"], "adv": o["adv"],
            "lpo": -A * torch.rand(M, generator=g), "vt": o["vt"], "value": o["value"], "zero": o["zero"],
            "one": torch.ones(M)}


def _on(dev, o):
    return {k: t.to(dev).contiguous() for k, t in o.items()}


def _ppo_loss(dev, d, M, A):
    out = {"dz": _Guarded(M * A, dev), "dv": _Guarded(M, dev), "ws": _Guarded(3 * _cd(M, 256), dev, F64),
           "out4": _Guarded(4, dev)}
    mt.check(_native.lib().pfrl_ppo_loss(
        _p(d["z"]), _p(d["value"]), _p(d["action"]), _p(d["adv"]), _p(d["lpo"]), None, _p(d["vt"]), M, A,
        _f(0.2), -1.0, V_COEF, BETA, _p(out["dz"].t), _p(out["dv"].t), _p(out["ws"].t), _p(out["out4"].t),
        _stream()), "ppo_loss")
    return _done(out)


def _a2c_loss(dev, d, M, A, value):
    out = {"dz": _Guarded(M * A, dev), "dv": _Guarded(M, dev), "ws": _Guarded(3 * _cd(M, 256), dev, F64),
           "out3": _Guarded(3, dev)}
    mt.check(_native.lib().pfrl_a2c_loss(
        _p(d["z"]), _p(value), _p(d["action_f32"]), _p(d["ret"]), M, A, 1.0, V_COEF, BETA,
        _p(out["dz"].t), _p(out["dv"].t), _p(out["ws"].t), _p(out["out3"].t), None, *DECAY, _stream()),
        "a2c_loss")
    return _done(out)


def _reinforce_loss(dev, d, M, A):
    out = {"dz": _Guarded(M * A, dev), "ws": _Guarded(2 * _cd(M, 256), dev, F64), "out2": _Guarded(2, dev)}
    mt.check(_native.lib().pfrl_reinforce_loss(
        _p(d["z"]), _p(d["action"]), _p(d["ret"]), M, A, _inv(M), BETA, _p(out["dz"].t), _p(out["ws"].t),
        _p(out["out2"].t), _stream()), "reinforce_loss")
    return _done(out)


def _gaussian_act(dev, d, M, A):
    out = {"action": _Guarded(M * A, dev), "entropy": _Guarded(M, dev), "lp": _Guarded(M, dev)}
    mt.check(_native.lib().pfrl_ppo_gaussian_act(
        _p(d["mean"]), _p(d["scale"]), _p(d["noise"]), _p(d["action"]), _p(out["action"].t),
        _p(out["entropy"].t), _p(out["lp"].t), M, A, _stream()), "ppo_gaussian_act")
    return _done(out)


def _ppo_gaussian_loss(dev, d, M, A):
    out = {"dmean": _Guarded(M * A, dev), "dv": _Guarded(M, dev), "dscale": _Guarded(A, dev),
           "ws": _Guarded((3 + A) * _cd(M, 256), dev, F64), "out4": _Guarded(4, dev)}
    mt.check(_native.lib().pfrl_ppo_gaussian_loss(
        _p(d["mean"]), _p(d["scale"]), _p(d["value"]), _p(d["action"]), _p(d["adv"]), _p(d["lpo"]), None,
        _p(d["vt"]), M, A, _f(0.2), -1.0, V_COEF, BETA, _p(out["dmean"].t), _p(out["dv"].t),
        _p(out["dscale"].t), _p(out["ws"].t), _p(out["out4"].t), _stream()), "ppo_gaussian_loss")
    return _done(out)


def _a2c_gaussian_loss(dev, d, M, A, value, beta=BETA):
    out = {"dmean": _Guarded(M * A, dev), "dv": _Guarded(M, dev), "dscale": _Guarded(A, dev),
           "ws": _Guarded((3 + A) * _cd(M, 256), dev, F64), "out3": _Guarded(3, dev)}
    mt.check(_native.lib().pfrl_a2c_gaussian_loss(
        _p(d["mean"]), _p(d["scale"]), _p(value), _p(d["action"]), _p(d["ret"]), M, A, 1.0, V_COEF, beta,
        _p(out["dmean"].t), _p(out["dv"].t), _p(out["dscale"].t), _p(out["ws"].t), _p(out["out3"].t), None,
        *DECAY, _stream()), "a2c_gaussian_loss")
    return _done(out)


def _reinforce_gaussian_loss(dev, d, M, A, beta=BETA):
    out = {"dmean": _Guarded(M * A, dev), "dscale": _Guarded(A, dev),
           "ws": _Guarded((2 + A) * _cd(M, 256), dev, F64), "out2": _Guarded(2, dev)}
    mt.check(_native.lib().pfrl_reinforce_gaussian_loss(
        _p(d["mean"]), _p(d["scale"]), _p(d["action"]), _p(d["ret"]), M, A, _inv(M), beta,
        _p(out["dmean"].t), _p(out["dscale"].t), _p(out["ws"].t), _p(out["out2"].t), _stream()),
        "reinforce_gaussian_loss")
    return _done(out)


def _shapes(a_list):
    return [(M, A) for M in M_LIST for A in a_list]


@gpu
@pytest.mark.parametrize("M,A", _shapes(SOFTMAX_A))
def test_categorical_rows_are_shared_by_ppo_a2c_and_reinforce(M, A):
    dev = _dev()
    d = _on(dev, _softmax_operands(M, A))
    tag = "M=%d A=%d" % (M, A)
    ppo = _ppo_loss(dev, d, M, A)
    a2c = _a2c_loss(dev, d, M, A, d["value"])
    rf = _reinforce_loss(dev, d, M, A)
    _same("mean entropy, a2c against ppo", tag, a2c["out3"][2], ppo["out4"][3])
    _same("mean entropy, reinforce against ppo", tag, rf["out2"][1], ppo["out4"][3])
    # the entropy column of the workspaces: the same wave and workgroup folds
    _same("entropy partials, a2c against ppo", tag, a2c["ws"].view(-1, 3)[:, 2], ppo["ws"].view(-1, 3)[:, 2])
    _same("entropy partials, reinforce against ppo", tag, rf["ws"].view(-1, 2)[:, 1], ppo["ws"].view(-1, 3)[:, 2])
    # value = 0, pi_coef = 1, ent_coef = beta, inv_batchsize = fl(1 / M): the REINFORCE gradient
    a2c0 = _a2c_loss(dev, d, M, A, d["zero"])
    _same("dlogits, a2c against reinforce", tag, a2c0["dz"], rf["dz"])


@gpu
@pytest.mark.parametrize("M,A", _shapes(GAUSSIAN_A))
def test_gaussian_rows_are_shared_by_ppo_a2c_reinforce_and_trpo(M, A):
    dev = _dev()
    d = _on(dev, _gaussian_operands(M, A))
    tag = "M=%d A=%d" % (M, A)
    act = _gaussian_act(dev, d, M, A)
    row_entropy = act["entropy"][0]
    _same("entropy of every row", tag, act["entropy"], row_entropy.expand(M))
    ppo = _ppo_gaussian_loss(dev, d, M, A)
    a2c = _a2c_gaussian_loss(dev, d, M, A, d["value"])
    rf = _reinforce_gaussian_loss(dev, d, M, A)
    _same("mean entropy, ppo against act", tag, ppo["out4"][3], row_entropy)
    _same("mean entropy, a2c against act", tag, a2c["out3"][2], row_entropy)
    _same("mean entropy, reinforce against act", tag, rf["out2"][1], row_entropy)
    a2c0 = _a2c_gaussian_loss(dev, d, M, A, d["zero"])
    _same("dmean, a2c against reinforce", tag, a2c0["dmean"], rf["dmean"])
    # (the scale-gradient sums before the entropy term: gaussian_grad_columns and the folds)
    _same("scale-gradient partials, a2c against reinforce", tag, a2c0["ws"].view(-1, 3 + A)[:, 3:],
          rf["ws"].view(-1, 2 + A)[:, 2:])
    if M & (M - 1) == 0:
        _same("dscale, a2c against reinforce", tag, a2c0["dscale"], rf["dscale"])
    _same("dscale without an entropy term, a2c against reinforce", tag,
          _a2c_gaussian_loss(dev, d, M, A, d["zero"], beta=0.0)["dscale"],
          _reinforce_gaussian_loss(dev, d, M, A, beta=0.0)["dscale"])
    # ratio exp(log pi - log pi_old) of the unchanged policy is exactly 1 in every row
    lp = act["lp"].to(dev)
    out3, ws = _Guarded(3, dev), _Guarded((2 + A) * _cd(M, 256), dev, F64)
    mt.check(_native.lib().pfrl_trpo_gaussian_eval(
        _p(d["mean"]), _p(d["scale"]), _p(d["mean"]), _p(d["scale"]), _p(d["action"]), _p(d["one"]), _p(lp),
        M, A, 0.0, None, None, _p(ws.t), _p(out3.t), _stream()), "trpo_gaussian_eval")
    torch.cuda.synchronize()
    ws.guards("ws")
    got = out3.done("out3").cpu()
    assert float(got[0]) == 1.0 and float(got[1]) == 0.0, (tag, got)
    _same("entropy, trpo against act", tag, got[2], row_entropy)
