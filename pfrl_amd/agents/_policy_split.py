"""Which models the fused head launches run behind (pfrl_ppo_act_head, pfrl_ppo_head_loss,
pfrl_ppo_gaussian_*, pfrl_a2c_*loss, pfrl_reinforce_*loss, pfrl_trpo_gaussian_eval): pure functions of
a model, for PPO, A2C, REINFORCE and TRPO.  Each returns None for a model it does not recognise, else
views of the model without its head: same classes, same children and parameters, so a fused trunk
stays fused and the model keeps its head.  Switches, stock-method checks and caches stay with the
agents."""
import collections
from typing import NamedTuple, Optional

import torch
from torch import nn

from pfrl_amd.nn import Branched
from pfrl_amd.ops import GAUSSIAN_MAX_A
from pfrl_amd.policies import (GaussianHeadWithFixedCovariance,
                               GaussianHeadWithStateIndependentCovariance, SoftmaxCategoricalHead)


def _view(module, children):
    """``module`` again -- same class, same attributes -- over ``children`` ([(name, child)])."""
    view = object.__new__(type(module))
    view.__dict__ = dict(module.__dict__)
    view._modules = collections.OrderedDict(children)
    return view


def prefix_view(seq, drop=1, replacement=None):
    """``seq`` without its last ``drop`` children; ``replacement`` stands in for the first one dropped."""
    items = list(seq._modules.items())
    keep = len(items) - drop
    tail = [] if replacement is None else [(items[keep][0], replacement)]
    return _view(seq, items[:keep] + tail)


def _all_f32(model):
    return all(p.dtype == torch.float32 for p in model.parameters())


def _softmax_layer_ok(pol, head):
    return (isinstance(pol, nn.Linear) and type(head) is SoftmaxCategoricalHead
            and 1 <= pol.out_features <= 31 and pol.bias is not None
            and pol.weight.dtype == torch.float32)


def softmax_actor_critic(model):
    """(body, policy layer, value layer) when ``model`` is ``Sequential(body..., Branched(Sequential(
    Linear(K, A <= 31), SoftmaxCategoricalHead()), Linear(K, 1)))`` -- the reference's example network
    (examples/atari/train_ppo_ale.py:247-264); ``body``: the model without its last child."""
    if not (isinstance(model, nn.Sequential) and len(model) >= 2
            and type(model[len(model) - 1]) is Branched):
        return None
    kids = list(model[len(model) - 1].child_modules)
    if not (len(kids) == 2 and type(kids[0]) is nn.Sequential and len(kids[0]) == 2):
        return None
    pol, head, val = kids[0][0], kids[0][1], kids[1]
    if not (_softmax_layer_ok(pol, head) and isinstance(val, nn.Linear) and val.out_features == 1
            and val.bias is not None and pol.in_features == val.in_features):
        return None
    return prefix_view(model), pol, val


def softmax_policy(model):
    """(body, policy layer) when ``model`` is ``Sequential(body..., Linear(K, A <= 31),
    SoftmaxCategoricalHead())``, a non-empty body, float32 parameters."""
    if type(model) is not nn.Sequential or len(model) < 3:
        return None
    pol, head = model[len(model) - 2], model[len(model) - 1]
    if not (_softmax_layer_ok(pol, head) and _all_f32(model)):
        return None
    return prefix_view(model, drop=2), pol


class GaussianSplit(NamedTuple):
    """``view``: the model without ``head``, yielding the mean [M, A] (an actor-critic model: next to
    the value [M, 1]); ``fixed``: the constant scale [A] of a fixed covariance, else None."""

    view: nn.Module
    head: nn.Module
    A: int
    fixed: Optional[torch.Tensor]

    def scale(self):
        """The policy's scale vector [A]: ``sqrt(var_func(var_param))`` computed by torch, so that any
        ``var_func`` works and its gradient is ``scale.backward(dscale)`` (a spherical variance
        expands to A equal entries); the constant of a fixed-covariance head."""
        if self.fixed is not None:
            return self.fixed
        return torch.sqrt(self.head.var_func(self.head.var_param)).reshape(-1).expand(self.A)


def _headless_gaussian_policy(policy):
    """(``policy`` up to its last Linear, head, A) when ``policy`` is ``Sequential(..., Linear(., A <= 32),
    head)`` with one of the two heads whose scale does not depend on the state."""
    if type(policy) is not nn.Sequential or len(policy) < 2:
        return None
    pol, head = policy[len(policy) - 2], policy[len(policy) - 1]
    if type(head) not in (GaussianHeadWithStateIndependentCovariance, GaussianHeadWithFixedCovariance):
        return None
    if not (isinstance(pol, nn.Linear) and 1 <= pol.out_features <= GAUSSIAN_MAX_A):
        return None
    return prefix_view(policy), head, pol.out_features


def _gaussian_split(model, view, head, A, device):
    """The conditions on the parameters and on the head's own state, then the result."""
    if not _all_f32(model):
        return None
    fixed = None
    if type(head) is GaussianHeadWithFixedCovariance:
        const = torch.as_tensor(head.scale, dtype=torch.float32).to(device)
        if const.numel() not in (1, A) or bool((const <= 0).any()):
            return None
        fixed = const.reshape(-1).expand(A).contiguous()
    elif head.var_param.numel() not in (1, A):
        return None
    return GaussianSplit(view, head, A, fixed)


def gaussian_actor_critic(model, device):
    """:class:`GaussianSplit` when ``model`` is ``Branched(Sequential(..., Linear(., A <= 32), head),
    value branch)`` -- the reference's example (examples/mujoco/reproduction/ppo/train_ppo.py:153-189)
    -- or ``Sequential(body..., Branched(that))``, the head a
    ``GaussianHeadWithStateIndependentCovariance`` (spherical or diagonal, any ``var_func``) or a
    ``GaussianHeadWithFixedCovariance``, all parameters float32.  ``view(x)`` is ``(mean [M, A],
    value [M, 1])``; a fixed scale is put on ``device``."""
    if type(model) is Branched:
        branched = model
    elif (isinstance(model, nn.Sequential) and len(model) >= 2
            and type(model[len(model) - 1]) is Branched):
        branched = model[len(model) - 1]
    else:
        return None
    kids = list(branched.child_modules)
    found = _headless_gaussian_policy(kids[0]) if len(kids) == 2 else None
    if found is None:
        return None
    policy, head, A = found
    view = _view(branched, [("child_modules", nn.ModuleList([policy, kids[1]]))])
    if branched is not model:
        view = prefix_view(model, replacement=view)
    return _gaussian_split(model, view, head, A, device)


def gaussian_policy(model, device):
    """:class:`GaussianSplit` when ``model`` is such a policy branch on its own: ``Sequential(...,
    Linear(., A <= 32), head)``.  ``view(x)`` is the mean [M, A]."""
    found = _headless_gaussian_policy(model)
    if found is None:
        return None
    return _gaussian_split(model, *found, device)
