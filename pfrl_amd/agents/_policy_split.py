"""Which models the fused head launches run behind (pfrl_ppo_act_head, pfrl_ppo_head_loss,
pfrl_ppo_gaussian_*, pfrl_a2c_*loss, pfrl_reinforce_*loss, pfrl_trpo_gaussian_eval): pure functions of
a model, for PPO, A2C, REINFORCE and TRPO.  Each returns None for a model it does not recognise, else
views of the model without its head: same classes, same children and parameters, so a fused trunk
stays fused and the model keeps its head.  Switches, stock-method checks and caches stay with the
agents.  At the end: the two policies the acting launches of SAC, TD3 and DDPG run behind
(pfrl_squashed_head_act, pfrl_deterministic_head_act; agents/_actor_device_step.py)."""
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


def hidden_ok(h, lin, N=None):
    """``h`` is what a fused head launch reads in front of ``lin``: [N, in_features] float32,
    contiguous (``N`` None: any number of rows)."""
    return (torch.is_tensor(h) and h.dim() == 2 and h.dtype == torch.float32 and h.is_contiguous()
            and h.shape[1] == lin.in_features and (N is None or h.shape[0] == N))


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


# -------------------------------------------------------------------------------------------------
# the continuous replay agents' acting launches (pfrl_squashed_head_act, pfrl_deterministic_head_act)
# -------------------------------------------------------------------------------------------------
def _act_layer_ok(lin, n_out_per_action):
    """The last ``nn.Linear`` as the acting launches read it: float32, with a bias, contiguous,
    inside the gates of csrc/actor_act.hip."""
    from pfrl_amd.ops import ACTOR_ACT_MAX_A, ACTOR_ACT_MAX_K

    return (isinstance(lin, nn.Linear) and lin.bias is not None and lin.weight.dtype == torch.float32
            and lin.bias.dtype == torch.float32 and lin.weight.is_contiguous()
            and lin.out_features % n_out_per_action == 0
            and 1 <= lin.out_features // n_out_per_action <= ACTOR_ACT_MAX_A
            and 1 <= lin.in_features <= ACTOR_ACT_MAX_K)


class SquashedGaussianSplit(NamedTuple):
    """``body``: the policy without its last layer and head, yielding h [M, K]; ``layer``: the
    ``nn.Linear(K, 2A)``; ``spec``: the ``HeadSpec`` of the head function."""

    body: nn.Module
    layer: nn.Linear
    spec: object


def squashed_gaussian_policy(policy, device, spec=None):
    """:class:`SquashedGaussianSplit` when ``policy`` is ``Sequential(body..., Linear(K, 2A),
    Lambda(head))`` -- the reference's example (examples/mujoco/reproduction/soft_actor_critic/
    train_soft_actor_critic.py:159-179) -- with a non-empty body, float32 parameters, A <= 32,
    K <= 1024 and ``head`` accepted by ``utils.squashed_gaussian.recognise_head`` (probed on
    ``device``; ``spec``: the answer of an earlier probe of this head, taken as it is)."""
    from pfrl_amd.nn import Lambda
    from pfrl_amd.utils import squashed_gaussian

    if not isinstance(policy, nn.Sequential) or len(policy) < 3:
        return None
    lin, head = policy[len(policy) - 2], policy[len(policy) - 1]
    if type(head) is not Lambda or not _act_layer_ok(lin, 2) or not _all_f32(policy):
        return None
    if spec is None:
        spec = squashed_gaussian.recognise_head(head.lambd, lin.out_features, device)
    if spec is None or 2 * spec.A != lin.out_features:
        return None
    return SquashedGaussianSplit(prefix_view(policy, drop=2), lin, spec)


class DeterministicSplit(NamedTuple):
    """``body``: the policy without its last layer and what follows, yielding h [M, K]; ``layer``:
    the ``nn.Linear(K, A)``; ``bound``: the ``BoundByTanh`` behind it, or None."""

    body: nn.Module
    layer: nn.Linear
    bound: Optional[nn.Module]


def deterministic_policy(policy):
    """:class:`DeterministicSplit` when ``policy`` is ``Sequential(body..., Linear(K, A),
    [BoundByTanh], DeterministicHead())`` -- the reference's DDPG example (examples/mujoco/
    reproduction/ddpg/train_ddpg.py:133-141) -- with a non-empty body, float32 parameters, a bias,
    A <= 32 and K <= 1024.  (An ``nn.Tanh`` in place of the ``BoundByTanh``, as in the reference's
    train_td3.py:122-130, is not taken: the agent keeps calling the policy.)"""
    from pfrl_amd.nn import BoundByTanh
    from pfrl_amd.policies import DeterministicHead

    if not isinstance(policy, nn.Sequential) or len(policy) < 3:
        return None
    kids = list(policy._modules.values())
    if type(kids[-1]) is not DeterministicHead:
        return None
    bound = kids[-2] if type(kids[-2]) is BoundByTanh else None
    drop = 2 if bound is None else 3
    if len(kids) <= drop:
        return None
    lin = kids[-drop]
    if not _act_layer_ok(lin, 1) or not _all_f32(policy):
        return None
    return DeterministicSplit(prefix_view(policy, drop=drop), lin, bound)
