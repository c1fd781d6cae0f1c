"""The whole-MLP route (ops.mlp_fused) behind ``pfrl_amd.nn.accelerate_mlp`` and the on-policy agents."""
import collections
import copy

import pytest
import torch
from torch import nn

import pfrl_amd
from pfrl_amd import _native
from pfrl_amd.agents import TRPO, trpo
from pfrl_amd.nn import Branched, accelerate_mlp

pytestmark = pytest.mark.gpu
OBS, A, ROWS = 11, 3, 64


def mlp(*sizes, act=nn.Tanh, bias=True):
    mods = []
    for i, o in zip(sizes[:-1], sizes[1:]):
        mods += [nn.Linear(i, o, bias=bias), act()]
    return mods[:-1]


def ppo_model():
    """The model of examples/train_ppo_gaussian_synthetic.py."""
    head = pfrl_amd.policies.GaussianHeadWithStateIndependentCovariance(
        action_size=A, var_type="diagonal", var_func=lambda x: torch.exp(2 * x), var_param_init=0)
    return Branched(nn.Sequential(*mlp(OBS, 64, 64, A), head), nn.Sequential(*mlp(OBS, 64, 64, 1)))


@pytest.fixture
def launches(monkeypatch):
    lib, counts = _native.lib(), collections.Counter()
    for name in ("pfrl_mlp_fwd", "pfrl_mlp_bwd"):
        monkeypatch.setattr(lib, name, lambda *a, _f=getattr(lib, name), _n=name: (counts.update([_n]), _f(*a))[1])
    return counts


def outputs_and_grads(model, x, g_mean, g_value):
    """{name: tensor}: mean and value of ``model(x)`` and every parameter gradient of a weighted sum."""
    model.zero_grad()
    dist, value = model(x)
    (dist.mean * g_mean).sum().add((value * g_value).sum()).backward()
    out = {"mean": dist.mean.detach(), "value": value.detach()}
    out.update({k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None})
    return {k: v.double().cpu() for k, v in out.items()}


def test_module_parity_and_launch_count(monkeypatch, launches):
    torch.manual_seed(3)
    model = ppo_model()
    x, g_mean, g_value = torch.randn(ROWS, OBS), torch.randn(ROWS, A), torch.randn(ROWS, 1)
    ref = outputs_and_grads(copy.deepcopy(model).double(), x.double(), g_mean.double(), g_value.double())
    dev = [t.cuda() for t in (x, g_mean, g_value)]
    on = accelerate_mlp(copy.deepcopy(model).cuda())
    assert list(on.state_dict()) == list(model.state_dict())
    got = outputs_and_grads(on, *dev)
    assert launches == {"pfrl_mlp_fwd": 1, "pfrl_mlp_bwd": 1}     # policy and value function together
    monkeypatch.setenv("PFRL_MLP_FUSED", "0")
    off = outputs_and_grads(accelerate_mlp(copy.deepcopy(model).cuda()), *dev)
    assert launches == {"pfrl_mlp_fwd": 1, "pfrl_mlp_bwd": 1}
    kinds = {"outputs": ("mean", "value"), "weight gradients": [k for k in ref if k.endswith("weight")],
             "bias gradients": [k for k in ref if k.endswith("bias")]}
    for kind, names in kinds.items():
        e_on = max((got[k] - ref[k]).abs().max().item() for k in names)
        e_off = max((off[k] - ref[k]).abs().max().item() for k in names)
        print("%s: route %.3e, route off %.3e" % (kind, e_on, e_off))
        assert e_on <= 2 * e_off, kind


def test_trpo_policy_takes_the_route_with_gradients_off_only(monkeypatch, launches):
    def fisher_vector_product(x, vec):
        torch.manual_seed(5)
        model = ppo_model()
        policy, vf = model.child_modules
        agent = TRPO(policy, vf, torch.optim.Adam(vf.parameters(), lr=1e-3), gpu=0)
        with torch.no_grad():
            n0 = launches["pfrl_mlp_fwd"]
            agent.policy(x)
            routed = launches["pfrl_mlp_fwd"] - n0
        found, params = agent._gaussian_found(), list(agent.policy.parameters())
        n0 = launches["pfrl_mlp_fwd"]
        mean = found.view.child_modules[0](x)
        assert launches["pfrl_mlp_fwd"] == n0                      # differentiated twice: the library
        with torch.no_grad():
            old = found.head(mean.detach())
        kl = torch.mean(torch.distributions.kl_divergence(old, found.head(mean)))
        flat = trpo._flat_grads([kl], params, create_graph=True)
        return routed, trpo._hessian_vector_product(flat, params, vec)

    torch.manual_seed(4)
    x = torch.randn(ROWS, OBS).cuda()
    vec = torch.randn(sum(p.numel() for p in ppo_model().child_modules[0].parameters())).cuda()
    routed, on = fisher_vector_product(x, vec)
    monkeypatch.setenv("PFRL_MLP_FUSED", "0")
    unrouted, off = fisher_vector_product(x, vec)
    assert (routed, unrouted) == (1, 0)
    assert torch.equal(on, off) and bool(on.abs().sum() > 0)


@pytest.mark.parametrize("case", ["mixed", "wide", "no bias", "cpu"])
def test_not_recognised_models_keep_their_result(monkeypatch, launches, case):
    torch.manual_seed(6)
    model = {
        "mixed": lambda: nn.Sequential(nn.Linear(OBS, 64), nn.Tanh(), nn.Linear(64, 64), nn.ReLU(), nn.Linear(64, A)),
        "wide": lambda: nn.Sequential(*mlp(OBS, 65, 64, A)),
        "no bias": lambda: nn.Sequential(*mlp(OBS, 64, 64, A, bias=False)),
        "cpu": lambda: nn.Sequential(*mlp(OBS, 64, 64, A)),
    }[case]()
    x = torch.randn(ROWS, OBS)
    if case != "cpu":
        model, x = model.cuda(), x.cuda()
    on = accelerate_mlp(copy.deepcopy(model))(x)
    monkeypatch.setenv("PFRL_MLP_FUSED", "0")
    off = accelerate_mlp(copy.deepcopy(model))(x)
    assert torch.equal(on, off) and not launches
