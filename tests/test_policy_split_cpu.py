"""``pfrl_amd.agents._policy_split``: which models the four recognition functions admit, what their
views are, and that the module stands apart from the agents that call it.  No GPU.

The expectations in ``TABLE`` are literals recorded from the code these functions replace, on the
same constructions: ``_ActGraph._split`` / ``_gaussian_split`` around a stand-in agent for the two
actor-critic columns (and, for the bare ``Branched`` rows, a TRPO agent's own graph object),
``reinforce._head_split`` for the two policy-only columns.  They are not derived from the functions
under test."""
import inspect
import os
import subprocess
import sys

import pytest
import torch
from torch import nn

OBS, HID, BATCH = 11, 16, 7
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _exp2(x):
    return torch.exp(2 * x)


# ---- constructions ---------------------------------------------------------------------------------
def softmax_ac(A=4, pol_bias=True, val_out=1, val_in=HID, head=None, branched=None, seq=nn.Sequential,
               extra=False):
    import pfrl_amd as pfrl

    head = head or pfrl.policies.SoftmaxCategoricalHead()
    branch = [nn.Linear(HID, A, bias=pol_bias)] + ([nn.Identity()] if extra else []) + [head]
    return seq(nn.Linear(OBS, HID), nn.Tanh(),
               (branched or pfrl.nn.Branched)(nn.Sequential(*branch), nn.Linear(val_in, val_out)))


def softmax_pi(A=4, pol_bias=True, head=None, seq=nn.Sequential, short=False):
    import pfrl_amd as pfrl

    head = head or pfrl.policies.SoftmaxCategoricalHead()
    if short:
        return seq(nn.Linear(OBS, A, bias=pol_bias), head)
    return seq(nn.Linear(OBS, HID), nn.Tanh(), nn.Linear(HID, A, bias=pol_bias), head)


def gaussian(form, A=3, head="spherical", out=None, branch_of_one=False):
    """``form``: "bare" = Branched(policy, vf), "wrapped" = Sequential(body..., Branched(policy branch,
    value layer)), "policy" = the policy branch on its own."""
    import pfrl_amd as pfrl

    P = pfrl.policies
    if head in ("spherical", "diagonal"):
        head = P.GaussianHeadWithStateIndependentCovariance(action_size=A, var_type=head,
                                                            var_param_init=0.5)
    elif head == "var_func":
        head = P.GaussianHeadWithStateIndependentCovariance(action_size=A, var_type="diagonal",
                                                            var_func=_exp2, var_param_init=0.1)
    out = out or A
    if form == "wrapped":
        branch = nn.Sequential(head) if branch_of_one else nn.Sequential(nn.Linear(HID, out), head)
        return nn.Sequential(nn.Linear(OBS, HID), nn.Tanh(), pfrl.nn.Branched(branch, nn.Linear(HID, 1)))
    policy = (nn.Sequential(head) if branch_of_one else
              nn.Sequential(nn.Linear(OBS, HID), nn.Tanh(), nn.Linear(HID, out), head))
    if form == "policy":
        return policy
    assert form == "bare"
    return pfrl.nn.Branched(policy, nn.Sequential(nn.Linear(OBS, HID), nn.Tanh(), nn.Linear(HID, 1)))


def _subclasses():
    import pfrl_amd as pfrl

    class MySoftmax(pfrl.policies.SoftmaxCategoricalHead):
        pass

    class MyGaussian(pfrl.policies.GaussianHeadWithStateIndependentCovariance):
        pass

    class MyBranched(pfrl.nn.Branched):
        pass

    class MySequential(nn.Sequential):
        pass

    return MySoftmax, MyGaussian, MyBranched, MySequential


def _fixed(scale):
    import pfrl_amd as pfrl

    return pfrl.policies.GaussianHeadWithFixedCovariance(scale=scale)


def _gaussian_rows():
    """(id, construction by form, recognised) -- the same verdict for all three forms, in the
    column that the form belongs to."""
    import pfrl_amd as pfrl

    MyGaussian = _subclasses()[1]
    return [
        ("spherical", lambda f: gaussian(f, head="spherical"), True),
        ("diagonal", lambda f: gaussian(f, head="diagonal"), True),
        ("var_func", lambda f: gaussian(f, head="var_func"), True),
        ("A1", lambda f: gaussian(f, A=1, head="diagonal"), True),
        ("A32", lambda f: gaussian(f, A=32, head="diagonal"), True),
        ("A33", lambda f: gaussian(f, A=33, head="diagonal"), False),
        ("fixed_scalar", lambda f: gaussian(f, head=_fixed(0.4)), True),
        ("fixed_vector", lambda f: gaussian(f, head=_fixed(torch.tensor([0.4, 0.5, 0.6]))), True),
        ("fixed_wrong_length", lambda f: gaussian(f, head=_fixed(torch.tensor([0.4, 0.5]))), False),
        ("fixed_non_positive", lambda f: gaussian(f, head=_fixed(torch.tensor([0.4, 0.0, 0.6]))), False),
        ("state_dependent", lambda f: gaussian(
            f, head=pfrl.policies.GaussianHeadWithDiagonalCovariance(), out=6), False),
        ("head_subclass", lambda f: gaussian(f, head=MyGaussian(action_size=3)), False),
        ("double", lambda f: gaussian(f).double(), False),
        ("branch_of_one", lambda f: gaussian(f, branch_of_one=True), False),
        ("diagonal_var_of_two", lambda f: gaussian(
            f, head=pfrl.policies.GaussianHeadWithStateIndependentCovariance(2, var_type="diagonal")),
         False),
    ]


def _table():
    """(id, construction, (softmax_actor_critic, softmax_policy, gaussian_actor_critic,
    gaussian_policy) recognised)."""
    MySoftmax, _, MyBranched, MySequential = _subclasses()
    ac, pi = (True, False, False, False), (False, True, False, False)
    no = (False, False, False, False)
    rows = [
        ("softmax_ac-A1", lambda: softmax_ac(A=1), ac),
        ("softmax_ac-A4", lambda: softmax_ac(), ac),
        ("softmax_ac-A31", lambda: softmax_ac(A=31), ac),
        ("softmax_ac-A32", lambda: softmax_ac(A=32), no),
        ("softmax_ac-policy_without_bias", lambda: softmax_ac(pol_bias=False), no),
        ("softmax_ac-value_of_two", lambda: softmax_ac(val_out=2), no),
        ("softmax_ac-unequal_in_features", lambda: softmax_ac(val_in=HID + 1), no),
        ("softmax_ac-head_subclass", lambda: softmax_ac(head=MySoftmax()), no),
        ("softmax_ac-branched_subclass", lambda: softmax_ac(branched=MyBranched), no),
        ("softmax_ac-sequential_subclass", lambda: softmax_ac(seq=MySequential), ac),
        ("softmax_ac-double", lambda: softmax_ac().double(), no),
        ("softmax_ac-branch_of_three", lambda: softmax_ac(extra=True), no),
        ("softmax_pi-A1", lambda: softmax_pi(A=1), pi),
        ("softmax_pi-A4", lambda: softmax_pi(), pi),
        ("softmax_pi-A31", lambda: softmax_pi(A=31), pi),
        ("softmax_pi-A32", lambda: softmax_pi(A=32), no),
        ("softmax_pi-policy_without_bias", lambda: softmax_pi(pol_bias=False), no),
        ("softmax_pi-two_children", lambda: softmax_pi(short=True), no),
        ("softmax_pi-sequential_subclass", lambda: softmax_pi(seq=MySequential), no),
        ("softmax_pi-head_subclass", lambda: softmax_pi(head=MySoftmax()), no),
        ("softmax_pi-double", lambda: softmax_pi().double(), no),
    ]
    for name, make, ok in _gaussian_rows():
        for form, col in (("bare", 2), ("wrapped", 2), ("policy", 3)):
            want = tuple(ok and i == col for i in range(4))
            rows.append(("gaussian_%s-%s" % (form, name), (lambda make=make, form=form: make(form)), want))
    return rows


TABLE = _table()


def _recognise(model):
    from pfrl_amd.agents import _policy_split as ps

    cpu = torch.device("cpu")
    return (ps.softmax_actor_critic(model), ps.softmax_policy(model),
            ps.gaussian_actor_critic(model, cpu), ps.gaussian_policy(model, cpu))


def _pre_head(model, x):
    """What the model hands its head on ``x``, and what the model returns."""
    import pfrl_amd as pfrl

    P = pfrl.policies
    seen = []
    heads = [m for m in model.modules() if isinstance(m, (
        P.SoftmaxCategoricalHead, P.GaussianHeadWithStateIndependentCovariance,
        P.GaussianHeadWithFixedCovariance, P.GaussianHeadWithDiagonalCovariance))]
    assert len(heads) == 1
    hook = heads[0].register_forward_hook(lambda mod, args, out: seen.append(args[0]))
    try:
        out = model(x)
    finally:
        hook.remove()
    assert len(seen) == 1
    return seen[0], out


@pytest.mark.parametrize("name,make,want", TABLE, ids=[row[0] for row in TABLE])
def test_decision_table(name, make, want):
    torch.manual_seed(3)
    model = make()
    found = _recognise(model)
    assert tuple(f is not None for f in found) == want, name
    if not any(want):
        return
    x = torch.randn(BATCH, OBS, dtype=next(model.parameters()).dtype)
    with torch.no_grad():
        pre, out = _pre_head(model, x)
        if found[0] is not None:
            body, pol, val = found[0]
            assert torch.equal(pol(body(x)), pre) and torch.equal(val(body(x)), out[1])
        if found[1] is not None:
            body, pol = found[1]
            assert torch.equal(pol(body(x)), pre)
        if found[2] is not None:
            mean, value = found[2].view(x)
            assert tuple(value.shape) == (BATCH, 1)
            assert torch.equal(mean, pre) and torch.equal(value, out[1])
        if found[3] is not None:
            assert torch.equal(found[3].view(x), pre)
        for f in found[2:]:
            if f is not None:
                assert tuple(pre.shape) == (BATCH, f.A) and tuple(f.scale().shape) == (f.A,)


def test_prefix_view():
    from pfrl_amd.agents._policy_split import prefix_view

    class MySequential(nn.Sequential):
        pass

    seq = MySequential(nn.Linear(3, 4), nn.Tanh(), nn.Linear(4, 2), nn.ReLU())
    seq.tag = "kept"
    for drop in (1, 2, 4):
        view = prefix_view(seq, drop=drop)
        assert type(view) is MySequential and view.tag == "kept"
        assert list(view._modules) == list(seq._modules)[:4 - drop]
        assert all(a is b for a, b in zip(view, seq))
    other = nn.Identity()
    view = prefix_view(seq, replacement=other)
    assert list(view._modules) == list(seq._modules) and view[3] is other and view[2] is seq[2]
    assert len(seq) == 4 and seq[3] is not other            # the model itself is untouched


VIEWED = {
    "softmax_ac": lambda: softmax_ac(),
    "softmax_pi": lambda: softmax_pi(),
    "gaussian_bare": lambda: gaussian("bare", head="var_func"),
    "gaussian_wrapped": lambda: gaussian("wrapped", head="spherical"),
    "gaussian_policy": lambda: gaussian("policy", head="diagonal"),
    "gaussian_bare_fixed": lambda: gaussian("bare", head=_fixed(0.4)),
    "gaussian_policy_fixed": lambda: gaussian("policy", head=_fixed(torch.tensor([0.4, 0.5, 0.6]))),
}


@pytest.mark.parametrize("form", sorted(VIEWED))
def test_view_properties(form):
    torch.manual_seed(4)
    model = VIEWED[form]()
    keys = list(model.state_dict())
    params = [p.data_ptr() for p in model.parameters()]
    (found,) = [f for f in _recognise(model) if f is not None]
    view = found[0]
    assert type(view) is type(model)
    # a view: the model keeps its head and its parameters, the same parameters sit behind both
    x = torch.randn(BATCH, OBS)
    out = model(x)
    distrib = out[0] if isinstance(out, tuple) else out
    assert isinstance(distrib, torch.distributions.Distribution)
    assert list(model.state_dict()) == keys
    assert [p.data_ptr() for p in model.parameters()] == params
    assert {p.data_ptr() for p in view.parameters()} <= set(params)
    assert not any(p.is_meta for m in (model, view) for p in m.parameters())
    if not form.startswith("gaussian"):
        return
    scale = found.scale()
    A = found.A
    assert tuple(scale.shape) == (A,)
    assert torch.equal(scale.expand(BATCH, A), distrib.base_dist.scale.expand(BATCH, A))
    if form.endswith("fixed"):
        assert found.fixed is not None and not scale.requires_grad and found.scale() is scale
        return
    # the gradient of a learnable variance: through the result's scale and through the head's own
    # graph.  (Small whole numbers in g: every partial sum of a broadcast's backward is exact, so
    # the order in which either graph adds them cannot show.)
    var_param = found.head.var_param
    g = torch.tensor([3.0, -2.0, 5.0])[:A]
    scale.backward(g)
    got = var_param.grad.clone()
    var_param.grad = None
    distrib.base_dist.scale[0].backward(g)
    assert got.abs().sum() > 0 and torch.equal(got, var_param.grad)


AGENT_MODULES = ("pfrl_amd.agents.ppo", "pfrl_amd.agents.a2c", "pfrl_amd.agents.reinforce",
                 "pfrl_amd.agents.trpo")

ISOLATED_IMPORT = """
import importlib.abc, os, sys, types

AGENTS = %r
root = sys.argv[1]
sys.path.insert(0, root)


class Refuse(importlib.abc.MetaPathFinder):
    def find_spec(self, name, path, target=None):
        if name in AGENTS:
            raise ImportError("the module under test asked for " + name)


sys.meta_path.insert(0, Refuse())
# the packages as bare namespaces: ``pfrl_amd/__init__.py`` and ``agents/__init__.py`` import every
# agent, which is the packages' doing and would hide what the module itself asks for
for name, path in (("pfrl_amd", os.path.join(root, "pfrl_amd")),
                   ("pfrl_amd.agents", os.path.join(root, "pfrl_amd", "agents"))):
    pkg = types.ModuleType(name)
    pkg.__path__ = [path]
    sys.modules[name] = pkg
assert not any(name in sys.modules for name in AGENTS)
import pfrl_amd.agents._policy_split as ps
assert not any(name in sys.modules for name in AGENTS)
assert callable(ps.prefix_view) and callable(ps.softmax_actor_critic) and callable(ps.softmax_policy)
assert callable(ps.gaussian_actor_critic) and callable(ps.gaussian_policy)
print("isolated ok")
"""


def test_the_module_imports_without_the_agents():
    """In a fresh interpreter, with the four agent modules refused outright: the module and all it
    imports load, and none of the four is in ``sys.modules`` before or after."""
    done = subprocess.run([sys.executable, "-c", ISOLATED_IMPORT % (AGENT_MODULES,), ROOT],
                          capture_output=True, text=True, timeout=120)
    assert done.returncode == 0 and "isolated ok" in done.stdout, done.stderr[-2000:]


def test_the_module_keeps_to_itself():
    from pfrl_amd.agents import _policy_split

    src = inspect.getsource(_policy_split)
    assert "environ" not in src and "pfrl_amd.agents" not in src


def test_the_agents_are_stand_alone():
    from pfrl_amd.agents import a2c, reinforce

    for mod in (a2c, reinforce):
        assert not hasattr(mod, "_PolicyOnly")
        assert "_ActGraph" not in inspect.getsource(mod)
