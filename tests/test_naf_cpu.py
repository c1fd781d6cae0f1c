"""NAF on the DQN family without a GPU: ``ops.naf_td_loss_closed_form`` (the arithmetic of
pfrl_naf_td_loss restated in torch) against autograd through the reference expression -- the module's
``forward``, ``QuadraticActionValue.evaluate_actions`` / ``max`` / ``greedy_actions``,
``compute_value_loss`` / ``compute_weighted_value_loss`` -- in float64, the decision table of
``agents/_naf_split.py``, and that the module stands apart from the agents that call it.

Tolerance of the float64 comparison: both sides are O(n^2) float64 operations on numbers of
magnitude <= ~1e3 (exp(e) <= e^1.5, |d| <= 4, n <= 17), i.e. absolute errors around 1e-16 * 1e3 * n^2
~ 3e-11 at the very worst; 1e-9 (absolute and relative) is comfortably above that and ten orders of
magnitude below any wrong term."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBS, HID, B = 5, 16, 9
TOL = dict(rtol=1e-9, atol=1e-9)


def make_model(n, scale_mu, seed=0, dtype=torch.float64, low=-1.0, high=1.0):
    import pfrl_amd as pfrl

    torch.manual_seed(seed)
    space = pfrl.spaces.Box(np.linspace(low, low / 2, n), np.linspace(high / 2, high, n), (n,))
    q = pfrl.q_functions.FCQuadraticStateQFunction(OBS, n, HID, 2, space, scale_mu=scale_mu)
    with torch.no_grad():
        # raw heads of some size: mu beyond the box, a diagonal away from 1, real off-diagonals
        for layer, gain in ((q.mu, 6.0), (q.mat_diag, 4.0), (q.v, 3.0)):
            layer.weight.mul_(gain)
            layer.bias.uniform_(-0.5, 0.5)
        if n > 1:
            q.mat_non_diag.weight.mul_(5.0)
    return q.to(dtype)


class Taps:
    """The outputs of the four head layers of one forward pass, kept with their gradients."""

    def __init__(self, q):
        self.out = {}
        self.handles = [getattr(q, name).register_forward_hook(self._hook(name))
                        for name in ("v", "mu", "mat_diag", "mat_non_diag") if hasattr(q, name)]

    def _hook(self, name):
        def hook(module, args, output):
            if output.requires_grad:
                output.retain_grad()
            self.out[name] = output
        return hook

    def close(self):
        for h in self.handles:
            h.remove()

    def raw(self):
        return (self.out["v"], self.out["mu"], self.out["mat_diag"], self.out.get("mat_non_diag"))


def strip_bounds(av):
    from pfrl_amd.action_value import QuadraticActionValue

    return QuadraticActionValue(av.mu, av.mat, av.v)


def make_batch(n, seed, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    r = lambda *shape: torch.rand(*shape, generator=g, dtype=dtype)  # noqa: E731
    return dict(state=r(B, OBS) * 2 - 1, next_state=r(B, OBS) * 2 - 1,
                action=r(B, n) * 3 - 1.5,                   # inside and outside the box
                reward=r(B) * 2 - 1, discount=0.9 + 0.09 * r(B),
                terminal=(r(B) < 0.3).to(dtype), weights=r(B) + 0.5)


def reference(q, target, batch, bounds, double, clip_delta, mean, weighted):
    """loss, y, |delta| and the gradients at the four raw head outputs, by autograd through the
    composite expression of DQN / DoubleDQN."""
    from pfrl_amd.agents.dqn import compute_value_loss, compute_weighted_value_loss
    from pfrl_amd.utils.contexts import evaluating

    taps = Taps(q)
    try:
        qout = q(batch["state"])
        raw = taps.raw()
    finally:
        taps.close()
    y = qout.evaluate_actions(batch["action"])
    with torch.no_grad():
        tav = target(batch["next_state"])
        tav = tav if bounds else strip_bounds(tav)
        if double:
            with evaluating(q):
                nav = q(batch["next_state"])
            nav = nav if bounds else strip_bounds(nav)
            nxt = tav.evaluate_actions(nav.greedy_actions)
        else:
            nxt = tav.max
        t = batch["reward"] + batch["discount"] * (1.0 - batch["terminal"]) * nxt
    acc = "mean" if mean else "sum"
    if weighted:
        loss = compute_weighted_value_loss(y, t, batch["weights"], clip_delta=clip_delta,
                                           batch_accumulator=acc)
    else:
        loss = compute_value_loss(y, t, clip_delta=clip_delta, batch_accumulator=acc)
    loss.backward()
    grads = tuple(None if r is None else r.grad for r in raw)
    return loss.detach(), y.detach(), (y.detach() - t).abs(), grads


def raw_of(q, x):
    taps = Taps(q)
    try:
        with torch.no_grad():
            q(x)
        return tuple(None if r is None else r.detach() for r in taps.raw())
    finally:
        taps.close()


def bound_vectors(q, dtype):
    low = torch.as_tensor(q.action_space.low).to(dtype)
    high = torch.as_tensor(q.action_space.high).to(dtype)
    if not q.scale_mu:
        return None, None, low, high
    return (high - low) / 2, (high + low) / 2, low, high


def closed_form(q, target, batch, bounds, double, clip_delta, mean, weighted):
    from pfrl_amd import ops

    dtype = batch["state"].dtype
    v, m, e, c = raw_of(q, batch["state"])
    tv, tm, te, tc = raw_of(target, batch["next_state"])
    m2 = raw_of(q, batch["next_state"])[1] if double else None
    hw, ce, low, high = bound_vectors(q, dtype)
    return ops.naf_td_loss_closed_form(
        v, m, e, c, tv, tm, te, tc, m2, batch["action"], batch["reward"], batch["discount"],
        batch["terminal"], batch["weights"] if weighted else None, hw, ce,
        low if bounds else None, high if bounds else None, clip_delta, mean)


def place_td_errors(q, target, batch, bounds, double):
    """Rewards such that the first rows have |delta| = 0.25, exactly 1 (both signs), 1 +- 1e-9 and 3:
    those rows are terminal (t = reward), so delta = y - (y - wanted)."""
    y = reference(q, target, batch, bounds, double, True, True, False)[1]
    q.zero_grad()
    wanted = torch.tensor([0.25, 1.0, -1.0, 1.0 - 1e-9, 1.0 + 1e-9, -3.0], dtype=y.dtype)
    k = wanted.numel()
    batch["terminal"][:k] = 1.0
    r = y[:k] - wanted
    for _ in range(8):              # (y - r is rounded: walk r until the difference is the wanted one)
        r = r + ((y[:k] - r) - wanted)
    batch["reward"][:k] = r
    return k


@pytest.mark.parametrize("double", [False, True], ids=["dqn", "double"])
@pytest.mark.parametrize("bounds", [False, True], ids=["free", "box"])
@pytest.mark.parametrize("scale_mu", [False, True], ids=["raw_mu", "tanh_mu"])
@pytest.mark.parametrize("n", [1, 2, 3, 6, 17])
def test_closed_form_equals_autograd_through_the_reference_expression(n, scale_mu, bounds, double):
    q = make_model(n, scale_mu, seed=n)
    target = make_model(n, scale_mu, seed=100 + n)
    batch = make_batch(n, seed=7 * n + 2 * scale_mu + bounds)
    k = place_td_errors(q, target, batch, bounds, double)
    if not scale_mu:
        # some greedy actions of the target pass lie outside the box, in some coordinates only
        tm = raw_of(target, batch["next_state"])[1]
        out = (tm < torch.as_tensor(q.action_space.low)) | (tm > torch.as_tensor(q.action_space.high))
        assert out.any() and (n == 1 or not out.all())
    for clip_delta, mean, weighted in itertools.product([False, True], repeat=3):
        q.zero_grad()
        want = reference(q, target, batch, bounds, double, clip_delta, mean, weighted)
        got = closed_form(q, target, batch, bounds, double, clip_delta, mean, weighted)
        ad = want[2]
        assert bool((ad[:k] == torch.tensor([0.25, 1, 1, 1 - 1e-9, 1 + 1e-9, 3],
                                            dtype=ad.dtype)).sum() >= 4), ad[:k]
        # (y - reward == -1 has no solution where y + 1 needs one more bit than y: one of the two)
        assert bool((ad[1:3] == 1.0).any()), ad[1:3]
        torch.testing.assert_close(got[0], want[0], **TOL)
        torch.testing.assert_close(got[1], want[1], **TOL)
        torch.testing.assert_close(got[2], want[2], **TOL)
        for name, g, w in zip("vmec", got[3], want[3]):
            if n == 1 and name == "c":
                assert g is None and w is None
                continue
            torch.testing.assert_close(g, w, **TOL, msg=lambda s, name=name: "d%s: %s" % (name, s))
    if not bounds and not double:
        # the maximiser is mu' itself: the target value is v'
        tv = raw_of(target, batch["next_state"])[0].reshape(-1)
        t = batch["reward"] + batch["discount"] * (1.0 - batch["terminal"]) * tv
        got = closed_form(q, target, batch, bounds, double, True, True, False)
        assert torch.equal(got[2], (got[1] - t).abs())


# ---- recognition ------------------------------------------------------------------------------------
def test_the_stock_model_is_split_at_its_four_linear_outputs():
    from pfrl_amd import ops
    from pfrl_amd.agents import _naf_split

    for n, scale_mu in ((3, True), (3, False), (1, True), (32, True)):
        q = make_model(n, scale_mu, dtype=torch.float32)
        split = _naf_split.naf_q_function(q, torch.device("cpu"))
        assert split is not None and split.model is q and split.n == n
        before = {k: v.clone() for k, v in q.state_dict().items()}
        x = torch.rand(4, OBS) * 2 - 1
        v, m, e, c = split.raw(x)
        want = raw_of(q, x)
        for a, b in zip((v, m, e, c), want):
            assert (a is None and b is None) or torch.equal(a, b)
        assert (c is None) == (n == 1) and not hasattr(q, "mat_non_diag") == (n == 1)
        assert torch.equal(split.raw_mu(x), want[1])
        hw, ce, low, high = bound_vectors(q, torch.float32)
        assert torch.equal(split.low, low) and torch.equal(split.high, high)
        if scale_mu:
            assert torch.equal(split.half_width, hw) and torch.equal(split.centre, ce)
        else:
            assert split.half_width is None and split.centre is None
        # the raw outputs rebuild the module's own action value
        av = q(x)
        th, mu, L = ops._naf_factor(m, e, c, split.half_width, split.centre)
        torch.testing.assert_close(mu, av.mu, rtol=0, atol=0)
        torch.testing.assert_close(L @ L.transpose(1, 2), av.mat, rtol=1e-6, atol=1e-6)
        assert torch.equal(v, av.v)
        # another copy of the model (the target network) walks its own layers
        other = make_model(n, scale_mu, seed=5, dtype=torch.float32)
        assert torch.equal(split.raw(x, other)[1], raw_of(other, x)[1])
        assert all(torch.equal(before[k], t) for k, t in q.state_dict().items())
        assert list(before) == list(q.state_dict())


def test_anything_but_the_stock_model_is_refused():
    import pfrl_amd as pfrl
    from pfrl_amd.action_value import QuadraticActionValue
    from pfrl_amd.agents import _naf_split

    cpu = torch.device("cpu")
    FCQ = pfrl.q_functions.FCQuadraticStateQFunction

    class Sub(FCQ):
        pass

    class Other(nn.Module):
        def __init__(self):
            super().__init__()
            self.inner = make_model(3, True, dtype=torch.float32)

        def forward(self, x):
            av = self.inner(x)
            return QuadraticActionValue(av.mu, av.mat, av.v)

    space = pfrl.spaces.Box(-1.0, 1.0, (3,))
    assert _naf_split.naf_q_function(Sub(OBS, 3, HID, 2, space), cpu) is None
    overridden = make_model(3, True, dtype=torch.float32)
    overridden.forward = lambda x: FCQ.forward(overridden, x)
    assert _naf_split.naf_q_function(overridden, cpu) is None
    assert _naf_split.naf_q_function(Other(), cpu) is None
    assert _naf_split.naf_q_function(nn.Sequential(nn.Linear(OBS, 3),
                                                   pfrl.q_functions.DiscreteActionValueHead()),
                                     cpu) is None
    assert _naf_split.naf_q_function(make_model(33, True, dtype=torch.float32), cpu) is None
    assert _naf_split.naf_q_function(make_model(3, True, dtype=torch.float64), cpu) is None
    wide = FCQ(OBS, 3, HID, 2, pfrl.spaces.Box(-1.0, 1.0, (3,), dtype=np.float64))
    assert _naf_split.naf_q_function(wide, cpu) is None
    unbounded = FCQ(OBS, 3, HID, 2, pfrl.spaces.Box(-np.inf, np.inf, (3,)), scale_mu=False)
    assert _naf_split.naf_q_function(unbounded, cpu) is None
    swapped = make_model(3, True, dtype=torch.float32)
    swapped.mu = nn.Sequential(swapped.mu)
    assert _naf_split.naf_q_function(swapped, cpu) is None
    assert _naf_split.naf_q_function(make_model(3, True, dtype=torch.float32), cpu) is not None


def test_the_agent_decides_once_per_model_and_the_host_keeps_the_composite_path():
    import pfrl_amd as pfrl

    def agent(q, cls=pfrl.agents.DQN):
        opt = torch.optim.Adam(q.parameters(), lr=1e-3)
        ex = pfrl.explorers.AdditiveGaussian(0.1)
        return cls(q, opt, pfrl.replay_buffers.ReplayBuffer(100), 0.9, ex, gpu=None,
                   replay_start_size=4, minibatch_size=4)

    naf = agent(make_model(3, True, dtype=torch.float32))
    assert not naf._discrete_values() and not naf._fused_td_loss_applicable()
    disc = agent(nn.Sequential(nn.Linear(OBS, 3), pfrl.q_functions.DiscreteActionValueHead()))
    assert disc._discrete_values()                          # (until an action value says otherwise)
    assert disc._discrete_values(disc.model(torch.zeros(1, OBS)))
    assert disc.__dict__["_discrete_values_cache"][1] is True

    class Single(nn.Module):
        def __init__(self):
            super().__init__()
            self.lin = nn.Linear(OBS + 3, 1)

        def forward(self, x):
            from pfrl_amd.action_value import SingleActionValue

            return SingleActionValue(lambda a: self.lin(torch.cat([x, a], 1)).reshape(-1),
                                     lambda: torch.zeros(x.shape[0], 3))

    single = agent(Single())
    assert single._discrete_values()
    assert not single._discrete_values(single.model(torch.zeros(1, OBS)))
    assert not single._discrete_values()
    # the host path of a NAF agent: an update through the composite expression
    batch = make_batch(3, 1, torch.float32)
    exp = dict(state=batch["state"], next_state=batch["next_state"], action=batch["action"],
               reward=batch["reward"], discount=batch["discount"],
               is_state_terminal=batch["terminal"])
    for cls in (pfrl.agents.DQN, pfrl.agents.DoubleDQN):
        ag = agent(make_model(3, True, dtype=torch.float32), cls)
        loss, _ = ag._compute_loss(exp)
        q64 = make_model(3, True, dtype=torch.float32)
        want = reference(q64, ag.target_model, exp | {"terminal": batch["terminal"]}, True,
                         cls is pfrl.agents.DoubleDQN, True, True, False)[0]
        torch.testing.assert_close(loss.detach(), want, rtol=1e-6, atol=1e-6)


# ---- the module stands apart ------------------------------------------------------------------------
AGENT_MODULES = ("pfrl_amd.agents.dqn", "pfrl_amd.agents.double_dqn", "pfrl_amd.agents.graphed_update")

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
import torch
torch.cuda.is_available = lambda: False
import pfrl_amd.agents._naf_split as ns
assert not any(name in sys.modules for name in AGENTS)
assert callable(ns.naf_q_function) and hasattr(ns.NAFSplit, "raw")
print("isolated ok")
"""


def test_the_module_imports_without_the_agents_and_without_a_gpu():
    done = subprocess.run([sys.executable, "-c", ISOLATED_IMPORT % (AGENT_MODULES,), ROOT],
                          capture_output=True, text=True, timeout=120)
    assert done.returncode == 0 and "isolated ok" in done.stdout, done.stderr[-2000:]


def test_the_module_keeps_to_itself():
    import inspect

    from pfrl_amd.agents import _naf_split

    src = inspect.getsource(_naf_split)
    assert "environ" not in src and "pfrl_amd.agents" not in src
