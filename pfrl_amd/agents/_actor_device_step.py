"""The batched acting step of the continuous replay agents (SAC, TD3, DDPG) on the device.

``SoftActorCritic.batch_select_greedy_action`` and ``ReplayActorCritic._batch_select_actions`` /
``batch_act`` (reference pfrl/agents/soft_actor_critic.py:317-352, td3.py:262-281, ddpg.py:253-273)
upload the observations from pageable memory, run the policy launch by launch, build a distribution
object to sample from, come back with ``.cpu().numpy()`` and -- TD3 / DDPG -- loop over the envs
calling ``explorer.select_action``.  Here one step is

* one pinned staging slot: the observations (phi is a plain cast) and, for an exploring step, the
  explorer's noise rows [N, A] with its two bound rows behind them -- the noise never depends on the
  actions, so the host draws it first, on NumPy's global stream, exactly as N successive
  ``select_action`` calls would (:func:`gaussian_noise`, :func:`ou_noise`);
* one ``pfrl_h2d_async`` into the input block of a captured graph and one replay: the policy body as
  the model has it, then ONE launch for the last layer and everything behind it
  (``pfrl_squashed_head_act``: chunk / clamp / exp / sqrt / normal / tanh; ``pfrl_deterministic_head_act``:
  BoundByTanh, + noise, clip).  SAC's standard-normal draw is ``torch.randn``'s inside the graph:
  what ``Normal.sample`` draws, at the generator offsets it would use;
* one copy of the actions into pinned memory and one event to wait for.

The graph is a single-stream chain.  It is keyed by N, training / evaluation and the explorer kind
(and by the policy's module tree) and reads the parameters in place: optimizer steps need no new
capture.  ``PFRL_ACTOR_ACT_GRAPH=0`` makes the same launches without capture;
``PFRL_ACTOR_ACT_HEAD=0`` runs the agents' own acting code.

Everything here is a fast path with the agents' code behind it: :func:`squashed_act` and
:func:`deterministic_act` return None -- having touched nothing, no generator included -- when the
policy, ``phi``, the observations or the explorer are not what the step restates (the conditions
are the functions below; tests/test_actor_act_cpu.py holds the table).
"""
import logging
import os

import numpy as np
import torch

from pfrl_amd import ops
from pfrl_amd.agents import _capture, _policy_split
from pfrl_amd.agents._policy_split import hidden_ok
from pfrl_amd.staging import StagingRing, _align16
from pfrl_amd.utils.contexts import evaluating

GREEDY, GAUSSIAN, OU = "greedy", "gaussian", "ou"       # explorer kinds of the deterministic step
SAMPLE, MODE = "sample", "mode"                         # ... and of the squashed-Gaussian step

# how many steps took this path / how many graphs were captured, over all agents of the process
# (what the tests assert the path by)
calls = 0
captures = 0


def head_enabled():
    return os.environ.get("PFRL_ACTOR_ACT_HEAD", "1") != "0"


def graph_enabled():
    return os.environ.get("PFRL_ACTOR_ACT_GRAPH", "1") != "0"


# -------------------------------------------------------------------------------------------------
# the explorers restated (host, NumPy's global stream)
# -------------------------------------------------------------------------------------------------
def _own_methods(ex, cls, names):
    """``ex`` is exactly ``cls`` and none of ``names`` is patched on the instance."""
    return type(ex) is cls and not any(n in vars(ex) for n in names)


def _bound_row(b, A, absent):
    """One side of ``AdditiveGaussian``'s clip as the float32 row [A] the kernel compares with, or
    None when ``np.clip(float32 action, ...)`` with it is not a float32 comparison: None (``absent``:
    the infinity that never clips), a Python int / float (weak: cast to float32) or a float32 array
    of one or A elements.  Anything else -- a float64 array or NumPy scalar would make the reference
    return float64 -- and NaN bounds (``np.maximum`` propagates them, the kernel's compare does not)
    are refused."""
    if b is None:
        return np.full(A, absent, dtype=np.float32)
    if type(b) in (int, float):
        with np.errstate(over="ignore"):
            v = np.float32(b)
        if np.isnan(v) or (np.isinf(v) and not np.isinf(float(b))):
            return None
        return np.full(A, v, dtype=np.float32)
    if (isinstance(b, np.ndarray) and b.dtype == np.float32 and b.ndim <= 1 and b.size in (1, A)
            and not np.isnan(b).any()):
        return np.broadcast_to(b.reshape(-1), (A,))
    return None


def gaussian_bounds(ex, A):
    """(low [A], high [A]) float32 of an ``AdditiveGaussian``, or None (:func:`_bound_row`)."""
    low, high = _bound_row(ex.low, A, -np.inf), _bound_row(ex.high, A, np.inf)
    if low is None or high is None:
        return None
    return low, high


def explorer_kind(ex, A):
    """The kind under which the deterministic step restates ``ex`` for actions of width ``A``, or
    None: exactly ``Greedy``, ``AdditiveGaussian`` (bounds: :func:`gaussian_bounds`) or
    ``AdditiveOU`` (a noise state that is None or float32 of shape (A,), no DEBUG logging of it),
    each with its own ``select_action``."""
    from pfrl_amd.explorers.additive_gaussian import AdditiveGaussian
    from pfrl_amd.explorers.additive_ou import AdditiveOU
    from pfrl_amd.explorers.greedy import Greedy

    if _own_methods(ex, Greedy, ("select_action",)):
        return GREEDY
    if _own_methods(ex, AdditiveGaussian, ("select_action",)):
        return GAUSSIAN if gaussian_bounds(ex, A) is not None else None
    if _own_methods(ex, AdditiveOU, ("select_action", "evolve")):
        s = ex.ou_state
        if s is not None and not (isinstance(s, np.ndarray) and s.dtype == np.float32
                                  and s.shape == (A,)):
            return None
        if ex.logger.isEnabledFor(logging.DEBUG):
            return None
        return OU
    return None


def gaussian_noise(ex, out):
    """``out`` [N, A] f32 <- what N successive ``AdditiveGaussian.select_action`` calls add to their
    actions (pfrl/explorers/additive_gaussian.py:26-36): one ``normal`` of the action's shape each."""
    N, A = out.shape
    for i in range(N):
        out[i] = np.random.normal(scale=ex.scale, size=(A,)).astype(np.float32)


def ou_noise(ex, out):
    """``out`` [N, A] f32 <- what N successive ``AdditiveOU.select_action`` calls add to their
    actions (pfrl/explorers/additive_ou.py:49-66): ``select_action`` without its last line, on the
    explorer's own state -- created on the first call (at ``mu``, or drawn from the stationary
    distribution), evolved in place (float32 ``+=``) on every later one; row i is the state after
    call i.  One state for all envs, as in the reference; the explorer is left as the loop would
    leave it."""
    N, A = out.shape
    for i in range(N):
        if ex.ou_state is not None:
            ex.evolve()
        elif ex.start_with_mu:
            ex.ou_state = np.full((A,), ex.mu, dtype=np.float32)
        else:
            stationary = ex.sigma / np.sqrt(2 * ex.theta - ex.theta ** 2)
            ex.ou_state = np.random.normal(size=(A,), loc=ex.mu, scale=stationary).astype(np.float32)
        out[i] = ex.ou_state


# -------------------------------------------------------------------------------------------------
# conditions on the agent and the observations
# -------------------------------------------------------------------------------------------------
def observation_shape(batch_obs):
    """The common shape of plain floating-point observation arrays, or None."""
    if not isinstance(batch_obs, (list, tuple, np.ndarray)) or len(batch_obs) == 0:
        return None
    first = batch_obs[0]
    if not (isinstance(first, np.ndarray) and first.dtype.kind == "f" and first.ndim >= 1
            and first.size > 0):
        return None
    for o in batch_obs:
        if not (isinstance(o, np.ndarray) and o.dtype == first.dtype and o.shape == first.shape):
            return None
    return first.shape


_phi_cache = {}


def _phi_is_cast(agent, sample_obs):
    """``phi(x) == float32(x)`` for observations of this dtype (``recognise_phi``: evaluated on the
    observation and on a probe; kept per phi and dtype), behind the stock ``batch_states``."""
    import importlib

    from pfrl_amd.device_store import recognise_phi

    bs = importlib.import_module("pfrl_amd.utils.batch_states")     # (the package re-exports the function)
    if agent.batch_states is not bs.batch_states:
        return False
    phi = agent.phi
    key = (id(phi), sample_obs.dtype.str)
    hit = _phi_cache.get(key)
    if hit is not None and hit[0] is phi:
        return hit[1] == 1.0
    d = recognise_phi(phi, sample_obs)
    if d is not None or bool(np.any(sample_obs != 0)):      # (an all-zero sample is inconclusive)
        if len(_phi_cache) > 64:
            _phi_cache.clear()
        _phi_cache[key] = (phi, d)
    return d == 1.0


def _split_of(agent, policy, recognise):
    """``recognise(policy)``, kept per policy object and module tree."""
    tree = tuple(id(m) for m in policy.modules())
    hit = agent.__dict__.get("_actor_act_split")
    if hit is not None and hit[0] is policy and hit[1] == tree:
        return hit[2]
    out = recognise(policy)
    agent._actor_act_split = (policy, tree, out)
    return out


def _bound_vectors(agent, bound, A):
    """The two vectors [A] ``BoundByTanh`` multiplies and adds with on the agent's device -- its own
    (made by calling it once, kept by it per device and dtype) -- or None when they are not one
    value or A.  Kept per module."""
    hit = agent.__dict__.get("_actor_act_bound")
    if hit is not None and hit[0] is bound:
        return hit[1]
    probe = torch.zeros((1, A), dtype=torch.float32, device=agent.device)
    with torch.no_grad():
        bound(probe)
    consts = bound._consts[(probe.device, probe.dtype)]
    out = None
    if all(c.numel() in (1, A) and c.dtype == torch.float32 for c in consts):
        out = tuple(c.reshape(-1).expand(A).contiguous() for c in consts)
    agent._actor_act_bound = (bound, out)
    return out


# -------------------------------------------------------------------------------------------------
# the step
# -------------------------------------------------------------------------------------------------
class _Entry:
    """One captured graph (or, uncaptured, nothing but the fact that the launches take this key)."""

    __slots__ = ("graph", "inp", "out")

    def __init__(self, graph, inp, out):
        self.graph, self.inp, self.out = graph, inp, out


class ActorStep:
    """Staging ring, pinned action block and graphs of one agent."""

    def __init__(self, agent):
        self.device = agent.device
        self.entries = {}
        self.pool = None
        self.ring = None
        self.pinned = None
        self.event = torch.cuda.Event()

    def _views(self, block, N, shape, A, rows):
        D = int(np.prod(shape))
        obs = block[:4 * N * D].view(torch.float32).view((N,) + tuple(shape))
        off = _align16(4 * N * D)
        noise = block[off:off + 4 * rows * A].view(torch.float32).view(rows, A) if rows else None
        return obs, noise

    def _prepare(self, launch, N, shape, A, rows, need):
        """Warm-up of ``launch(obs, noise, out)`` on zeros with the device generator put back behind
        it, then -- unless switched off -- the capture.  False: the policy body does not yield what
        the head launch reads."""
        global captures
        dev = self.device
        inp = torch.zeros(_align16(need), dtype=torch.uint8, device=dev)
        out = torch.empty((N, A), dtype=torch.float32, device=dev)
        obs, noise = self._views(inp, N, shape, A, rows)

        def body(i=None):
            if launch(obs, noise, out) is None:
                return _capture.REFUSED

        snap = _capture.Snapshot((), (), dev)       # (the generator: warm-up draws are not part of the run)
        try:
            if not _capture.warm_up(dev, body):
                return False
        finally:
            snap.restore()
        if not graph_enabled():
            return _Entry(None, None, None)
        g, _ = _capture.capture(self, body)
        captures += 1
        return _Entry(g, inp, out)

    def run(self, key, launch, batch_obs, shape, A, fill):
        """One step: None when ``launch`` does not take this key, else the actions, a fresh float32
        ndarray [N, A].  ``fill(rows)``: writes the noise rows [N, A] and the two bound rows into the
        staging slot (None: a step without noise); called once it is certain that the step runs."""
        global calls
        N = len(batch_obs)
        D = int(np.prod(shape))
        rows = N + 2 if fill is not None else 0
        off = _align16(4 * N * D)
        need = off + 4 * rows * A
        e = self.entries.get(key)
        if e is None:
            if len(self.entries) > 16:
                self.entries.clear()
            e = self.entries[key] = self._prepare(launch, N, shape, A, rows, need)
        if e is False:
            return None
        if self.ring is None or self.ring.slot_bytes < need:
            self.ring = StagingRing(self.device, slot_bytes=max(1 << 14, need + 64), n_slots=4)
        if self.pinned is None or self.pinned.numel() < N * A:
            self.pinned = torch.empty(max(1024, N * A), dtype=torch.float32).pin_memory()
        host, tok = self.ring.reserve()
        obs_host = host[:4 * N * D].view(np.float32).reshape((N,) + tuple(shape))
        for i, o in enumerate(batch_obs):
            obs_host[i] = o                        # (phi: the cast to float32)
        if fill is not None:
            fill(host[off:need].view(np.float32).reshape(rows, A))
        if e.graph is not None:
            self.ring.commit_to(tok, need, e.inp)
            e.graph.replay()
            out = e.out
        else:
            obs, noise = self._views(self.ring.commit(tok, need), N, shape, A, rows)
            out = launch(obs, noise, None)
        flat = self.pinned[:N * A]
        flat.copy_(out.reshape(-1), non_blocking=True)
        self.event.record()
        self.event.synchronize()
        calls += 1
        return flat.numpy().reshape(N, A).copy()


def _step_of(agent):
    st = agent.__dict__.get("_actor_act_step")
    if st is None:
        st = agent._actor_act_step = ActorStep(agent)
    return st


def _applicable(agent, batch_obs):
    """The observations' shape when device, switch, ``phi`` and observations allow the step."""
    if agent.device.type != "cuda" or not head_enabled():
        return None
    shape = observation_shape(batch_obs)
    if shape is None or not _phi_is_cast(agent, batch_obs[0]):
        return None
    return shape


def squashed_act(agent, batch_obs, deterministic):
    """``SoftActorCritic.batch_select_greedy_action``: the actions [N, A] float32, or None."""
    shape = _applicable(agent, batch_obs)
    if shape is None:
        return None
    policy = agent.policy
    split = _split_of(agent, policy, lambda p: _policy_split.squashed_gaussian_policy(
        p, agent.device, spec=agent.__dict__.get("_policy_head")))
    if split is None:
        return None
    from pfrl_amd.utils.squashed_gaussian import _eps

    body, lin, spec = split
    N, A = len(batch_obs), spec.A
    if N > ops.ACTOR_ACT_MAX_M:
        return None

    def launch(obs, noise, out):
        with torch.no_grad(), evaluating(policy):
            h = body(obs)
            if not hidden_ok(h, lin, N):
                return None
            # the draw Normal.sample makes (torch.normal's normal_ on [N, A]): same generator offsets
            eps = None if deterministic else _eps((N, A), torch.float32, h.device)
            return ops.squashed_head_act(h, lin.weight, lin.bias, spec, eps, out=out)[0]

    kind = MODE if deterministic else SAMPLE
    key = (N, shape, bool(agent.training), kind, id(policy), tuple(id(m) for m in policy.modules()),
           graph_enabled())
    return _step_of(agent).run(key, launch, batch_obs, shape, A, None)


def deterministic_act(agent, batch_obs, explore):
    """``ReplayActorCritic._batch_select_actions`` (``explore`` False: the policy's own actions) or
    the exploring branch of ``batch_act`` (True: the explorer's noise added and clipped): the
    actions [N, A] float32, or None.  The explorer's state and NumPy's stream move only when the
    step runs."""
    shape = _applicable(agent, batch_obs)
    if shape is None:
        return None
    policy = agent._policy()
    split = _split_of(agent, policy, _policy_split.deterministic_policy)
    if split is None:
        return None
    body, lin, bound_module = split
    N, A = len(batch_obs), lin.out_features
    if N > ops.ACTOR_ACT_MAX_M:
        return None
    ex = agent.explorer
    kind = explorer_kind(ex, A) if explore else GREEDY
    if kind is None:
        return None
    bound = None
    if bound_module is not None:
        bound = _bound_vectors(agent, bound_module, A)
        if bound is None:
            return None

    def launch(obs, noise, out):
        with torch.no_grad(), evaluating(policy):
            h = body(obs)
            if not hidden_ok(h, lin, N):
                return None
            if noise is None:
                return ops.deterministic_head_act(h, lin.weight, lin.bias, bound, out=out)[0]
            return ops.deterministic_head_act(h, lin.weight, lin.bias, bound, noise[:N], noise[N],
                                              noise[N + 1], out=out)[0]

    fill = None
    if kind == GAUSSIAN:
        def fill(rows):
            rows[N], rows[N + 1] = gaussian_bounds(ex, A)
            gaussian_noise(ex, rows[:N])
    elif kind == OU:
        def fill(rows):
            rows[N], rows[N + 1] = -np.inf, np.inf
            ou_noise(ex, rows[:N])
    key = (N, shape, bool(agent.training), kind, id(policy), tuple(id(m) for m in policy.modules()),
           id(bound_module), graph_enabled())
    return _step_of(agent).run(key, launch, batch_obs, shape, A, fill)
