"""The batched DQN step with NO host round trip (device env + uniform one-step device replay).

``DQN.batch_act`` / ``DQN._batch_observe_train`` (reference pfrl/agents/dqn.py:490-549) spend
their time on the host: a per-env epsilon-greedy loop that has to wait for the greedy actions
(``.cpu().numpy()``, :497), a per-env append loop and one ``sample_n_k`` per update.  None of it
needs the GPU's results:

* the epsilon-greedy draws do not depend on the network -- the native planner
  (``pfrl_amd.host_plan``, csrc/hostplan.hip) makes them on NumPy's global stream, the GPU
  resolves ``action = draw fired ? random action : argmax Q`` (``pfrl_select_actions``) and
  the actions stay in HBM as :class:`DeviceActions`;
* the appends of an env range, the queue bookkeeping and every index set the reference's loop
  would draw between them come from ONE planner call, written into ONE pinned block that
  crosses PCIe in one transfer; the transition rows take their action column from the device
  tensor.

So the host never blocks on the device inside a step: it runs ahead (bounded by ``RUN_AHEAD``
steps) and the GPU queue stays full.  Order of appends, NumPy draws, target syncs and updates is
the reference's (tests/test_host_plan.py: stream position after every call;
tests/test_bench_path_parity.py, tests/test_agent_parity.py: whole traces).

A second explorer kind takes the same step: ``explorers.Boltzmann`` (reference
pfrl/explorers/boltzmann.py:18-26).  Its ``np.random.choice(arange(A), p=probs)`` consumes exactly
one ``random_sample()`` per env whatever the probabilities are, so the host draws the N uniforms
up front (``np.random.random_sample(N)``: the same stream positions), the staging slot carries
``refs | u (f64, 16-byte aligned) | T (f32)`` and softmax, cdf and search run behind the Q head
(``pfrl_dqn_act_head_boltzmann``; ``pfrl_boltzmann_select`` for heads the split does not take).
``choice`` raises ``ValueError("probabilities contain NaN")`` on the spot; here the launch raises
a status word that is copied into pinned memory behind it and looked at when that step's event is
waited for in the run-ahead loop -- the same ``ValueError``, at most ``RUN_AHEAD`` steps late, at
the latest on ``stop_episode``, ``save`` and ``get_statistics`` (:func:`check_pending`).

Everything here is a fast path with the general code behind it: any condition that does not
hold (another explorer, a host env, prioritized or n-step replay, recurrent model, the dense
``sample_n_k`` regime of a tiny buffer) falls back to ``DQN``'s own methods.
"""
import collections
import ctypes
import logging
import os

import numpy as np
import torch

from pfrl_amd import _native, host_plan, ops
from pfrl_amd.agents import _capture
from pfrl_amd.agents._policy_split import hidden_ok, prefix_view
from pfrl_amd.device_store import DeviceActions, DeviceObsBatch
from pfrl_amd.staging import StagingRing, _align16
from pfrl_amd.utils.contexts import evaluating

RUN_AHEAD = 3       # batched steps the host may be ahead of the GPU


class LastBatch:
    """``agent.batch_last_obs`` / ``batch_last_action`` over a device batch: indexable like the
    lists the reference keeps (pfrl/agents/dqn.py:503-505), entries can be set to None, nothing
    is materialised unless somebody looks."""

    def __init__(self, batch):
        self.batch = batch
        self.cleared = None

    def __len__(self):
        return len(self.batch)

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(len(self)))]
        if self.cleared is not None and self.cleared[i]:
            return None
        return self.batch[i]

    def __setitem__(self, i, value):
        assert value is None
        if self.cleared is None:
            self.cleared = np.zeros(len(self), dtype=bool)
        self.cleared[i] = True

    def __iter__(self):
        return (self[i] for i in range(len(self)))

    def all_set(self, lo, hi):
        return self.cleared is None or not self.cleared[lo:hi].any()


def act_split(agent):
    """(body, head layer) when the model is ``Sequential(..., Linear(K, A <= 16),
    DiscreteActionValueHead())`` -- the example Q-network (examples/atari/train_dqn_batch_ale.py:35-41):
    its narrow head, the argmax and the epsilon-greedy decision then run as ONE launch
    (pfrl_dqn_act_head) instead of head + torch argmax + cast + select.  ``body`` is a view of the model
    without its last two children (same class, children and parameters: a fused trunk stays fused)."""
    model = agent.model
    hit = agent.__dict__.get("_act_split_cache")
    if hit is not None and hit[0] is model and hit[2] == tuple(id(m) for m in model.children()):
        return hit[1]
    from pfrl_amd.q_functions import DiscreteActionValueHead

    out = None
    nn = torch.nn
    if (os.environ.get("PFRL_DQN_ACT_HEAD", "1") != "0" and isinstance(model, nn.Sequential)
            and len(model) >= 3 and type(model[len(model) - 1]) is DiscreteActionValueHead):
        lin = model[len(model) - 2]
        if (isinstance(lin, nn.Linear) and 1 <= lin.out_features <= 16
                and lin.weight.dtype == torch.float32 and lin.weight.is_contiguous()):
            out = (prefix_view(model, drop=2), lin)
    agent._act_split_cache = (model, out, tuple(id(m) for m in model.children()))
    return out


EPS_GREEDY, BOLTZMANN = "eps_greedy", "boltzmann"      # the explorer kinds of the device step
MAX_BOLTZMANN_ACTIONS = 64                             # (kMaxBoltzmannA of csrc/boltzmann_row.h)


def boltzmann_temperature(ex):
    """``ex.T`` as the float32 the kernels divide by when ``ex`` is exactly ``explorers.Boltzmann``
    with its own ``select_action`` and a positive finite temperature (also as float32); else None."""
    from pfrl_amd.explorers.boltzmann import Boltzmann

    if type(ex) is not Boltzmann or "select_action" in vars(ex):
        return None
    T = ex.T
    if isinstance(T, bool) or not isinstance(T, (int, float, np.integer, np.floating)):
        return None
    with np.errstate(over="ignore"):
        T = np.float32(T)
    return T if np.isfinite(T) and T > 0 else None


def act_kind(agent, batch_obs):
    """The explorer kind under which :func:`act` takes this step, or None (the general code of
    ``DQN.batch_act`` runs): training mode, a DeviceObsBatch, a non-recurrent model on CUDA and
    either the epsilon-greedy family or plain Boltzmann."""
    if not (agent.training and isinstance(batch_obs, DeviceObsBatch) and not agent.recurrent
            and agent.device.type == "cuda"):
        return None
    if agent._explorer_draws_before_greedy():
        return EPS_GREEDY
    return BOLTZMANN if boltzmann_temperature(agent.explorer) is not None else None


def boltzmann_action_values(av):
    """The [N, A] float32 action values the Boltzmann kernels read, or None: a
    ``DiscreteActionValue`` (what ``Boltzmann.select_action`` asserts) with 1 <= A <= 64."""
    from pfrl_amd.action_value import DiscreteActionValue

    if not isinstance(av, DiscreteActionValue):
        return None
    q = av.q_values
    if not (torch.is_tensor(q) and q.dim() == 2 and q.dtype == torch.float32
            and 1 <= q.shape[1] <= MAX_BOLTZMANN_ACTIONS):
        return None
    return q.detach().contiguous()


def _boltzmann_model_ok(agent, batch_obs):
    """Whether the model's output is one the Boltzmann launches take -- known before the host
    draws, because a step that falls back must leave NumPy's stream to the general code.  A
    recognised head (act_split) is; any other model is evaluated ONCE on the first batch, with
    torch's generators restored behind it (NoisyNet layers draw), and the answer kept per model."""
    if act_split(agent) is not None:
        return True
    model = agent.model
    key = tuple(id(m) for m in model.modules())
    hit = agent.__dict__.get("_boltzmann_model_cache")
    if hit is not None and hit[0] is model and hit[1] == key:
        return hit[2]
    with torch.random.fork_rng(devices=[agent.device]), torch.no_grad(), evaluating(model):
        ok = boltzmann_action_values(agent._evaluate_model(batch_obs)) is not None
    batch_obs._refs_dev = None
    agent._boltzmann_model_cache = (model, key, ok)
    return ok


def _wait_step(agent, step):
    """Waits for a step's event; raises what ``np.random.choice`` raises in the reference when
    that step's status word (Boltzmann steps only) came back set.  The device word is sticky (the
    kernels only OR into it): it is cleared here, so that the error is reported once."""
    ev, status = step
    ev.synchronize()
    if status is not None and int(status[0]) != 0:
        status.zero_()
        agent._act_status.zero_()
        raise ValueError("probabilities contain NaN")


def check_pending(agent):
    """Looks at the status word of every Boltzmann step still in flight (module docstring)."""
    evs = agent.__dict__.get("_step_events")
    pending = [step for step in evs or () if step[1] is not None]
    if pending:
        rest = [step for step in evs if step[1] is None]
        evs.clear()
        evs.extend(rest)
        for step in pending:
            _wait_step(agent, step)


class ActGraph:
    """The device side of ``DQN.batch_act`` on the device-step path -- observation gather, trunk,
    Q head + argmax + epsilon-greedy decision, or Q head + Boltzmann draw -- as ONE captured HIP
    graph per batch shape and explorer kind, fed by
    the step's single staging transfer (frame slots + the host's draws) landing in the graph's own
    input block (reference pfrl/agents/dqn.py:490-507).  Two instances alternate, so the actions
    of a step stay valid while the next step's are computed.  The graph reads the frame ring and
    the parameters in place: optimizer steps, target syncs and new frames need no re-capture."""

    def __init__(self, agent):
        self.agent = agent
        self.entries = {}
        self.pool = None

    @staticmethod
    def applicable(agent):
        return (os.environ.get("PFRL_DQN_ACT_GRAPH", "1") != "0" and agent.use_graphs
                and act_split(agent) is not None)

    def _body(self, agent, batch_obs, inp, N, k, off_choice, out, kind):
        refs_bytes = 4 * N * k
        batch_obs._refs_dev = inp[:refs_bytes].view(torch.int32).view(N, k)
        if kind == BOLTZMANN:
            return _act_launches_boltzmann(agent, batch_obs, *_boltzmann_draws(inp, N, off_choice), out)
        choice = inp[off_choice:off_choice + 4 * N].view(torch.int32)
        return _act_launches(agent, batch_obs, choice, out)

    def _capture(self, agent, batch_obs, N, k, off_choice, need, kind):
        dev = agent.device
        pair = []
        for _ in range(2):
            inp = torch.zeros(_align16(need), dtype=torch.uint8, device=dev)
            inp[:4 * N * k].view(torch.int32).copy_(
                torch.from_numpy(np.ascontiguousarray(batch_obs.refs.reshape(-1))).to(dev))
            if kind == BOLTZMANN:
                _boltzmann_draws(inp, N, off_choice)[1].fill_(1.0)    # (u = 0 at T = 1 until a step lands)
            else:
                inp[off_choice:off_choice + 4 * N].view(torch.int32).fill_(-1)
            out = torch.empty(N, dtype=torch.int64, device=dev)

            def body(i=None, inp=inp, out=out):
                if self._body(agent, batch_obs, inp, N, k, off_choice, out, kind) is None:
                    return _capture.REFUSED

            snap = _capture.Snapshot((), (), dev)       # (the generator: warm-up draws are not part of the run)
            try:
                if not _capture.warm_up(dev, body):
                    return None
            finally:
                snap.restore()
            pair.append((_capture.capture(self, body)[0], inp, out))
        return [pair, 0]

    def run(self, agent, batch_obs, ring, tok, N, k, off_choice, need, kind=EPS_GREEDY):
        """Ships pinned slot ``tok`` into the graph's input block and replays; returns the
        actions (int64 [N], owned by the graph instance) or None when the model cannot take the
        fused head (the caller then commits the slot to the ring and launches eagerly).  The
        explorer kind is part of the key: another explorer on a live agent is another graph."""
        model = agent.model
        fr = batch_obs.store
        key = (N, k, id(model), tuple(id(m) for m in model.modules()), id(fr),
               getattr(fr, "emit_channels_last", None), id(agent.phi), kind)
        e = self.entries.get(key)
        if e is None:
            if len(self.entries) > 8:
                self.entries.clear()
            e = self.entries[key] = self._capture(agent, batch_obs, N, k, off_choice, need, kind) or False
        if e is False:
            return None
        pair, at = e
        e[1] = at ^ 1
        g, inp, out = pair[at]
        ring.commit_to(tok, need, inp)
        batch_obs._refs_dev = inp[:4 * N * k].view(torch.int32).view(N, k)
        g.replay()
        return out


def _act_launches(agent, batch_obs, choice, out=None):
    """gather -> trunk -> fused head: the actions (int64 [N]), or None when the hidden activations
    are not what pfrl_dqn_act_head reads."""
    split = act_split(agent)
    with torch.no_grad(), evaluating(agent.model):
        if split is None:
            greedy = agent._evaluate_model(batch_obs).greedy_actions.detach()
            return ops.select_actions(greedy, choice, out=out)
        body, lin = split
        agent._route_observation_layout(batch_obs)
        h = body(agent.batch_states(batch_obs, agent.device, agent.phi))
        if not hidden_ok(h, lin):
            if out is not None:
                return None
            greedy = list(agent.model._modules.values())[-1](lin(h)).greedy_actions.detach()
            return ops.select_actions(greedy, choice)
        return ops.dqn_act_head(h, lin.weight, lin.bias, choice, out=out)[0]


def _boltzmann_draws(block, N, off):
    """(u f64 [N], T f32 [1]) of a staging block, host array or device tensor alike."""
    f64, f32 = (np.float64, np.float32) if isinstance(block, np.ndarray) else (torch.float64, torch.float32)
    return block[off:off + 8 * N].view(f64), block[off + 8 * N:off + 8 * N + 4].view(f32)


def _act_launches_boltzmann(agent, batch_obs, u, temperature, out=None):
    """gather -> trunk -> fused head with the Boltzmann draw behind it, or model -> q_values ->
    pfrl_boltzmann_select for a head the split does not take: the actions (int64 [N]), or None
    when a capture (``out``) meets hidden activations pfrl_dqn_act_head_boltzmann does not read."""
    split = act_split(agent)
    status = agent._act_status
    with torch.no_grad(), evaluating(agent.model):
        if split is None:
            av = agent._evaluate_model(batch_obs)
        else:
            body, lin = split
            agent._route_observation_layout(batch_obs)
            h = body(agent.batch_states(batch_obs, agent.device, agent.phi))
            if hidden_ok(h, lin):
                return ops.dqn_act_head_boltzmann(h, lin.weight, lin.bias, u, temperature, status,
                                                  out=out)[0]
            if out is not None:
                return None
            av = list(agent.model._modules.values())[-1](lin(h))
        q = boltzmann_action_values(av)
        if q is None:
            raise RuntimeError("pfrl_amd: the model's action values changed kind under Boltzmann "
                               "exploration on the device step")
        return ops.boltzmann_select(q, u, temperature, status, out=out)[0]


def act(agent, batch_obs):
    """``DQN.batch_act`` in training mode for a DeviceObsBatch; None = conditions not met.  A
    Boltzmann step whose probabilities hold a NaN raises the reference's ``ValueError`` up to
    ``RUN_AHEAD`` steps late (module docstring)."""
    kind = act_kind(agent, batch_obs)
    if kind is None:
        return None
    ex = agent.explorer
    N, k = batch_obs.refs.shape
    refs_bytes = 4 * N * k
    off_choice = _align16(refs_bytes)
    if kind == EPS_GREEDY:
        n_act = host_plan.recognise_randint(ex.random_action_func)
        if n_act is None or ex.logger.isEnabledFor(logging.DEBUG):
            return None
        need = off_choice + 4 * N
    else:
        if not _boltzmann_model_ok(agent, batch_obs):
            return None
        need = off_choice + 8 * N + 4           # refs | u (f64, 16-byte aligned) | T (f32)
        if "_act_status" not in agent.__dict__:
            agent._act_status = torch.zeros(1, dtype=torch.int32, device=agent.device)
            agent._act_status_host = torch.zeros(2 * RUN_AHEAD, dtype=torch.int32).pin_memory()
            agent._act_status_at = 0
    ring = agent.__dict__.get("_act_ring")
    if ring is None or ring.slot_bytes < need:
        check_pending(agent)
        ring = agent._act_ring = StagingRing(agent.device, slot_bytes=max(1 << 14, need + 64),
                                             n_slots=2 * RUN_AHEAD + 2)
        agent._step_events = collections.deque()
    # bounded run-ahead: wait for the step RUN_AHEAD steps back
    evs = agent._step_events
    while len(evs) >= RUN_AHEAD:
        _wait_step(agent, evs.popleft())
    host, tok = ring.reserve()
    host[:refs_bytes].view(np.int32)[:] = batch_obs.refs.reshape(-1)
    if kind == EPS_GREEDY:
        choice = host[off_choice:need].view(np.int32)
        ex.epsilon = eps = ex.compute_epsilon(agent.t)
        host_plan.eps_greedy(N, eps, n_act, out=choice)
    else:
        u, temperature = _boltzmann_draws(host, N, off_choice)
        u[:] = np.random.random_sample(N)       # env order: the positions of N scalar choice() calls
        temperature[0] = boltzmann_temperature(ex)
    actions = None
    if ActGraph.applicable(agent):
        graph = agent.__dict__.get("_act_graph")
        if graph is None:
            graph = agent._act_graph = ActGraph(agent)
        actions = graph.run(agent, batch_obs, ring, tok, N, k, off_choice, need, kind)
    if actions is None:
        dev = ring.commit(tok, need)
        batch_obs._refs_dev = dev[:refs_bytes].view(torch.int32).view(N, k)
        if kind == EPS_GREEDY:
            actions = _act_launches(agent, batch_obs, dev[off_choice:need].view(torch.int32))
        else:
            actions = _act_launches_boltzmann(agent, batch_obs, *_boltzmann_draws(dev, N, off_choice))
    status = None
    if kind == BOLTZMANN:
        at = agent._act_status_at
        agent._act_status_at = (at + 1) % (2 * RUN_AHEAD)
        status = agent._act_status_host[at:at + 1]
        status.copy_(agent._act_status, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record()
    evs.append((ev, status))
    agent._last_obs_batch = batch_obs
    agent._last_actions_dev = actions
    agent.batch_last_obs = LastBatch(batch_obs)
    agent.batch_last_action = LastBatch(DeviceActions(actions))
    return agent.batch_last_action.batch


def begin_observe(agent, batch_obs, batch_reward, batch_done, batch_reset):
    """Per-step preparation of the native append path: contiguous reward / done columns."""
    agent._obs_cols = None
    acts = agent.__dict__.get("_last_actions_dev")
    prev = agent.__dict__.get("_last_obs_batch")
    rbuf = agent.replay_buffer
    if not (acts is not None and isinstance(batch_obs, DeviceObsBatch)
            and isinstance(prev, DeviceObsBatch) and prev.store is batch_obs.store
            and len(prev) == len(batch_obs) == acts.shape[0]
            and isinstance(agent.batch_last_obs, LastBatch)
            and agent.batch_last_obs.batch is prev
            and not agent.recurrent and rbuf.batch_append_supported(batch_obs)):
        return
    agent._obs_cols = (np.ascontiguousarray(batch_reward, dtype=np.float64),
                       np.ascontiguousarray(batch_done, dtype=np.uint8),
                       np.logical_or(np.asarray(batch_done, dtype=bool),
                                     np.asarray(batch_reset, dtype=bool)))


def plan_range(agent, lo, hi, batch_obs):
    """Appends + index draws of envs [lo, hi) through the native planner.  Returns
    (plan_env, slots_dev, U) -- the env after whose append each update runs, the sampled entry
    slots on the device, the number of updates -- or None when the Python path has to run."""
    cols = agent.__dict__.get("_obs_cols")
    if cols is None or not agent.batch_last_obs.all_set(lo, hi):
        return None
    rbuf, up = agent.replay_buffer, agent.replay_updater
    st = rbuf.store
    planner = agent.__dict__.get("_planner")
    if planner is None or not planner.valid_for(rbuf):
        planner = agent._planner = host_plan.DQNRangePlanner(rbuf)
    prev = agent._last_obs_batch
    N = len(prev)
    B = up.batchsize
    m = hi - lo
    need = planner.block_bytes(N, (N // up.update_interval + 1) * up.n_times_update, B)
    ring = agent.__dict__.get("_obs_ring")
    if ring is None or ring.slot_bytes < need:
        ring = agent._obs_ring = StagingRing(agent.device, slot_bytes=max(1 << 16, need),
                                             n_slots=4 * RUN_AHEAD + 4)
    st.flush()                  # rows the Python path may have left pending go first
    reward, done, ended = cols
    host, tok = ring.reserve()
    t0 = agent.t
    U = planner.plan(prev.refs[lo:hi], prev.min_seq[lo:hi], batch_obs.refs[lo:hi],
                     batch_obs.min_seq[lo:hi], reward[lo:hi], done[lo:hi], t0,
                     up.replay_start_size, up.update_interval, up.n_times_update, B, host)
    if U == host_plan.PLAN_DENSE:
        return None
    o = planner.offs
    dev = ring.commit(tok, int(o[9]))
    base = dev.data_ptr()
    lib = _native.lib()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    V = ctypes.c_void_p
    a_ptr = agent._last_actions_dev.data_ptr() + 8 * lo
    _native.check(lib.pfrl_table_append(ctypes.byref(st.desc), m, V(base + int(o[0])),
                                        V(base + int(o[1])), V(base + int(o[2])), V(a_ptr),
                                        V(base + int(o[3])), V(base + int(o[4])), stream),
                  "table_append")
    _native.check(lib.pfrl_entries_append(ctypes.byref(st.desc), m, V(base + int(o[5])),
                                          V(base + int(o[6])), V(base + int(o[7])), stream),
                  "entries_append")
    st.h_action_stale = True     # the action column exists on the device only
    if ended[lo:hi].any():
        for i in np.flatnonzero(ended[lo:hi]):
            agent.batch_last_obs[lo + int(i)] = None
            agent.batch_last_action[lo + int(i)] = None
    if U == 0:
        return [], None, 0
    ui = up.update_interval
    first = (-(t0 + 1)) % ui          # offset of the first env whose t is a multiple of ui
    # (updates only start once len >= replay_start_size: the LAST U // n_times due envs)
    due = [lo + j for j in range(first, m, ui)]
    due = due[len(due) - U // up.n_times_update:]
    plan_env = [i for i in due for _ in range(up.n_times_update)]
    slots_dev = dev[int(o[8]):int(o[8]) + 4 * U * B].view(torch.int32)
    return plan_env, slots_dev, U
