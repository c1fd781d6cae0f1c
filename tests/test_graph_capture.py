"""pfrl_amd/agents/_capture.py: the one warm-up, snapshot and capture protocol of the agents.

CPU: the protocol has a single home (no other module of ``pfrl_amd.agents`` makes a graph, a stream
or touches the device generator's state) and the noise buffer's layout is the one both former
``_noise_buffers`` produced.  GPU: what a site relies on -- a restore that leaves no trace of the
warm-up, streams joined and switches put back on refusal and on error, one pool per holder, recorded
draws served exactly -- on ``Linear(4, 8) -> ReLU -> Linear(8, 2)`` at batch 3 with a capturable Adam.
"""
import copy
import gc
import importlib
import inspect
import pathlib
import pkgutil
import types

import numpy as np
import pytest
import torch
from torch import nn

import pfrl_amd
from pfrl_amd import agents, ops
from pfrl_amd.agents import _capture
from pfrl_amd.agents.graphed_update import _make_capturable

gpu = pytest.mark.gpu


# -------------------------------------------------------------------------------------------------
# CPU
# -------------------------------------------------------------------------------------------------
def test_the_protocol_has_a_single_home():
    sources = {m.name: inspect.getsource(importlib.import_module("pfrl_amd.agents." + m.name))
               for m in pkgutil.iter_modules(agents.__path__)}
    assert "_capture" in sources and "graphed_update" in sources and len(sources) > 20
    for needle in ("CUDAGraph(", "cuda.Stream(", "get_rng_state", "set_rng_state"):
        assert [name for name, src in sources.items() if needle in src] == ["_capture"], needle
    package = pathlib.Path(pfrl_amd.__file__).parent
    assert sum(p.read_text().count("def _align16") for p in package.rglob("*.py")) == 1


@pytest.mark.parametrize("repeat", [1, 3])
def test_noise_buffer_layout(repeat):
    sizes = [1, 3, 4, 5]
    # the parent commit's two formulas: GraphedUpdate's running offsets, CapturedStep's sum
    want_sizes = list(sizes) * repeat
    want_offs, pos = [], 0
    for n in want_sizes:
        want_offs.append(pos)
        pos += (n + 3) & ~3
    want_total = sum((n + 3) & ~3 for n in want_sizes)
    assert pos == want_total == 20 * repeat
    got_sizes, got_offs, got_total = _capture.noise_layout(sizes, repeat)
    assert got_sizes == want_sizes and got_offs == want_offs and got_total == want_total
    assert got_offs[:4] == [0, 4, 8, 12] and all(o % 4 == 0 for o in got_offs)


# -------------------------------------------------------------------------------------------------
# GPU
# -------------------------------------------------------------------------------------------------
def _setup(seed=0):
    dev = torch.device("cuda:0")
    torch.manual_seed(seed)
    model = nn.Sequential(nn.Linear(4, 8), nn.ReLU(), nn.Linear(8, 2))
    model.register_buffer("steps_seen", torch.zeros(1))
    model.to(dev)
    opt = torch.optim.Adam(model.parameters())
    assert _make_capturable(opt, dev)
    x = torch.randn(3, 4, device=dev)

    def step(i=None):
        torch.randn(5, device=dev)
        opt.zero_grad(set_to_none=True)
        model(x).pow(2).mean().backward()
        opt.step()
        with torch.no_grad():
            model.steps_seen.add_(1.0)

    return dev, model, opt, step, x


def _tensors(model):
    return [t.detach().clone() for t in list(model.parameters()) + list(model.buffers())]


def _state_tensors(opt):
    return [v for st in opt.state.values() for v in st.values() if torch.is_tensor(v)]


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


@gpu
@pytest.mark.parametrize("state_present", [False, True])
def test_snapshot_restores_parameters_buffers_state_and_generator(state_present):
    dev, model, opt, step, _ = _setup()
    if state_present:
        step()
    before = _tensors(model)
    state = [v.detach().clone() for v in _state_tensors(opt)]
    rng = torch.cuda.get_rng_state(dev).clone()
    snap = _capture.Snapshot([model], [opt], dev)
    step()
    step()
    assert not _same(_tensors(model), before) and not torch.equal(torch.cuda.get_rng_state(dev), rng)
    snap.restore()
    assert _same(_tensors(model), before)
    assert torch.equal(torch.cuda.get_rng_state(dev), rng)
    now = _state_tensors(opt)
    assert len(now) == 3 * 4                            # (step, exp_avg, exp_avg_sq per parameter)
    if state_present:
        assert _same(now, state)
    else:
        assert state == [] and all(not bool(v.any()) for v in now)


@gpu
def test_snapshot_of_the_generator_alone():
    dev = torch.device("cuda:0")
    rng = torch.cuda.get_rng_state(dev).clone()
    snap = _capture.Snapshot((), (), dev)
    torch.randn(5, device=dev)
    snap.restore()
    assert torch.equal(torch.cuda.get_rng_state(dev), rng)


@gpu
def test_warm_up_and_capture_leave_no_trace_and_the_replay_is_one_eager_step():
    dev, model, opt, step, x = _setup()
    # one eager step from the same start, on a copy
    twin = copy.deepcopy(model)
    twin_opt = torch.optim.Adam(twin.parameters())
    _make_capturable(twin_opt, dev)
    twin_opt.zero_grad(set_to_none=True)
    twin(x).pow(2).mean().backward()
    twin_opt.step()

    before = _tensors(model)
    rng = torch.cuda.get_rng_state(dev).clone()
    holder = types.SimpleNamespace(pool=None)
    passes = []
    snap = _capture.Snapshot([model], [opt], dev)
    try:
        assert _capture.warm_up(dev, lambda i: (passes.append(i), step())[1]) is True
        _make_capturable(opt, dev)
        opt.zero_grad(set_to_none=True)
        g, result = _capture.capture(holder, lambda: (step(), "result")[1])
    finally:
        snap.restore()
    assert passes == [0, 1] and result == "result"
    assert torch.equal(torch.cuda.get_rng_state(dev), rng)
    assert _same(_tensors(model), before)
    g.replay()
    torch.cuda.synchronize()
    assert _same(list(model.parameters()), list(twin.parameters()))
    assert float(model.steps_seen) == 1.0
    assert not torch.equal(torch.cuda.get_rng_state(dev), rng)   # (the replay's own draw)


@gpu
def test_a_refused_body_stops_the_warm_up_and_leaves_the_streams_joined():
    dev = torch.device("cuda:0")
    rng = torch.cuda.get_rng_state(dev).clone()
    passes = []

    def body(i):
        passes.append(i)
        torch.randn(5, device=dev)
        return _capture.REFUSED if i == 1 else None

    snap = _capture.Snapshot((), (), dev)
    try:
        assert _capture.warm_up(dev, body, passes=3) is False
    finally:
        snap.restore()
    assert passes == [0, 1]                                     # (no further pass, no graph)
    assert torch.equal(torch.cuda.get_rng_state(dev), rng)
    assert torch.cuda.current_stream(dev) == torch.cuda.default_stream(dev)
    y = torch.ones(4, device=dev) + 1
    torch.cuda.synchronize()
    assert y.tolist() == [2.0] * 4


@gpu
def test_an_error_in_the_warm_up_propagates_and_puts_every_switch_back():
    dev = torch.device("cuda:0")
    was_gc, was_profile = gc.isenabled(), ops._PROFILE_ON[0]

    def body(i):
        raise RuntimeError("refused by the test")       # (a plain raise, before any launch)

    with pytest.raises(RuntimeError, match="refused by the test"):
        _capture.warm_up(dev, body)
    assert gc.isenabled() == was_gc and ops._PROFILE_ON[0] == was_profile
    assert torch.cuda.current_stream(dev) == torch.cuda.default_stream(dev)
    y = torch.ones(4, device=dev) + 1
    torch.cuda.synchronize()
    assert y.tolist() == [2.0] * 4


@gpu
def test_the_first_graphs_pool_is_the_holders():
    dev = torch.device("cuda:0")
    buf = torch.zeros(8, device=dev)
    holder = types.SimpleNamespace(pool=None)
    _capture.warm_up(dev, lambda i: buf.add_(1.0))
    g1, _ = _capture.capture(holder, lambda: buf.add_(1.0))
    first = holder.pool
    assert first is not None and first == g1.pool()
    g2, _ = _capture.capture(holder, lambda: buf.mul_(2.0))
    assert holder.pool == first == g1.pool() == g2.pool()
    torch.cuda.synchronize()
    buf.zero_()
    g1.replay()
    g2.replay()
    torch.cuda.synchronize()
    assert buf.tolist() == [2.0] * 8


def _drawing_step(dev, updates, extra=0):
    """A step that draws 6 and 10 normals per update as the noisy layers do."""
    from pfrl_amd.nn import noisy_linear

    like = torch.zeros(1, device=dev)
    out = torch.zeros(updates, 16, device=dev)

    def step(i=None):
        out.zero_()
        for u in range(updates):
            out[u, :6].copy_(noisy_linear._draw(6, like))
            out[u, 6:].copy_(noisy_linear._draw(10, like))
        for _ in range(extra):
            noisy_linear._draw(6, like)

    return step, out


@gpu
@pytest.mark.parametrize("repeat", [1, 2])
def test_recorded_noise_is_laid_out_served_and_consumed_exactly(repeat):
    dev = torch.device("cuda:0")
    if ops.philox_variant(dev) is None:
        pytest.skip("pfrl_philox_normal does not reproduce torch.randn on this stack")
    assert _capture.noise_feed_available(dev)
    warm, _ = _drawing_step(dev, 1)                      # (warm-up: the first update only)
    step, out = _drawing_step(dev, repeat)
    holder = types.SimpleNamespace(pool=None)
    snap = _capture.Snapshot((), (), dev)
    try:
        noise = _capture.warm_up_noise(dev, warm, True, repeat)
        assert noise["sizes"] == [6, 10] * repeat
        assert [v.numel() for v in noise["views"]] == noise["sizes"]
        assert all(v.data_ptr() % 16 == 0 for v in noise["views"])
        assert noise["buf"].numel() == 20 * repeat and noise["plan"].views is noise["views"]
        with _capture.serving(noise) as feed:
            g, _ = _capture.capture(holder, step)
        assert feed.at == len(noise["views"]) == 2 * repeat
    finally:
        snap.restore()
    # a replay reads what the plan wrote: the normals torch.randn draws at this generator state
    snap = _capture.Snapshot((), (), dev)
    try:
        gen = torch.cuda.default_generators[0]
        gen.manual_seed(11)
        want = torch.cat([torch.randn(n, device=dev) for n in noise["sizes"]])
        end = gen.get_offset()
        gen.manual_seed(11)
        noise["plan"].run()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.reshape(-1), want) and gen.get_offset() == end
    finally:
        snap.restore()


@gpu
def test_a_capture_that_draws_more_than_was_recorded_is_stopped_by_the_feed():
    dev = torch.device("cuda:0")
    if ops.philox_variant(dev) is None:
        pytest.skip("pfrl_philox_normal does not reproduce torch.randn on this stack")
    warm, _ = _drawing_step(dev, 1)
    drawing, _ = _drawing_step(dev, 1, extra=1)
    inside = []

    def step():
        inside.append((gc.isenabled(), ops._PROFILE_ON[0]))
        drawing()

    holder = types.SimpleNamespace(pool=None)
    snap = _capture.Snapshot((), (), dev)
    was_gc = gc.isenabled()
    assert was_gc and not ops._PROFILE_ON[0]
    ops.profile_enable(True)                # (so that the pause inside ``capturing`` is a change)
    try:
        noise = _capture.warm_up_noise(dev, warm, True)
        with pytest.raises(AssertionError, match="noise feed exhausted"):
            _capture.capture(holder, step, _capture.serving(noise))
        # the error crossed ``capturing``: collector and profiler are what they were
        assert inside == [(False, False)]
        assert gc.isenabled() == was_gc and ops._PROFILE_ON[0] is True
    finally:
        ops.profile_enable(False)
        snap.restore()
    assert holder.pool is None
    assert not torch.cuda.is_current_stream_capturing()
    torch.cuda.synchronize()


@gpu
def test_warm_up_without_a_feed_records_nothing():
    dev = torch.device("cuda:0")
    warm, _ = _drawing_step(dev, 1)
    snap = _capture.Snapshot((), (), dev)
    try:
        assert _capture.warm_up_noise(dev, warm, False) is None
    finally:
        snap.restore()


@gpu
def test_actor_step_refusal_touches_nothing():
    from pfrl_amd.agents import _actor_device_step as ads

    dev = torch.device("cuda:0")
    step = ads.ActorStep(types.SimpleNamespace(device=dev))
    launches = []

    def launch(obs, noise, out):
        launches.append(tuple(obs.shape))
        torch.randn(5, device=dev)              # (a body that drew before it found out)
        return None

    captures = ads.captures
    rng = torch.cuda.get_rng_state(dev).clone()
    batch_obs = [np.zeros(4, dtype=np.float32) for _ in range(3)]
    assert step.run("key", launch, batch_obs, (4,), 2, None) is None
    assert launches == [(3, 4)]
    assert ads.captures == captures
    assert torch.equal(torch.cuda.get_rng_state(dev), rng)
    assert step.run("key", launch, batch_obs, (4,), 2, None) is None and len(launches) == 1
    torch.cuda.synchronize()
