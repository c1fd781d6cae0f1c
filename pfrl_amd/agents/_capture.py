"""The one protocol by which the agents capture a HIP graph: warm up on a side stream, put back what
the warm-up consumed, capture with the collector and the profiler paused, share one memory pool.

A site reads

    snap = Snapshot(modules, optimizers, device)        # (acting steps: the generator alone)
    try:
        if warm_up(device, lambda i: ...):              # False: the body refused (REFUSED)
            ...                                         # what must happen between the two
            graph, result = capture(self, lambda: ...)  # self.pool: the pool all its graphs share
    finally:
        snap.restore()

and, where the step's normals are to leave the graph (NoisyNet layers, ``Normal.rsample``),
``warm_up_noise`` in place of ``warm_up`` and ``with serving(noise):`` around the capture(s).
``distributed.captured_collectives_work`` keeps a capture of its own: it must be able to abandon a
probe that hangs."""
import contextlib
import gc
import os

import torch

from pfrl_amd import ops

REFUSED = object()      # what a warm-up body returns when the path does not apply to this model


def new_stream(device):
    """The only place the agents construct a stream -- the warm-up's side stream, and the long-lived
    ones of DQN's replay overlap and C51's forked passes -- so that a search for stream creation
    in ``pfrl_amd/agents/`` ends here and a hand-written warm-up elsewhere stands out."""
    return torch.cuda.Stream(device)


def _capture_kwargs(pool):
    """Arguments of ``torch.cuda.graph``: the shared memory pool, and thread-local capture error
    mode -- in the default global mode a HIP call from ANY other thread while this one captures
    (a process group's watchdog polling events, a runtime helper thread) aborts the process."""
    kw = {} if pool is None else {"pool": pool}
    kw["capture_error_mode"] = "thread_local"
    return kw


@contextlib.contextmanager
def capturing(g, pool):
    """``with capturing(g, pool):`` -- ``torch.cuda.graph`` with the collector paused.  A
    collection that starts mid-capture runs finalizers on the capturing thread (graphs, pinned
    buffers and events of an agent that went out of scope): their HIP calls are not allowed in a
    capture, the error is thrown inside a destructor and the process aborts -- seen as a rare
    "Fatal Python error: Aborted ... Garbage-collecting" when several agents are built in one
    process.  ``torch.cuda.graph`` collects once on entry, before the capture begins.

    The fused-gather profiler is paused too (``ops.profile_paused``: an event pair created inside
    a capture would belong to the capture, and a replay never signals it)."""
    was_enabled = gc.isenabled()
    try:
        with ops.profile_paused(), torch.cuda.graph(g, **_capture_kwargs(pool)):
            gc.disable()
            yield
    finally:
        if was_enabled:
            gc.enable()


def capture(holder, fn, *contexts):
    """``fn()`` recorded into a new graph inside ``capturing`` and the caller's ``contexts``:
    (graph, what ``fn`` returned).  ``holder.pool`` is the pool of all graphs of one holder: the
    first graph's, adopted here."""
    g = torch.cuda.CUDAGraph()
    with contextlib.ExitStack() as stack:
        stack.enter_context(capturing(g, holder.pool))
        for ctx in contexts:
            stack.enter_context(ctx)
        result = fn()
    if holder.pool is None:
        holder.pool = g.pool()
    return g, result


def warm_up(device, fn, passes=2):
    """The iterations PyTorch needs before a capture: ``fn(i)`` for i < ``passes`` on a side stream
    that waits for the current one and is joined again whatever happens.  False when ``fn``
    returned ``REFUSED`` (no further pass is made), else True."""
    try:
        torch.autograd.graph.set_warn_on_accumulate_grad_stream_mismatch(False)
    except AttributeError:
        pass
    cur = torch.cuda.current_stream(device)
    side = new_stream(device)
    side.wait_stream(cur)
    try:
        with torch.cuda.stream(side):
            for i in range(passes):
                if fn(i) is REFUSED:
                    return False
    finally:
        cur.wait_stream(side)
    return True


def _optimizer_tensors(optimizer):
    out = []
    for st in optimizer.state.values():
        for k, v in st.items():
            if isinstance(v, torch.Tensor):
                out.append((st, k, v))
    return out


class Snapshot:
    """Parameters and buffers of ``modules``, every tensor of the ``optimizers``' state and the
    device generator as they are now; ``restore()`` undoes the warm-up steps (also when the capture
    itself fails), so that no extra optimizer step and no draw leaks into training."""

    def __init__(self, modules, optimizers, device):
        self.modules, self.optimizers, self.device = list(modules), list(optimizers), device
        self.saved = [t.detach().clone() for t in self._tensors()]
        self.had_state = [len(o.state) > 0 for o in self.optimizers]
        self.opt_saved = [[(st, k, v.detach().clone()) for st, k, v in _optimizer_tensors(o)]
                          for o in self.optimizers]
        self.rng = torch.cuda.get_rng_state(device)

    def _tensors(self):
        out = []
        for m in self.modules:
            out.extend(m.parameters())
            out.extend(m.buffers())
        return out

    def restore(self):
        with torch.no_grad():
            for t, s in zip(self._tensors(), self.saved):
                t.copy_(s)
            for o, had, saved in zip(self.optimizers, self.had_state, self.opt_saved):
                if had:
                    for st, k, v in saved:
                        st[k].copy_(v)
                else:
                    # state was created by the warm-up: reset it to its initial value
                    for st, k, v in _optimizer_tensors(o):
                        v.zero_()
        torch.cuda.set_rng_state(self.rng, self.device)


# -- the normals of a step as ONE launch in front of its graph ------------------------------------
def noise_feed_available(device):
    """csrc/philox.hip reproduces this PyTorch build's torch.randn bit for bit (probed) on a GPU:
    the draws can then leave the captured graph -- one eager launch per replay writes all of them,
    in call order, from the device generator (PFRL_NOISE_FEED=0: torch.randn inside the graph)."""
    if os.environ.get("PFRL_NOISE_FEED", "1") == "0" or torch.device(device).type != "cuda":
        return False
    return ops.philox_variant(device) is not None


def noise_layout(sizes, repeat=1):
    """(sizes x repeat, offset of each draw, length) of the buffer all draws of a replay live in:
    back to back, each rounded up to 4 floats (16-byte aligned views)."""
    sizes = list(sizes) * repeat
    offsets, pos = [], 0
    for n in sizes:
        offsets.append(pos)
        pos += (n + 3) & ~3
    return sizes, offsets, pos


def noise_buffers(sizes, repeat, device):
    sizes, offsets, total = noise_layout(sizes, repeat)
    buf = torch.zeros(total, dtype=torch.float32, device=device)
    plan = ops.RandnPlan(sizes, device, out=buf)        # (argument arrays built once)
    assert [v.storage_offset() for v in plan.views] == offsets
    return {"sizes": sizes, "buf": buf, "views": plan.views, "plan": plan}


def warm_up_noise(device, fn, feed_ok, repeat=1):
    """``warm_up`` for a step whose draws go through ``noisy_linear.noise_feed``.  With ``feed_ok``
    pass 0 draws through torch.randn as usual and notes the sizes; if there were any, the later
    passes (and, under ``serving``, the capture) read views of one static buffer -- ``repeat``
    copies of the recorded sizes, filled once here for the rest of the warm-up (the generator is
    the caller's to restore either way).  Returns the noise dict a replay runs the plan of
    (sizes, buf, views, plan), or None."""
    from pfrl_amd.nn.noisy_linear import NoiseFeed, noise_feed

    rec = NoiseFeed() if feed_ok else None
    noise = None

    def one(i):
        nonlocal noise
        if i == 1 and rec is not None and rec.sizes:
            noise = noise_buffers(rec.sizes, repeat, device)
            noise["plan"].run()
        with noise_feed(rec if i == 0 else (NoiseFeed(noise["views"]) if noise else None)):
            return fn(i)

    warm_up(device, one)
    return noise


@contextlib.contextmanager
def serving(noise):
    """The capture(s) inside are served ``noise``'s views (None: they draw for themselves) and
    must have consumed exactly all of them -- a step that draws more is stopped by the feed, one
    that draws less would replay with normals nobody reads.  Yields the feed."""
    from pfrl_amd.nn.noisy_linear import NoiseFeed, noise_feed

    feed = NoiseFeed(noise["views"]) if noise else None
    with noise_feed(feed):
        yield feed
    assert feed is None or feed.at == len(feed.views), \
        "the captured step drew %d normals' tensors, %d were recorded" % (feed.at, len(feed.views))
