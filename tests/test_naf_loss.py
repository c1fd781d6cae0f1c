"""``pfrl_naf_td_loss`` (csrc/naf.hip) through the C ABI: every output lies between two guard zones
that must be untouched after the launch, and the payload must be fully written.

Shapes.  B in {1, 2, 3, 4, 5, 32, 63, 64, 65, 257} and, because one workgroup of W waves walks the
rows (wave w: rows w, w + W, ...) with W = 16 (n <= 4), 8 (n <= 16) or 4 (n <= 32), the edges of that
mapping: B in {7, 8, 9, 15, 16, 17} (one row short of, exactly, one row past a full sweep), all with
n in {1, 2, 3, 6, 17, 31, 32}; the last n of each unroll bucket and the first of the next (4, 5, 8,
9, 16) at B in {5, 32, 65}.  The six flags (scale_mu, bounds, Double, clip_delta, mean, weights) by
a pairwise covering set of rows (``FLAG_ROWS``, checked below), every row with every shape.

What is exact: refusals write nothing; a second launch and three replays of a captured graph give the
first launch's bits; with no Double, bounds on and scale_mu on the target value is v' itself.

What is rounded, and the rule (the project's, from tests/test_boltzmann_head.py): the reference
expression -- scale_by_tanh, exp, lower_triangular_matrix, L L^T, QuadraticActionValue,
compute_value_loss / compute_weighted_value_loss, gradients by autograd -- is evaluated in float64 on
the same float32 inputs.  The yardstick is the same expression in float32 in stock torch on the CPU,
measured against that float64 value; the launch may err at most twice as much (|L^T d|^2 and
d^T (L L^T) d round differently and neither is privileged).  Maxima of the absolute error are taken
per flag row over all shapes, per quantity (``RATIO`` lines with ``pytest -s``)."""
import ctypes
import itertools

import pytest
import torch

from pfrl_amd import _native

pytestmark = pytest.mark.gpu

GUARD = 1024
PFRL_ERR_ARG = -2
BATCHES, EDGE_BATCHES = (1, 2, 3, 4, 5, 32, 63, 64, 65, 257), (7, 8, 9, 15, 16, 17)
DIMS, EDGE_DIMS = (1, 2, 3, 6, 17, 31, 32), (4, 5, 8, 9, 16)
# every B with every n of the two main lists; the bucket-edge n at three batch sizes
SHAPES = ([(B, n) for n in DIMS for B in BATCHES + EDGE_BATCHES]
          + [(B, n) for n in EDGE_DIMS for B in (5, 32, 65)])
FLAGS = ("scale_mu", "bounds", "double", "clip_delta", "mean", "weights")
# a pairwise covering array of six binary factors
FLAG_ROWS = ((0, 0, 0, 0, 0, 0), (1, 1, 1, 1, 1, 1), (1, 1, 0, 1, 0, 0), (1, 0, 1, 0, 1, 0),
             (0, 1, 1, 0, 0, 1), (0, 0, 0, 1, 1, 1), (1, 0, 0, 0, 0, 1), (0, 1, 0, 0, 1, 0),
             (0, 0, 1, 1, 0, 0))
QUANTITIES = ("loss", "y", "dv", "dm", "de", "dc")


def test_the_flag_rows_cover_every_pair():
    for i, j in itertools.combinations(range(len(FLAGS)), 2):
        assert {(r[i], r[j]) for r in FLAG_ROWS} == {(0, 0), (0, 1), (1, 0), (1, 1)}, (i, j)


def _dev():
    return torch.device("cuda:0")


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class _Guarded:
    """n float32 elements between two guard zones of NaNs, which no launch writes."""

    def __init__(self, n):
        self.n = n
        self.full = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32, device=_dev())
        self.t = self.full[GUARD:GUARD + n]

    def done(self, what):
        assert bool(torch.isnan(self.full[:GUARD]).all()), "guard zone before %s was written" % what
        assert bool(torch.isnan(self.full[GUARD + self.n:]).all()), "guard zone after %s was written" % what
        assert not bool(torch.isnan(self.t).any()), "%s: payload not fully written" % what
        return self.t.cpu()

    def untouched(self, what):
        assert bool(torch.isnan(self.full).all()), "%s was written" % what


def make_inputs(B, n, flags, seed):
    """float32 inputs on the CPU in the issue's ranges: e in [-1.5, 1.5], c and m in [-2, 2], actions
    inside and outside the box."""
    f = dict(zip(FLAGS, flags))
    g = torch.Generator().manual_seed(seed)
    u = lambda lo, hi, *shape: torch.rand(*shape, generator=g) * (hi - lo) + lo  # noqa: E731
    nc = n * (n - 1) // 2
    low, high = torch.linspace(-1.0, -0.5, n), torch.linspace(0.5, 1.0, n)
    x = dict(v=u(-1, 1, B), m=u(-2, 2, B, n), e=u(-1.5, 1.5, B, n), c=u(-2, 2, B, nc) if n > 1 else None,
             tv=u(-1, 1, B), tm=u(-2, 2, B, n), te=u(-1.5, 1.5, B, n),
             tc=u(-2, 2, B, nc) if n > 1 else None,
             m2=u(-2, 2, B, n) if f["double"] else None, action=u(-1.5, 1.5, B, n),
             reward=u(-1, 1, B), discount=u(0.9, 0.99, B), terminal=(u(0, 1, B) < 0.25).float(),
             weights=u(0.5, 1.5, B) if f["weights"] else None,
             half_width=(high - low) / 2 if f["scale_mu"] else None,
             centre=(high + low) / 2 if f["scale_mu"] else None,
             low=low if f["bounds"] else None, high=high if f["bounds"] else None)
    return x, f


ORDER = ("v", "m", "e", "c", "tv", "tm", "te", "tc", "m2", "action", "reward", "discount", "terminal",
         "weights", "half_width", "centre", "low", "high")


def launch(x, f, B, n, outs=None):
    xd = {k: (None if t is None else t.to(_dev()).contiguous()) for k, t in x.items()}
    nc = n * (n - 1) // 2
    if outs is None:
        outs = dict(loss=_Guarded(1), y=_Guarded(max(B, 0)), delta=_Guarded(max(B, 0)),
                    dv=_Guarded(max(B, 0)), dm=_Guarded(max(B * n, 0)), de=_Guarded(max(B * n, 0)),
                    dc=_Guarded(max(B * nc, 0)))
    rc = _native.lib().pfrl_naf_td_loss(
        *[_p(xd[k]) for k in ORDER], B, n, int(f["clip_delta"]), int(f["mean"]),
        *[_p(outs[k].t) for k in ("loss", "y", "delta", "dv", "dm", "de")],
        _p(outs["dc"].t) if nc > 0 else None, _stream())
    torch.cuda.synchronize()
    return rc, outs, xd


def collect(outs, B, n):
    nc = n * (n - 1) // 2
    got = {k: outs[k].done(k) for k in ("loss", "y", "delta", "dv", "dm", "de")}
    if nc:
        got["dc"] = outs["dc"].done("dc")
    else:
        outs["dc"].untouched("dc (n == 1)")
        got["dc"] = torch.zeros(0)
    return got


def reference(x, f, dtype):
    """The composite expression in stock torch on the CPU, in ``dtype``."""
    from pfrl_amd.action_value import QuadraticActionValue
    from pfrl_amd.agents.dqn import compute_value_loss, compute_weighted_value_loss
    from pfrl_amd.functions.lower_triangular_matrix import lower_triangular_matrix

    c = lambda t: None if t is None else t.detach().to(dtype).clone()  # noqa: E731

    def action_value(v, m, e, tri, leaves=False):
        v, m, e, tri = c(v), c(m), c(e), c(tri)
        raw = [t for t in (v, m, e, tri) if t is not None]
        if leaves:
            for t in raw:
                t.requires_grad_(True)
        mu = torch.tanh(m) * c(x["half_width"]) + c(x["centre"]) if f["scale_mu"] else m
        diag = torch.exp(e)
        if tri is not None:
            L = lower_triangular_matrix(diag, tri)
            mat = torch.matmul(L, L.transpose(1, 2))
        else:
            mat = (diag ** 2).unsqueeze(2)
        low = x["low"].numpy() if f["bounds"] else None
        high = x["high"].numpy() if f["bounds"] else None
        av = QuadraticActionValue(mu, mat, v.reshape(-1, 1), min_action=low, max_action=high)
        if low is not None:         # (the class keeps its bounds in float32)
            av.min_action, av.max_action = c(x["low"]), c(x["high"])
        return av, raw

    qout, raw = action_value(x["v"], x["m"], x["e"], x["c"], leaves=True)
    y = qout.evaluate_actions(c(x["action"]))
    with torch.no_grad():
        tav, _ = action_value(x["tv"], x["tm"], x["te"], x["tc"])
        if f["double"]:
            nav, _ = action_value(x["tv"], x["m2"], x["te"], x["tc"])
            nxt = tav.evaluate_actions(nav.greedy_actions)
        else:
            nxt = tav.max
        t = c(x["reward"]) + c(x["discount"]) * (1.0 - c(x["terminal"])) * nxt
    acc = "mean" if f["mean"] else "sum"
    if f["weights"]:
        loss = compute_weighted_value_loss(y, t, c(x["weights"]), clip_delta=bool(f["clip_delta"]),
                                           batch_accumulator=acc)
    else:
        loss = compute_value_loss(y, t, clip_delta=bool(f["clip_delta"]), batch_accumulator=acc)
    loss.backward()
    out = dict(loss=loss.detach().reshape(1), y=y.detach(), delta=(y.detach() - t).abs(),
               dv=raw[0].grad.reshape(-1), dm=raw[1].grad.reshape(-1), de=raw[2].grad.reshape(-1),
               dc=raw[3].grad.reshape(-1) if len(raw) > 3 else torch.zeros(0, dtype=dtype))
    return {k: v.double() for k, v in out.items()}


@pytest.fixture(scope="module")
def sweep():
    """Every (flag row, n, B) once: guard zones and payloads checked on the way; the errors of the
    launch and of the float32 yardstick against float64, per flag row and quantity."""
    errs = {(r, q): [0.0, 0.0] for r in range(len(FLAG_ROWS)) for q in QUANTITIES}
    seed = 0
    for r, flags in enumerate(FLAG_ROWS):
        for B, n in SHAPES:
            seed += 1
            x, f = make_inputs(B, n, flags, seed)
            rc, outs, _ = launch(x, f, B, n)
            assert rc == 0, (flags, n, B, _native.lib().pfrl_amd_last_error())
            got = collect(outs, B, n)
            want = reference(x, f, torch.float64)
            yard = reference(x, f, torch.float32)
            for q in QUANTITIES + ("delta",):
                if want[q].numel() == 0:
                    continue
                e = errs.setdefault((r, q), [0.0, 0.0])
                e[0] = max(e[0], float((got[q].double().reshape(-1) - want[q]).abs().max()))
                e[1] = max(e[1], float((yard[q] - want[q]).abs().max()))
    return errs


@pytest.mark.parametrize("quantity", QUANTITIES + ("delta",))
def test_the_launch_errs_at_most_twice_the_float32_yardstick(sweep, quantity):
    for r, flags in enumerate(FLAG_ROWS):
        mine, yard = sweep[(r, quantity)]
        print("RATIO %-5s %s launch %.3e yardstick %.3e ratio %.2f" % (
            quantity, "".join(map(str, flags)), mine, yard, mine / yard if yard else float("nan")))
    for r, flags in enumerate(FLAG_ROWS):
        mine, yard = sweep[(r, quantity)]
        assert yard > 0.0, (quantity, flags)
        assert mine <= 2.0 * yard, (quantity, flags, mine, yard)


@pytest.mark.parametrize("B,n", [(32, 0), (32, 33), (0, 3), (-1, 3), (32, -1)])
def test_outside_the_gate_nothing_is_written(B, n):
    x, f = make_inputs(4, 3, FLAG_ROWS[1], 1)
    outs = {k: _Guarded(64) for k in ("loss", "y", "delta", "dv", "dm", "de", "dc")}
    rc, outs, _ = launch(x, f, B, n, outs)
    assert rc == PFRL_ERR_ARG
    for k, o in outs.items():
        o.untouched(k)


def test_missing_tensors_are_refused():
    x, f = make_inputs(4, 3, FLAG_ROWS[1], 1)
    for drop in ("c", "tc", "centre", "m", "reward"):
        outs = {k: _Guarded(64) for k in ("loss", "y", "delta", "dv", "dm", "de", "dc")}
        rc, outs, _ = launch(dict(x, **{drop: None}), f, 4, 3, outs)
        assert rc == PFRL_ERR_ARG, drop
        for k, o in outs.items():
            o.untouched(k)


@pytest.mark.parametrize("B,n", [(32, 3), (65, 6), (17, 17), (9, 32), (1, 1)])
def test_the_same_inputs_give_the_same_bits_eagerly_and_from_a_graph(B, n):
    for flags in (FLAG_ROWS[1], FLAG_ROWS[4]):
        x, f = make_inputs(B, n, flags, 11)
        _, outs, xd = launch(x, f, B, n)
        first = collect(outs, B, n)
        _, outs2, _ = launch(x, f, B, n)
        again = collect(outs2, B, n)
        assert all(torch.equal(first[k].view(torch.int32), again[k].view(torch.int32)) for k in first)
        # three replays of a captured graph into the same buffers, refilled with NaNs in between
        nc = n * (n - 1) // 2

        def call():
            return _native.lib().pfrl_naf_td_loss(
                *[_p(xd[k]) for k in ORDER], B, n, int(f["clip_delta"]), int(f["mean"]),
                *[_p(outs[k].t) for k in ("loss", "y", "delta", "dv", "dm", "de")],
                _p(outs["dc"].t) if nc > 0 else None, _stream())

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            assert call() == 0
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            assert call() == 0
        for _ in range(3):
            for o in outs.values():
                o.full.fill_(float("nan"))
            graph.replay()
            torch.cuda.synchronize()
            replayed = collect(outs, B, n)
            assert all(torch.equal(first[k].view(torch.int32), replayed[k].view(torch.int32))
                       for k in first)


@pytest.mark.parametrize("n", [1, 3, 6, 17, 32])
def test_inside_the_box_the_target_value_is_v_prime_exactly(n):
    """No Double, bounds on, scale_mu on: mu' lies inside the box, its clip is mu' itself and
    next == v'.  Read off through rows with y == 0 (v = 0 and action = mu: raw m = 0 gives mu = centre
    exactly), reward 0, discount 1 and not terminal, where |delta| = |0 - v'|; and by the bits of a
    launch without the bounds, whose target value is v' by construction."""
    B = 33
    for clip_delta, mean, weights in itertools.product((0, 1), repeat=3):
        flags = (1, 1, 0, clip_delta, mean, weights)
        x, f = make_inputs(B, n, flags, 5)
        x["v"].zero_()
        x["m"].zero_()
        x["action"] = x["centre"].expand(B, n).clone()
        x["reward"].zero_()
        x["discount"].fill_(1.0)
        x["terminal"].zero_()
        _, outs, _ = launch(x, f, B, n)
        got = collect(outs, B, n)
        assert bool((got["y"] == 0).all())
        assert torch.equal(got["delta"], x["tv"].abs())
        x2, f2 = make_inputs(B, n, flags, 6)
        _, outs, _ = launch(x2, f2, B, n)
        boxed = collect(outs, B, n)
        _, outs, _ = launch(dict(x2, low=None, high=None), f2, B, n)
        free = collect(outs, B, n)
        assert all(torch.equal(boxed[k].view(torch.int32), free[k].view(torch.int32)) for k in boxed)


def test_the_front_end_hands_the_launch_its_gradients():
    """``ops.naf_td_loss``: the same numbers as the C entry, the gradients through autograd, scaled by
    the upstream gradient; ``naf_td_loss_supported`` follows the gate."""
    from pfrl_amd import ops

    for n in (1, 3):
        x, f = make_inputs(32, n, FLAG_ROWS[1], 3)
        _, outs, xd = launch(x, f, 32, n)
        want = collect(outs, 32, n)
        leaves = [xd[k].clone().reshape(32, -1).requires_grad_(True) if xd[k] is not None else None
                  for k in ("v", "m", "e", "c")]
        assert ops.naf_td_loss_supported(*leaves, xd["tv"], xd["tm"], xd["te"], xd["tc"], xd["m2"],
                                         xd["action"])
        loss, y, delta = ops.naf_td_loss(*leaves, *[xd[k] for k in ORDER[4:]], True, True)
        (3.0 * loss).backward()
        assert torch.equal(loss.detach().cpu().reshape(1), want["loss"])
        assert torch.equal(y.cpu(), want["y"]) and torch.equal(delta.cpu(), want["delta"])
        for leaf, k in zip(leaves, ("dv", "dm", "de", "dc")):
            if leaf is not None:
                assert leaf.grad.shape == leaf.shape
                assert torch.equal(leaf.grad.cpu().reshape(-1), want[k] * 3.0)
        assert not ops.naf_td_loss_supported(leaves[0], leaves[1].double(), *leaves[2:], xd["tv"],
                                             xd["tm"], xd["te"], xd["tc"])
    wide = torch.zeros(4, 33, device=_dev())
    tri = torch.zeros(4, 33 * 16, device=_dev())
    col = torch.zeros(4, 1, device=_dev())
    assert not ops.naf_td_loss_supported(col, wide, wide, tri, col, wide, wide, tri)
