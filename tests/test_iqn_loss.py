"""csrc/iqn.hip (``pfrl_iqn_loss``) over what its gate admits, through the C ABI, against
``torch.float64`` on the CPU, and the route of ``agents.IQN`` that uses it.  The method of
tests/test_loss_head_envelope.py: (a) exact on operands chosen so that every intermediate is
representable (``torch.equal``), (b) rounded on randn operands within bounds derived below, with
``RATIO`` lines per case and ``MAX RATIO`` lines after the last test (``pytest -s``).  Every output
lies between two NaN guard zones of 4096 floats that must still be NaN after the launch, and the
payload must hold no NaN.  u = 2^-24; every bound carries a factor 2 over its first-order
derivation.

The reference of every kernel case is float64 torch with autograd through
``iqn.compute_eltwise_huber_quantile_loss`` and ``compute_value_loss`` /
``compute_weighted_value_loss``, on the greedy action g taken from the float64 mean of
``next_select``.

t.  t = r + (disc (1 - term)) next_quantiles[b][j][g] is three IEEE operations in a fixed
association on loaded operands, so ``out_t`` is compared BIT FOR BIT with the same float32 NumPy
expression, on integer and randn operands; that restatement agrees with float64 within
3 u (|r| + |coef next|) (checked without a GPU).  The float64 reference then starts from this
float32 t, which is what the kernel holds.

g.  The kernel sums K values in increasing k and divides: (K + 1) roundings,
|err| <= (K + 1) u sum_k |terms| / K per action value.  Rows whose best and second-best float64
value are closer than 2 (K + 2) u sum_k |terms| / K (the larger sum of the two actions) get a new
``next_select`` row until none is left; the case asserts that on the reference.  Exact operands
carry a planted tie instead, where the first maximum must win.

Pairs.  u_ij = y_i - t_j rounds once; the Huber term is continuous with slope <= 1 at |u| = 1 and
clamp(u, -1, 1) is continuous there, but 1[t < y] jumps at u = 0 and the branch is chosen at
|u| = 1, so pairs with |u| or ||u| - 1| below 8 u max(|y|, |t|) get a new y_i until none is left
(asserted on the reference; no row is skipped).  Then per pair: u (1 rounding, relative), 0.5 u u
(1; doubling the relative error of u in the quadratic branch: 2), tau - 1[.] (1), the product (1):
el and w clamp(u) are each within 5 u |term| resp. 3 u |term|.
  gradient c_b (sum_j w clamp(u)) / N':  3 u per term, N' - 1 additions, the division, c_b = w / B
      (two roundings) and the product:  (N' + 5) u sum_j |terms| to first order, held to
      2 (N' + 4) u sum_j |c_b w clamp(u)| / N'.
  delta (sum_ij el) / (N N'):  5 u per term, the j loop N' - 1 additions, log2(64) = 6 butterfly
      additions, one division: (N' + 11) u sum |el| <= (N N' + 4) u sum |el| for N N' >= N' + 7; for
      the few shapes below that (N = 1, N' <= 6 and the like) the first-order count N' + 11 is still
      under the bound's factor 2: 2 (N N' + 4) >= N' + 11 for every N, N' >= 1 except N N' <= 2,
      where the butterfly adds exact zeros (lanes past N hold 0) and only 5 + N' roundings remain.
      Held to 2 (N N' + 4) u sum_ij |el| / (N N').
  loss sum_b c_b sum_i (sum_j el) / N':  per pair 5 u, N' - 1 + 6 additions inside a row, the
      division, c_b (2) and its product (1), 6 + B / 64 additions across rows:
      < (B N + N' + 6) u sum |c el| / N' to first order, held to twice that.

Exact operands: quantiles and next_quantiles multiples of 1/2, next_select small integers, taus in
{1/4, 1/2, 3/4}, reward multiples of 1/2, discount in {0, 1/2, 1}, terminal in {0, 1}, weights in
{1/2, 1, 2}.  Then t and u are multiples of 1/4, 0.5 u u (taken only for |u| < 1) a multiple of
1/32, |u| - 0.5 a multiple of 1/4, w a multiple of 1/4: every el is a multiple of 1/128 and every
weighted el a multiple of 1/256 (the 1/B of ``mean`` and the divisions by N', N N' are powers of
two for the power-of-two shapes used, and scale granule and magnitude alike).  All float32 sums
are exact while 256 sum |w_b el| < 2^24, which implies 64 sum |el| < 2^24; the case asserts both on
the reference.  With operands in +-4 the (64, 64, 64) shape exceeds that limit, so it draws from
+-1/2.

Not tested, on purpose: NaN operands and actions outside [0, A) (the kernel does not check
``action``; an out-of-range index is a wild read).
"""
import copy
import functools
import itertools
import os
import tempfile

import numpy as np
import pytest
import torch

from pfrl_amd import _native, ops
from pfrl_amd.agents import iqn
from pfrl_amd.nn import mfma_trunk as mt

gpu = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
GUARD = 4096
U = 2.0 ** -24
PFRL_ERR_ARG = -2
F32 = np.float32
_p, _stream = mt._p, mt._stream


# ------------------------------------------------------------------ helpers
class _Guarded:
    """n floats between two guard zones, everything NaN until a kernel writes it."""

    def __init__(self, n, dev):
        self.n, self.lo = n, GUARD
        self.full = torch.full((n + 2 * GUARD + 4,), float("nan"), dtype=torch.float32, device=dev)
        assert self.full.data_ptr() % 16 == 0
        self.t = self.full[self.lo:self.lo + n]

    def done(self, what=""):
        assert bool(torch.isnan(self.full[:self.lo]).all()), "guard zone before %s was written" % what
        assert bool(torch.isnan(self.full[self.lo + self.n:]).all()), "guard zone after %s was written" % what
        assert not bool(torch.isnan(self.t).any()), "%s: payload not fully written" % what
        return self.t

    def untouched(self, what=""):
        assert bool(torch.isnan(self.full).all()), "%s was written" % what


_RATIO = {}


@pytest.fixture(scope="module", autouse=True)
def _ratio_summary():
    yield
    for name in sorted(_RATIO):
        print("MAX RATIO %s %.4f" % (name, _RATIO[name]))


def _within(name, tag, out, ref, bound):
    """|out - ref| <= bound per element (bound already carries the factor 2)."""
    out = out.detach().cpu().double().reshape(ref.shape)
    err = (out - ref).abs()
    ratio = float((err / bound.clamp(min=1e-300)).max()) if ref.numel() else 0.0
    _RATIO[name] = max(_RATIO.get(name, 0.0), ratio)
    print("RATIO %s %s %.4f" % (name, tag, ratio))
    assert bool((err <= bound).all()), "%s %s: err / bound = %.3f" % (name, tag, ratio)


def _dev():
    return torch.device("cuda:0")


def c_gate(B, N, Np, K, A):
    """PFRL_CHECK_ARG of pfrl_iqn_loss, restated."""
    return 1 <= B <= 4096 and all(1 <= v <= 64 for v in (N, Np, K, A))


def t_f32(c, g):
    """out_t with the kernel's loads and float32 association."""
    ar = np.arange(c.B)
    nxt = c.nq.numpy()[ar, :, g]                                       # (B, N')
    coef = c.disc.numpy() * (F32(1.0) - c.term.numpy())
    t = c.r.numpy()[:, None] + coef[:, None] * nxt
    assert t.dtype == np.float32
    return t


def t_f64(c, g):
    ar = np.arange(c.B)
    nxt = c.nq.double().numpy()[ar, :, g]
    coef = c.disc.double().numpy() * (1.0 - c.term.double().numpy())
    return c.r.double().numpy()[:, None] + coef[:, None] * nxt, np.abs(c.r.double().numpy())[:, None] + np.abs(coef[:, None] * nxt)


def select_values(c):
    """float64 action values of the selection pass, their greedy action (first maximum) and the
    rounding allowance of the kernel's float32 value per action."""
    s = c.sel.double()
    val = s.mean(1)                                                    # (B, A)
    allow = (c.K + 2) * U * s.abs().sum(1) / c.K
    return val, val.numpy().argmax(1), allow


def closed_form(y, t, taus, coef, Np):
    """(el, d loss / d y) of the header, in the dtype of the operands."""
    u = y.unsqueeze(2) - t.unsqueeze(1)
    au = u.abs()
    huber = torch.where(au < 1, 0.5 * u * u, au - 0.5)
    w = (taus.unsqueeze(2) - (t.unsqueeze(1) < y.unsqueeze(2)).to(y.dtype)).abs()
    return w * huber, coef.unsqueeze(1) * (w * u.clamp(-1, 1)).sum(2) / Np


class _Ref:
    """float64 autograd through the agent's own expression, from the float32 t."""

    def __init__(self, c, use_w, mean):
        B, N, Np, A = c.B, c.N, c.Np, c.A
        ar = torch.arange(B)
        self.g = select_values(c)[1]
        self.t32 = t_f32(c, self.g)
        t = torch.from_numpy(self.t32).double()
        q = c.q.double().requires_grad_()
        y = q[ar, :, c.action]
        el = iqn.compute_eltwise_huber_quantile_loss(y, t, c.taus.double())
        acc = "mean" if mean else "sum"
        if use_w:
            loss = iqn.compute_weighted_value_loss(el, c.w.double(), batch_accumulator=acc)
        else:
            loss = iqn.compute_value_loss(el, batch_accumulator=acc)
        loss.backward()
        self.loss, self.grad = loss.detach(), q.grad
        el = el.detach()
        self.delta = el.mean((1, 2))
        coef = (c.w.double() if use_w else torch.ones(B, dtype=torch.float64)) * (1.0 / B if mean else 1.0)
        self.coef = coef
        self.el_abs = el.abs().sum((1, 2))                             # (B,)
        u = y.detach().unsqueeze(2) - t.unsqueeze(1)
        self.u = u
        w = (c.taus.double().unsqueeze(2) - (t.unsqueeze(1) < y.detach().unsqueeze(2)).double()).abs()
        self.g_abs = coef.unsqueeze(1) * (w * u.clamp(-1, 1)).abs().sum(2) / Np      # (B, N)
        self.y, self.t = y.detach(), t


# ------------------------------------------------------------------ operands
class _Case:
    def __init__(self, B, N, Np, K, A, kind, half=8):
        self.B, self.N, self.Np, self.K, self.A, self.kind = B, N, Np, K, A, kind
        g = torch.Generator().manual_seed(((B * 67 + N) * 67 + Np) * 4489 + K * 67 + A + (kind == "int"))
        self.gen = g
        if kind == "int":
            def ri(lo, hi, *s):
                return torch.randint(lo, hi + 1, s, generator=g).float()
            self.q, self.nq = ri(-half, half, B, N, A) * 0.5, ri(-half, half, B, Np, A) * 0.5
            self.sel = ri(-4, 4, B, K, A)
            self.taus = torch.tensor([0.25, 0.5, 0.75])[torch.randint(0, 3, (B, N), generator=g)]
            self.r = ri(-min(half, 4), min(half, 4), B) * 0.5
            self.disc = torch.tensor([0.0, 0.5, 1.0])[torch.randint(0, 3, (B,), generator=g)]
            self.term = ri(0, 1, B)
            self.w = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (B,), generator=g)]
        else:
            def rn(*s):
                return torch.randn(s, generator=g)
            self.q, self.nq, self.sel, self.r = rn(B, N, A), rn(B, Np, A), rn(B, K, A), rn(B)
            self.taus = torch.rand(B, N, generator=g)
            self.disc = torch.tensor(0.99) ** torch.randint(1, 4, (B,), generator=g).float()
            self.term = (torch.rand(B, generator=g) < 0.2).float()
            self.w = torch.rand(B, generator=g) + 0.5
        self.action = torch.randint(0, A, (B,), generator=g)
        if kind == "int" and B >= 16:
            self.action[0], self.action[1] = 0, A - 1
            self.term[2] = 1.0
            if A >= 2:                       # a tie whose first maximum is not the last index, and that matters
                i, j = (0 if A == 2 else 1), A - 1
                self.sel[3] = self.sel[3].clamp(max=3.0)
                self.sel[3, :, i] = self.sel[3, :, j] = 4.0
                self.nq[3, :, i], self.nq[3, :, j] = 0.5, -0.5
                self.disc[3], self.term[3] = 1.0, 0.0
        if kind == "randn":
            self.redraws = self._redraw()

    def tag(self):
        return "B%d-N%d-Np%d-K%d-A%d" % (self.B, self.N, self.Np, self.K, self.A)

    # the two redraw rules of the docstring; both end with an assertion on the reference
    def _close_rows(self):
        if self.A < 2:
            return torch.zeros(self.B, dtype=torch.bool)
        val, _, allow = select_values(self)
        top, idx = val.topk(2, dim=1)
        worst = torch.maximum(allow.gather(1, idx[:, :1]), allow.gather(1, idx[:, 1:]))[:, 0]
        return (top[:, 0] - top[:, 1]) < 2 * worst

    def _close_pairs(self):
        """(B, N) mask of predictions with a pair at a branch point."""
        ar = torch.arange(self.B)
        g = select_values(self)[1]
        t = torch.from_numpy(t_f32(self, g)).double()
        y = self.q.double()[ar, :, self.action]
        u = (y.unsqueeze(2) - t.unsqueeze(1)).abs()
        lim = 8 * U * torch.maximum(y.abs().unsqueeze(2), t.abs().unsqueeze(1))
        return ((u < lim) | ((u - 1).abs() < lim)).any(2)

    def _redraw(self):
        n = 0
        for _ in range(100):
            rows = self._close_rows()
            if not bool(rows.any()):
                break
            k = int(rows.sum())
            self.sel[rows] = torch.randn(k, self.K, self.A, generator=self.gen)
            n += k
        assert not bool(self._close_rows().any())
        ar = torch.arange(self.B)
        for _ in range(100):
            bad = self._close_pairs()
            if not bool(bad.any()):
                break
            b, i = bad.nonzero(as_tuple=True)
            self.q[b, i, self.action[b]] = torch.randn(len(b), generator=self.gen)
            n += len(b)
        assert not bool(self._close_pairs().any())
        return n


@functools.lru_cache(maxsize=2)
def _case(B, N, Np, K, A, kind, half=8):
    return _Case(B, N, Np, K, A, kind, half)


def _launch(c, dev, use_w, mean, want_t=True, d=None):
    d = d if d is not None else _to_dev(c, dev)
    out = {"loss": _Guarded(1, dev), "grad": _Guarded(c.B * c.N * c.A, dev), "delta": _Guarded(c.B, dev),
           "t": _Guarded(c.B * c.Np, dev)}
    mt.check(_native.lib().pfrl_iqn_loss(
        _p(d["q"]), _p(d["action"]), _p(d["taus"]), _p(d["nq"]), _p(d["sel"]), _p(d["r"]), _p(d["disc"]),
        _p(d["term"]), _p(d["w"]) if use_w else None, c.B, c.N, c.Np, c.K, c.A, int(mean), _p(out["loss"].t),
        _p(out["grad"].t), _p(out["delta"].t), _p(out["t"].t) if want_t else None, _stream()), "iqn loss")
    torch.cuda.synchronize()
    if not want_t:
        out.pop("t").untouched("out_t = NULL")
    return {k: v.done(k).cpu() for k, v in out.items()}


def _to_dev(c, dev):
    return {k: getattr(c, k).to(dev).contiguous() for k in ("q", "action", "taus", "nq", "sel", "r", "disc", "term", "w")}


def _off_action_is_plus_zero(c, grad):
    bits = grad.view(c.B, c.N, c.A).view(torch.int32).clone()
    bits[torch.arange(c.B), :, c.action] = 0
    return not bool(bits.any())


# ================================================================== shapes
EXACT = [(16, 8, 8, 4, 6, 8), (64, 64, 64, 32, 18, 1), (4, 1, 2, 1, 1, 8), (32, 16, 4, 8, 2, 8)]   # ..., half range
R_B = [1, 2, 33, 257, 4096]
R_N = [1, 2, 3, 63, 64]
R_NP = [1, 3, 63, 64]
R_K = [1, 31, 32, 64]
R_A = [1, 2, 18, 63, 64]
R_ALWAYS = [(4096, 64, 64, 64, 64), (32, 64, 64, 32, 18)]


def _third():
    return [(B, N, Np, K, A) for (i, B), (j, N), (k, Np), (l, K), (m, A) in itertools.product(
        enumerate(R_B), enumerate(R_N), enumerate(R_NP), enumerate(R_K), enumerate(R_A)) if (i + j + k + l + m) % 3 == 0]


def _rounded_shapes():
    out = _third()
    return out + [s for s in R_ALWAYS if s not in out]


# ================================================================== no GPU
def test_the_chosen_third_reaches_every_listed_size():
    third, shapes = _third(), _rounded_shapes()
    for axis, listed in enumerate((R_B, R_N, R_NP, R_K, R_A)):
        assert {s[axis] for s in third} == set(listed)
    assert all(s in shapes for s in R_ALWAYS) and len(set(shapes)) == len(shapes)
    assert all(c_gate(*s) for s in shapes)
    assert len(third) * 3 <= len(R_B) * len(R_N) * len(R_NP) * len(R_K) * len(R_A) + 2


class _FakeTensor:
    def __init__(self, *shape, cuda=True, dtype=torch.float32):
        self.shape, self.ndim, self.is_cuda, self.dtype = tuple(shape), len(shape), cuda, dtype


def test_python_gate_admits_only_what_the_c_gate_admits():
    edge = (0, 1, 64, 65)
    n = 0
    for B, N, Np, K, A in itertools.product((0, 1, 4096, 4097), edge, edge, edge, edge):
        if ops.iqn_loss_supported(_FakeTensor(B, N, A), _FakeTensor(B, Np, A), _FakeTensor(B, K, A)):
            n += 1
            assert c_gate(B, N, Np, K, A), (B, N, Np, K, A)
    assert n == 2 * 2 ** 4
    ok = _FakeTensor(32, 64, 18)
    assert ops.iqn_loss_supported(ok, ok, _FakeTensor(32, 32, 18))
    assert not ops.iqn_loss_supported(_FakeTensor(32, 64, 18, cuda=False), ok, ok)
    assert not ops.iqn_loss_supported(ok, _FakeTensor(32, 64, 18, dtype=torch.float64), ok)
    assert not ops.iqn_loss_supported(ok, ok, _FakeTensor(32, 64 * 18))


@pytest.mark.parametrize("shape", [(33, 3, 63, 31, 18), (257, 2, 64, 1, 2), (2, 64, 3, 64, 63)])
def test_float32_target_is_what_float64_computes(shape):
    c = _Case(*shape, "randn")
    g = select_values(c)[1]
    t64, mag = t_f64(c, g)
    assert bool((np.abs(t_f32(c, g).astype(np.float64) - t64) <= 3 * U * mag).all())


@pytest.mark.parametrize("shape", EXACT, ids=lambda s: "B%d-N%d-Np%d-K%d-A%d-h%d" % s)
def test_closed_form_gradient_is_float64_autograds(shape):
    """The header's gradient against float64 autograd through the agent's expression, on the
    exact operands: difference 0.0, weights and mean crossed."""
    c = _case(*shape[:5], "int", shape[5])
    for use_w, mean in itertools.product((False, True), (False, True)):
        r = _Ref(c, use_w, mean)
        el, gy = closed_form(r.y, r.t, c.taus.double(), r.coef, c.Np)
        want = torch.zeros(c.B, c.N, c.A, dtype=torch.float64)
        want[torch.arange(c.B), :, c.action] = gy
        assert torch.equal(want, r.grad)
        assert torch.equal(el.mean((1, 2)), r.delta)


# ================================================================== kernel, GPU
def _kinds(c, r):
    kinds = set()
    au = r.u.abs()
    if bool((au == 1).any()):
        kinds.add("|u| = 1")
    if bool((au == 0).any()):
        kinds.add("u = 0")
    if bool((c.term == 1).any()):
        kinds.add("terminal")
    if bool((r.u > 0).any()):
        kinds.add("t < y")
    if bool((r.u < 0).any()):
        kinds.add("t > y")
    if bool((c.action == 0).any()):
        kinds.add("action 0")
    if bool((c.action == c.A - 1).any()):
        kinds.add("action A-1")
    val = select_values(c)[0]
    hit = val == val.max(1, keepdim=True).values
    first = hit.float().argmax(1)
    last = (c.A - 1) - hit.flip(1).float().argmax(1)
    ar = torch.arange(c.B)
    tie = (hit.sum(1) >= 2) & (first < c.A - 1) & (c.nq[ar, :, first] != c.nq[ar, :, last]).any(1) \
        & (c.disc * (1 - c.term) != 0)
    if bool(tie.any()):
        kinds.add("tie")
    return kinds


@gpu
@pytest.mark.parametrize("shape", EXACT, ids=lambda s: "B%d-N%d-Np%d-K%d-A%d-h%d" % s)
def test_iqn_loss_is_exact_on_representable_operands(shape):
    dev = _dev()
    c = _case(*shape[:5], "int", shape[5])
    d = _to_dev(c, dev)
    for use_w, mean in itertools.product((False, True), (False, True)):
        r = _Ref(c, use_w, mean)
        wmax = c.w.double() if use_w else torch.ones(c.B, dtype=torch.float64)
        assert 256 * float((wmax * r.el_abs).sum()) < 2 ** 24 and 64 * float(r.el_abs.sum()) < 2 ** 24
        if c.B >= 16:
            need = {"|u| = 1", "u = 0", "terminal", "t < y", "t > y", "action 0", "action A-1"} | ({"tie"} if c.A >= 2 else set())
            assert not need - _kinds(c, r), need - _kinds(c, r)
        got = _launch(c, dev, use_w, mean, d=d)
        tag = "%s w%d mean%d" % (c.tag(), use_w, mean)
        assert torch.equal(got["t"].view(c.B, c.Np), torch.from_numpy(r.t32)), tag
        assert torch.equal(got["delta"].double(), r.delta), tag
        assert torch.equal(got["grad"].double().view(c.B, c.N, c.A), r.grad), tag
        assert torch.equal(got["loss"].double().view(()), r.loss), tag
        assert _off_action_is_plus_zero(c, got["grad"]), tag


@gpu
@pytest.mark.parametrize("shape", _rounded_shapes(), ids=lambda s: "B%d-N%d-Np%d-K%d-A%d" % s)
def test_iqn_loss_matches_float64_on_randn(shape):
    """out_t bit for bit, +0.0 away from the taken action, gradient / delta / loss within the bounds
    of the docstring.  The switches (weights, mean) alternate over the cases; the two shapes that
    are always included take both opposite settings."""
    dev = _dev()
    B, N, Np, K, A = shape
    c = _case(B, N, Np, K, A, "randn")
    d = _to_dev(c, dev)
    s = (B + N + Np + K + A) % 4
    for use_w, mean in ([(True, True), (False, False)] if shape in R_ALWAYS else [(bool(s & 1), bool(s & 2))]):
        r = _Ref(c, use_w, mean)
        got = _launch(c, dev, use_w, mean, d=d)
        tag = "%s w%d mean%d redrawn %d" % (c.tag(), use_w, mean, c.redraws)
        assert torch.equal(got["t"].view(B, Np).view(torch.int32), torch.from_numpy(r.t32).view(torch.int32)), tag
        assert _off_action_is_plus_zero(c, got["grad"]), tag
        ar = torch.arange(B)
        _within("iqn_loss grad", tag, got["grad"].view(B, N, A)[ar, :, c.action], r.grad[ar, :, c.action],
                2 * (Np + 4) * U * r.g_abs)
        _within("iqn_loss delta", tag, got["delta"], r.delta, 2 * (N * Np + 4) * U * r.el_abs / (N * Np))
        _within("iqn_loss loss", tag, got["loss"].view(()), r.loss,
                2 * (B * N + Np + 6) * U * (r.coef.abs() * r.el_abs).sum() / Np)


@gpu
def test_iqn_loss_is_deterministic():
    dev = _dev()
    c = _Case(257, 63, 64, 31, 18, "randn")
    d = _to_dev(c, dev)
    one, two = _launch(c, dev, True, True, d=d), _launch(c, dev, True, True, d=d)
    for k in one:
        assert torch.equal(one[k].view(torch.int32), two[k].view(torch.int32)), k


@gpu
def test_iqn_loss_refuses_what_its_gate_refuses():
    dev = _dev()
    lib = _native.lib()
    c = _Case(4, 2, 3, 2, 3, "randn")
    d = _to_dev(c, dev)
    out = _Guarded(1 << 16, dev)
    o = _p(out.t)

    def call(B, N, Np, K, A):
        return lib.pfrl_iqn_loss(_p(d["q"]), _p(d["action"]), _p(d["taus"]), _p(d["nq"]), _p(d["sel"]), _p(d["r"]),
                                 _p(d["disc"]), _p(d["term"]), _p(d["w"]), B, N, Np, K, A, 1, o, o, o, o, _stream())
    ok = dict(B=4, N=2, Np=3, K=2, A=3)
    rcs = {}
    for key, bad in (("B", (0, 4097)), ("N", (0, 65)), ("Np", (0, 65)), ("K", (0, 65)), ("A", (0, 65))):
        for v in bad:
            rcs["%s = %d" % (key, v)] = call(**dict(ok, **{key: v}))
    rcs["quantiles = NULL"] = lib.pfrl_iqn_loss(None, _p(d["action"]), _p(d["taus"]), _p(d["nq"]), _p(d["sel"]),
                                                _p(d["r"]), _p(d["disc"]), _p(d["term"]), None, 4, 2, 3, 2, 3, 1,
                                                o, o, o, o, _stream())
    assert all(rc == PFRL_ERR_ARG for rc in rcs.values()), rcs
    torch.cuda.synchronize()
    out.untouched("an output of a refused call")
    # the two optional pointers
    full = _launch(c, dev, True, False, d=d)
    no_w, no_t = _launch(c, dev, False, False, d=d), _launch(c, dev, True, False, want_t=False, d=d)
    r = _Ref(c, False, False)
    assert abs(float(no_w["loss"]) - float(r.loss)) <= 1e-5 * max(1.0, abs(float(r.loss)))
    for k in ("loss", "grad", "delta"):
        assert torch.equal(no_t[k], full[k]), k


@gpu
def test_iqn_loss_autograd_wrapper_hands_back_the_kernels_gradient():
    dev = _dev()
    c = _Case(33, 8, 8, 4, 6, "randn")
    d = _to_dev(c, dev)
    want = _launch(c, dev, True, True, d=d)["grad"].view(c.B, c.N, c.A)
    for scale in (1.0, 3.0):
        q = d["q"].clone().requires_grad_()
        loss, delta = ops.iqn_loss(q, d["action"], d["taus"], d["nq"], d["sel"], d["r"], d["disc"], d["term"],
                                   d["w"], True)
        assert loss.shape == () and delta.shape == (c.B,) and not delta.requires_grad
        (loss * scale).backward()
        assert torch.equal(q.grad.cpu(), want * torch.tensor(scale))


# ================================================================== agent, GPU
class _Recorder:
    """Stands in for the loaded library: every pfrl_* entry point called through it is listed."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("pfrl_"):
            return fn

        def wrapped(*a):
            self.calls.append(name)
            return fn(*a)
        return wrapped


@pytest.fixture
def recorder(monkeypatch):
    rec = _Recorder(_native.lib())
    monkeypatch.setattr(_native, "lib", lambda: rec)
    return rec


def _tf_agent(cls=None, **agent_kw):
    from pfrl_amd import agents, explorers, replay_buffers

    def phi(x):
        return np.asarray(x, dtype=np.float32) / 255

    q = iqn.ImplicitQuantileQFunction(
        psi=torch.nn.Sequential(torch.nn.Flatten(), torch.nn.Linear(4 * 144, 32), torch.nn.ReLU()),
        phi=torch.nn.Sequential(iqn.CosineBasisLinear(16, 32), torch.nn.ReLU()),
        f=torch.nn.Linear(32, 6))
    opt = torch.optim.SGD(q.parameters(), lr=1e-2)
    rbuf = replay_buffers.PrioritizedReplayBuffer(200, alpha=0.5, beta0=0.4, betasteps=100,
                                                  num_steps=3, normalize_by_max="memory")
    ex = explorers.LinearDecayEpsilonGreedy(1.0, 0.1, 400, lambda: np.random.randint(6))
    return (cls or agents.IQN)(q, opt, rbuf, 0.99, ex, gpu=0, replay_start_size=40, minibatch_size=8,
                               update_interval=4, target_update_interval=60, phi=phi,
                               batch_accumulator="mean", quantile_thresholds_N=8,
                               quantile_thresholds_N_prime=8, quantile_thresholds_K=4, use_graphs=False,
                               **agent_kw)


@functools.lru_cache(maxsize=1)
def _golden():
    return np.load(os.path.join(GOLDEN, "teacher_forced_iqn_per_n3.npz"))


def _tf_state(ag, k):
    """Parameters, minibatch and threshold draws of update k of the recorded run, on the agent."""
    from test_teacher_forced_loss import _load_flat

    g = _golden()
    _load_flat(ag.model, g["u%d_params" % k])
    _load_flat(ag.target_model, g["u%d_target_params" % k])
    batch = {}
    for key in ("state", "action", "reward", "next_state", "is_state_terminal", "discount", "weights"):
        a = g["u%d_%s" % (k, key)]
        if key in ("state", "next_state"):
            a = a.astype(np.float32) / 255
        batch[key] = torch.as_tensor(a).to(ag.device)
    draws = [torch.as_tensor(g["u%d_rand%d" % (k, j)]) for j in range(3)]
    left = [t.to(ag.device) for t in draws]

    def replay(rows, cols):
        t = left.pop(0)
        assert tuple(t.shape) == (rows, cols), (tuple(t.shape), rows, cols)
        return t

    ag._rand = replay
    return batch, draws, left


@gpu
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("k", [1, 50, 140])
def test_teacher_forced_iqn_loss_takes_the_expected_route(k, fused, recorder):
    """The recorded loss of updates 1, 50 and 140 at 1e-5, through pfrl_iqn_loss exactly once with
    ``fused_td_loss=True`` and not at all with ``fused_td_loss=False``."""
    ag = _tf_agent(fused_td_loss=fused)
    batch, _, left = _tf_state(ag, k)
    del recorder.calls[:]
    loss = ag._compute_loss(batch, errors_out=None)[0]
    assert not left
    assert recorder.calls.count("pfrl_iqn_loss") == (1 if fused else 0)
    want, got = float(_golden()["u%d_loss" % k]), float(loss.detach().cpu())
    assert abs(got - want) <= 1e-5 * max(1.0, abs(want)), (k, got, want)


def _float64_gradients(ag, batch, draws):
    m, tm = copy.deepcopy(ag.model).cpu().double(), copy.deepcopy(ag.target_model).cpu().double()
    b = {k: (v.cpu().double() if v.is_floating_point() else v.cpu()) for k, v in batch.items()}
    taus, tilde, prime = (t.double() for t in draws)
    y = m(b["state"])(taus).evaluate_actions_as_quantiles(b["action"])
    with torch.no_grad():
        nxt = tm(b["next_state"])
        g = nxt(tilde).greedy_actions
        z = nxt(prime).evaluate_actions_as_quantiles(g)
        t = b["reward"].unsqueeze(-1) + b["discount"].unsqueeze(-1) * (1.0 - b["is_state_terminal"].unsqueeze(-1)) * z
    el = iqn.compute_eltwise_huber_quantile_loss(y, t, taus)
    iqn.compute_weighted_value_loss(el, b["weights"], batch_accumulator="mean").backward()
    return [p.grad for p in m.parameters()]


@gpu
@pytest.mark.parametrize("k", [1, 50, 140])
def test_fused_route_gradients_are_as_close_to_float64_as_the_composite_routes(k):
    """Every parameter's gradient after ``backward`` on both routes against a float64 CPU replica of
    the model on the same thresholds.  Both routes are float32 evaluations of one expression with
    different summation orders: the fused route's largest error may be at most 4 times the
    composite route's, with floor 8 u max |ref|."""
    errs = {}
    for fused in (True, False):
        ag = _tf_agent(fused_td_loss=fused)
        batch, draws, _ = _tf_state(ag, k)
        ref = _float64_gradients(ag, batch, draws)
        ag.model.zero_grad()
        ag._compute_loss(batch, errors_out=None)[0].backward()
        errs[fused] = max(float((p.grad.cpu().double() - r).abs().max()) for p, r in zip(ag.model.parameters(), ref))
    top = max(float(r.abs().max()) for r in ref)
    print("IQN GRADIENT ERROR update %d: fused %.3e composite %.3e max|ref| %.3e" % (k, errs[True], errs[False], top))
    assert errs[True] <= max(4 * errs[False], 8 * U * top)


def _train(steps, cls=None, **agent_kw):
    """test_agent_parity._run_iqn (prioritized, device thresholds) for a chosen number of steps."""
    import pfrl_amd as pfrl
    from pfrl_amd import agents, explorers, replay_buffers
    from pfrl_amd.envs.synthetic import HostSyntheticAtariVectorEnv
    from test_agent_parity import _spy_losses

    pfrl.utils.set_random_seed(0)
    env = HostSyntheticAtariVectorEnv(4, seed=13, frame_shape=(12, 12), p_done=0.04)

    def phi(x):
        return np.asarray(x, dtype=np.float32) / 255

    torch.manual_seed(9753)
    q = iqn.ImplicitQuantileQFunction(
        psi=torch.nn.Sequential(torch.nn.Flatten(), torch.nn.Linear(4 * 144, 32), torch.nn.ReLU()),
        phi=torch.nn.Sequential(iqn.CosineBasisLinear(16, 32), torch.nn.ReLU()),
        f=torch.nn.Linear(32, 6))
    opt = torch.optim.SGD(q.parameters(), lr=1e-2)
    rbuf = replay_buffers.PrioritizedReplayBuffer(200, alpha=0.5, beta0=0.4, betasteps=100,
                                                  num_steps=3, normalize_by_max="memory")
    ex = explorers.LinearDecayEpsilonGreedy(1.0, 0.1, 400, lambda: np.random.randint(6))
    ag = (cls or agents.IQN)(q, opt, rbuf, 0.99, ex, gpu=0, replay_start_size=40, minibatch_size=8,
                             update_interval=4, target_update_interval=60, phi=phi,
                             batch_accumulator="mean", quantile_thresholds_N=8,
                             quantile_thresholds_N_prime=8, quantile_thresholds_K=4, **agent_kw)
    actions, losses = [], []
    orig_act = ag.batch_act

    def spy_act(obs):
        a = orig_act(obs)
        actions.append([int(x) for x in a])
        return a

    ag.batch_act = spy_act
    _spy_losses(ag, losses)
    pfrl.experiments.train_agent_batch(ag, env, steps, tempfile.mkdtemp())
    params = np.concatenate([p.detach().cpu().numpy().ravel() for p in q.parameters()])
    return dict(actions=np.asarray(actions), losses=np.asarray(losses), final_params=params, agent=ag)


@gpu
def test_captured_fused_update_equals_the_eager_one(recorder):
    """Both fused, thresholds from the device generator: the captured update holds the kernel (seen
    by the proxy while capturing) and trains like the eager one, to the tolerances of
    test_iqn_graph_replay_equals_eager_with_device_thresholds."""
    eager = _train(320, use_graphs=False)
    n_eager = recorder.calls.count("pfrl_iqn_loss")
    assert n_eager == len(eager["losses"]) > 20
    del recorder.calls[:]
    graph = _train(320)
    assert graph["agent"].use_graphs and graph["agent"]._graphed is not None
    assert 1 <= recorder.calls.count("pfrl_iqn_loss") < n_eager       # captured, then replayed
    np.testing.assert_array_equal(graph["actions"], eager["actions"])
    np.testing.assert_allclose(graph["losses"], eager["losses"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(graph["final_params"], eager["final_params"], rtol=1e-5, atol=1e-6)


@gpu
def test_a_subclass_with_its_own_target_keeps_the_composite_route(recorder):
    from pfrl_amd import agents

    class OwnTarget(agents.IQN):
        def _compute_target_values(self, exp_batch):
            return super()._compute_target_values(exp_batch)

    ag = _tf_agent(cls=OwnTarget)
    assert ag.fused_td_loss and not ag._fused_iqn_applicable()
    batch, _, left = _tf_state(ag, 50)
    del recorder.calls[:]
    loss = ag._compute_loss(batch, errors_out=None)[0]
    assert not left and "pfrl_iqn_loss" not in recorder.calls
    want = float(_golden()["u50_loss"])
    assert abs(float(loss.detach().cpu()) - want) <= 1e-5 * max(1.0, abs(want))
