"""csrc/operator_td.hip (``pfrl_dqn_operator_td_loss``) over what its gate admits, through the C
ABI, against references computed on the CPU only, and the route of the six operator agents (AL,
PAL, DoublePAL, DPP, DPPL, DPPGreedy) that uses it.  The method of tests/test_iqn_loss.py and
tests/test_loss_head_envelope.py: every output lies between two NaN guard zones of 4096 floats
that must still be NaN after the launch, the payload must hold no NaN, ``RATIO`` lines per case
and ``MAX RATIO`` lines after the last test (``pytest -s``).  u = 2^-24; every derived bound
carries a factor 2 over its first-order derivation.

Ops 0, 1, 2, 5 (AL, PAL, DoublePAL, DPPGreedy).  The target is a fixed sequence of IEEE
operations on loaded operands (maxima are exact), so ``out_t``, ``y`` (a load) and
|delta| = |fl(y - t)| are compared BIT FOR BIT with the same float32 NumPy expression
(``t_f32``), on integer and on randn operands.  That restatement agrees with the float64
composite expression of the agents within 6 u mag, mag = |r| + |coef next| + |alpha gap| (AL
family) resp. |Q'(s,a)| + |r| + |coef L'| + |L| (DPPGreedy): coef = fl(disc fl(1 - term)) carries
2 u, its product 3 u, every further sum one u of its own magnitude, alpha gap 2 u -- no
coefficient of a term exceeds 6 (checked without a GPU).  The float64 reference of loss and
gradient then starts from this float32 t, which is what the kernel holds: nothing is carried,
E_t = 0.

Exact operands (ops 0, 1, 2, 5): Q matrices integers -4..4, rewards multiples of 1/2, discount
in {0, 1/2, 1}, terminal in {0, 1}, weights in {1/2, 1, 2}, alpha in {1/2, 1/4}.  Then t and
delta are multiples of 1/4, the Huber / squared terms multiples of 1/32, the weighted ones of
1/64, and all float32 sums are exact while 64 sum |w L| < 2^24; the case asserts that and the
issue's sum < 2^20 on the reference.  ``mean`` divides by B: exact at power-of-two B only, so
loss and gradient are compared with ``torch.equal`` there and without ``mean`` elsewhere.

Ops 3, 4 (DPP, DPPL).  The reference of t is float64 torch through
``DiscreteActionValue.compute_expectation`` resp. ``torch.logsumexp``.  With z_a = fl(eta x_a),
m = fl(eta max x) = max_a z_a (rounding is monotone), ``expf`` and ``logf`` assumed 1 ulp = 2 u
relative (the project's standing assumption):
  argument z_a - m: u |z_a| from the product, u |z_a - m| from the difference (the shift m is the
      same float in every term, so its own error cancels):   d_a = u (|z_a| + |z_a - m|)
  e_a = expf(.): relative eps_a = d_a + 2 u;   S = sum_a e_a (A - 1 additions of positive terms):
      relative eps_S = max_a eps_a + (A - 1) u
  DPP:  p_a = e_a / S (u), p_a x_a (u), the sum over a ((A - 1) u of sum |p_a x_a|):
      E_L = (max_a eps_a + eps_S + (A + 1) u) sum_a |p_a x_a|
  DPPL: logf(S): eps_S + 2 u |log S|;  m + log S: u |m + log S|;  the division: u |L|:
      E_L = (eps_S + 2 u |log S| + u |m + log S|) / eta + u |L|
  t = fl(fl(Q'(s,a) + ahead) - L_c), ahead = fl(r + fl(coef L_n)):
      E_t = |coef| E_Ln + E_Lc + 3 u |coef L_n| + u |ahead| + u |Q'(s,a) + ahead| + u |t|
``out_t`` is held to 2 E_t.  Carried on, as the E_d / E_L / E_g chain of COVERAGE row a24:
E_d = E_t + u |d| (|delta| held to 2 E_d); the Huber term has slope <= 1 and the squared term
slope |d|, both branches and clamp(d, -1, 1) are continuous at |delta| = 1, so a row's loss term
moves by at most s_b E_t with s_b = 1 (Huber) or |d| + E_t (squared) and its gradient by E_t.
Rows with ||delta| - 1| <= 2 E_d get a new reward until the reference reports none (asserted; no
row is skipped).

Rounded, all ops (E_t = 0 for ops 0, 1, 2, 5):
  gradient at the taken action, g w scale with d = fl(y - t), scale = fl(1 / B): four roundings:
      <= 4 u |ref| + 2 E_t w scale
  loss: per term d (1, doubled by the square), the term (2), w (1), at most B / 16 + 15 additions
      (every wave adds its rows in increasing b, then the 16 partials are folded) and the scale (2):
      <= 2 (B + 3) u sum |w L| scale + 2 sum_b s_b E_t w_b scale
  away from the taken action the gradient is +0.0, bit for bit.

Not tested, on purpose: NaN operands, and actions outside [0, A) (the kernel reads lane
``action mod 64`` of the row it holds, so nothing outside the row is touched, but the result is
meaningless).
"""
import functools
import itertools
import os

import numpy as np
import pytest
import torch

from pfrl_amd import _native, ops
from pfrl_amd.action_value import DiscreteActionValue
from pfrl_amd.agents import dqn
from pfrl_amd.nn import mfma_trunk as mt

gpu = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
GUARD = 4096
U = 2.0 ** -24
PFRL_ERR_ARG = -2
F32 = np.float32
_p, _stream = mt._p, mt._stream

AL, PAL, DOUBLE_PAL, DPP, DPPL, DPP_GREEDY = range(6)
OPS = (AL, PAL, DOUBLE_PAL, DPP, DPPL, DPP_GREEDY)
FIXED = (AL, PAL, DOUBLE_PAL, DPP_GREEDY)          # fixed sequences of IEEE operations
OP_NAMES = ("AL", "PAL", "DoublePAL", "DPP", "DPPL", "DPPGreedy")
K_T = 6                                            # u count of the float32 target, ops 0, 1, 2, 5


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


def c_gate(B, A, op, has_next_online, param, null_operand=False):
    """PFRL_CHECK_ARG of pfrl_dqn_operator_td_loss, restated."""
    p32 = float(F32(param))
    return (B >= 1 and 1 <= A <= 64 and 0 <= op <= 5 and has_next_online == (op == 2)
            and bool(np.isfinite(p32)) and (op not in (DPP, DPPL) or p32 > 0) and not null_operand)


# ------------------------------------------------------------------ the targets, restated
def l_f32(x, eta, op):
    """The Boltzmann operators with the kernel's float32 operations and summation order (NumPy's
    exp / log stand in for the device's: this restatement is compared with float64, not bit for
    bit with the kernel)."""
    eta = F32(eta)
    z = eta * x
    m = z.max(1)
    e = np.exp(z - m[:, None])
    s = np.zeros(x.shape[0], dtype=F32)
    for a in range(x.shape[1]):
        s = s + e[:, a]
    if op == DPPL:
        out = (m + np.log(s)) / eta
    else:
        term = (e / s[:, None]) * x
        out = np.zeros(x.shape[0], dtype=F32)
        for a in range(x.shape[1]):
            out = out + term[:, a]
    assert out.dtype == F32
    return out


def t_f32(c, op, param):
    """out_t with the kernel's loads and float32 association."""
    ar = np.arange(c.B)
    a = c.action.numpy()
    tc, tn = c.tc.numpy(), c.tn.numpy()
    r = c.r.numpy()
    coef = c.disc.numpy() * (F32(1.0) - c.term.numpy())
    mc, mn = tc.max(1), tn.max(1)
    tca, tna = tc[ar, a], tn[ar, a]
    p = F32(param)
    if op in (AL, PAL, DOUBLE_PAL):
        nxt = tn[ar, c.no.numpy().argmax(1)] if op == DOUBLE_PAL else mn     # np.argmax: first maximum
        tq = r + coef * nxt
        gap = tca - mc
        if op != AL:
            gap = np.maximum(gap, tna - mn)
        t = tq + p * gap
    else:
        lc, ln = (mc, mn) if op == DPP_GREEDY else (l_f32(tc, p, op), l_f32(tn, p, op))
        ahead = r + coef * ln
        t = (tca + ahead) - lc
    assert t.dtype == F32
    return t


def l_f64(x, eta, op):
    """(L, E_L) of the docstring in float64 through the agents' own expressions."""
    A = x.shape[1]
    av = DiscreteActionValue(x)
    if op == DPP_GREEDY:
        return av.max, torch.zeros(x.shape[0], dtype=torch.float64)
    z = eta * x
    m = z.max(1, keepdim=True).values
    eps = U * (z.abs() + (z - m).abs()) + 2 * U
    epsmax = eps.max(1).values
    e = torch.exp(z - m)
    s = e.sum(1)
    eps_s = epsmax + (A - 1) * U
    if op == DPP:
        big_l = av.compute_expectation(eta)
        terms = ((e / s.unsqueeze(1)) * x).abs().sum(1)
        return big_l, (epsmax + eps_s + (A + 1) * U) * terms
    big_l = torch.logsumexp(eta * x, dim=1) / eta
    lse = m[:, 0] + torch.log(s)
    return big_l, (eps_s + 2 * U * torch.log(s).abs() + U * lse.abs()) / eta + U * big_l.abs()


def t_f64(c, op, param):
    """(t, E_t without the factor 2) in float64, the composite expression of the agents on float64
    copies of the operands, with fl32(param)."""
    p = float(F32(param))
    a = c.action
    tc, tn = DiscreteActionValue(c.tc.double()), DiscreteActionValue(c.tn.double())
    r, coef = c.r.double(), c.disc.double() * (1.0 - c.term.double())
    if op in (AL, PAL, DOUBLE_PAL):
        if op == DOUBLE_PAL:
            nxt = tn.evaluate_actions(DiscreteActionValue(c.no.double()).greedy_actions)
        else:
            nxt = tn.max
        gap, nadv = tc.compute_advantage(a), tn.compute_advantage(a)
        chosen = gap if op == AL else torch.max(gap, nadv)
        big = gap.abs() if op == AL else torch.max(gap.abs(), nadv.abs())
        t = (r + coef * nxt) + p * chosen
        return t, K_T * U * (r.abs() + (coef * nxt).abs() + abs(p) * big)
    lc, e_lc = l_f64(tc.q_values, p, op)
    ln, e_ln = l_f64(tn.q_values, p, op)
    tca = tc.evaluate_actions(a)
    ahead = r + coef * ln
    t = tca + ahead - lc
    if op == DPP_GREEDY:
        return t, K_T * U * (tca.abs() + r.abs() + (coef * ln).abs() + lc.abs())
    e_t = coef.abs() * e_ln + e_lc + 3 * U * (coef * ln).abs() + U * ahead.abs() + U * (tca + ahead).abs() + U * t.abs()
    return t, e_t


class _Ref:
    """float64 loss, gradient and |delta| through the agents' loss functions with autograd; from
    the float32 t for the fixed-sequence ops (E_t = 0), from the float64 t otherwise."""

    def __init__(self, c, op, param, clip, mean, use_w):
        B = c.B
        ar = torch.arange(B)
        if op in FIXED:
            self.t32 = t_f32(c, op, param)
            t, self.e_t = torch.from_numpy(self.t32).double(), torch.zeros(B, dtype=torch.float64)
        else:
            t, self.e_t = t_f64(c, op, param)
        q = c.q.double().requires_grad_()
        y = q[ar, c.action]
        acc = "mean" if mean else "sum"
        if use_w:
            loss = dqn.compute_weighted_value_loss(y, t, c.w.double(), clip_delta=bool(clip), batch_accumulator=acc)
        else:
            loss = dqn.compute_value_loss(y, t, clip_delta=bool(clip), batch_accumulator=acc)
        loss.backward()
        self.loss, self.grad, self.t = loss.detach(), q.grad, t
        d = (y.detach() - t)
        self.d = d
        ad = d.abs()
        row = torch.where(ad < 1, 0.5 * d * d, ad - 0.5) if clip else 0.5 * d * d
        self.wscale = (c.w.double() if use_w else torch.ones(B, dtype=torch.float64)) * (1.0 / B if mean else 1.0)
        self.sum_wl = float((self.wscale * row).abs().sum())
        self.terms = (c.w.double() if use_w else torch.ones(B, dtype=torch.float64)) * row
        slope = torch.ones(B, dtype=torch.float64) if clip else ad + self.e_t
        self.e_loss = float((slope * self.e_t * self.wscale).sum())
        self.e_d = self.e_t + U * ad


def closed_form_grad(c, r, clip):
    g = r.d.clamp(-1, 1) if clip else r.d
    out = torch.zeros(c.B, c.A, dtype=torch.float64)
    out[torch.arange(c.B), c.action] = g * r.wscale
    return out


# ------------------------------------------------------------------ operands
DELTAS = (0.0, 0.5, -0.5, 1.0, -1.0, 1.5, -1.5)


class _Case:
    def __init__(self, B, A, kind, op, param):
        self.B, self.A, self.kind, self.op, self.param = B, A, kind, op, param
        g = torch.Generator().manual_seed((B * 131 + A) * 17 + op + (1000003 if kind == "int" else 0))
        self.gen = g
        if kind == "int":
            def ri(lo, hi, *s):
                return torch.randint(lo, hi + 1, s, generator=g).float()
            self.q, self.tc, self.tn, self.no = (ri(-4, 4, B, A) for _ in range(4))
            self.r = ri(-4, 4, B) * 0.5
            self.disc = torch.tensor([0.0, 0.5, 1.0])[torch.randint(0, 3, (B,), generator=g)]
            self.term = ri(0, 1, B)
            self.w = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (B,), generator=g)]
        else:
            def rn(*s):
                return torch.randn(s, generator=g)
            self.q, self.tc, self.tn, self.no, self.r = rn(B, A), rn(B, A), rn(B, A), rn(B, A), rn(B)
            self.disc = torch.tensor(0.99) ** torch.randint(1, 4, (B,), generator=g).float()
            self.term = (torch.rand(B, generator=g) < 0.2).float()
            self.w = torch.rand(B, generator=g) + 0.5
        self.action = torch.randint(0, A, (B,), generator=g)
        self.redraws = 0
        if kind == "int" and B >= 16:
            self._plant()
        if kind == "randn" and op in (DPP, DPPL):
            self._redraw()

    def tag(self):
        return "%s-B%d-A%d-%s" % (OP_NAMES[self.op], self.B, self.A, self.kind)

    def _plant(self):
        A = self.A
        self.action[0], self.action[1] = 0, A - 1
        self.term[2] = 1.0
        if A >= 2:
            i, j = (0 if A == 2 else 1), A - 1
            # DoublePAL: an online tie at two indices with different target values, and it matters
            self.no[3] = self.no[3].clamp(max=3.0)
            self.no[3, i] = self.no[3, j] = 4.0
            self.tn[3, i], self.tn[3, j] = 2.0, -3.0
            self.disc[3], self.term[3] = 1.0, 0.0
            # a maximum tie whose first index is not the last, in both target rows
            for m in (self.tc, self.tn):
                m[4] = m[4].clamp(max=3.0)
                m[4, i] = m[4, j] = 4.0
            # PAL: gap > next_adv (and the taken action is the greedy one, gap 0), <, ==
            for row in (5, 6, 7):
                self.tc[row], self.tn[row] = 0.0, 0.0
            self.tn[5, (int(self.action[5]) + 1) % A] = 3.0
            self.tc[6, (int(self.action[6]) + 1) % A] = 3.0
        # delta = 0, +-1/2, +-1, +-1 1/2 (t does not depend on q)
        t = torch.from_numpy(t_f32(self, self.op, self.param))
        for k, dl in enumerate(DELTAS):
            self.q[8 + k, self.action[8 + k]] = t[8 + k] + dl

    def planted(self, r):
        """What the exact case holds, read off the reference."""
        kinds = set()
        A, ar = self.A, torch.arange(self.B)
        for dl in DELTAS:
            if bool((r.d == dl).any()):
                kinds.add("delta %g" % dl)
        if bool((self.term == 1).any()):
            kinds.add("terminal")
        if bool((self.action == 0).any()):
            kinds.add("action 0")
        if bool((self.action == A - 1).any()):
            kinds.add("action A-1")
        gap = self.tc[ar, self.action] - self.tc.max(1).values
        nadv = self.tn[ar, self.action] - self.tn.max(1).values
        if bool((gap == 0).any()):
            kinds.add("gap 0")
        for name, hit in (("gap > next_adv", gap > nadv), ("gap < next_adv", gap < nadv), ("gap == next_adv", gap == nadv)):
            if bool(hit.any()):
                kinds.add(name)
        live = self.disc * (1 - self.term) != 0
        for name, m in (("target tie", self.tn), ("online tie", self.no)):
            hit = m == m.max(1, keepdim=True).values
            first = hit.float().argmax(1)
            last = (A - 1) - hit.flip(1).float().argmax(1)
            tie = (hit.sum(1) >= 2) & (first < A - 1)
            if name == "online tie":
                tie = tie & (self.tn[ar, first] != self.tn[ar, last]) & live
            if bool(tie.any()):
                kinds.add(name)
        return kinds

    def _near_branch(self):
        t, e_t = t_f64(self, self.op, self.param)
        d = self.q.double()[torch.arange(self.B), self.action] - t
        return ((d.abs() - 1).abs() <= 2 * (e_t + U * d.abs()))

    def _redraw(self):
        for _ in range(100):
            rows = self._near_branch()
            if not bool(rows.any()):
                break
            k = int(rows.sum())
            self.r[rows] = torch.randn(k, generator=self.gen)
            self.redraws += k
        assert not bool(self._near_branch().any())


@functools.lru_cache(maxsize=4)
def _case(B, A, kind, op, param):
    return _Case(B, A, kind, op, param)


def _to_dev(c, dev):
    return {k: getattr(c, k).to(dev).contiguous() for k in ("q", "tc", "tn", "no", "action", "r", "disc", "term", "w")}


def _launch(c, dev, op, param, clip, mean, use_w, want_t=True, d=None):
    d = d if d is not None else _to_dev(c, dev)
    out = {"loss": _Guarded(1, dev), "grad": _Guarded(c.B * c.A, dev), "y": _Guarded(c.B, dev),
           "delta": _Guarded(c.B, dev), "t": _Guarded(c.B, dev)}
    mt.check(_native.lib().pfrl_dqn_operator_td_loss(
        _p(d["q"]), _p(d["tc"]), _p(d["tn"]), _p(d["no"]) if op == DOUBLE_PAL else None, _p(d["action"]),
        _p(d["r"]), _p(d["disc"]), _p(d["term"]), _p(d["w"]) if use_w else None, c.B, c.A, op, float(param),
        int(clip), int(mean), _p(out["loss"].t), _p(out["grad"].t), _p(out["y"].t), _p(out["delta"].t),
        _p(out["t"].t) if want_t else None, _stream()), "operator td loss")
    torch.cuda.synchronize()
    if not want_t:
        out.pop("t").untouched("out_t = NULL")
    return {k: v.done(k).cpu() for k, v in out.items()}


def _bits(t):
    return t.contiguous().view(torch.int32)


def _off_action_is_plus_zero(c, grad):
    bits = _bits(grad).view(c.B, c.A).clone()
    bits[torch.arange(c.B), c.action] = 0
    return not bool(bits.any())


# ================================================================== shapes
R_B = [1, 2, 63, 64, 255, 256, 257, 1000, 4096]
R_A = [1, 2, 6, 18, 63, 64]
ALWAYS = (4096, 64)
SWITCHES = list(itertools.product((0, 1), (0, 1), (0, 1)))       # clip_delta, mean, weights


def _switches(B, A, op):
    """The third of the switch settings a (B, A, op) runs: index sum % 3 == 0; all at (4096, 64)."""
    if (B, A) == ALWAYS:
        return list(SWITCHES)
    i, j = R_B.index(B), R_A.index(A)
    return [s for s in SWITCHES if (i + j + op + sum(s)) % 3 == 0]


def _launches():
    return [(B, A, op, s) for B in R_B for A in R_A for op in OPS for s in _switches(B, A, op)]


SHAPES = [(B, A, op) for B in R_B for A in R_A for op in OPS]


def _params(B, A, op, kind):
    """alpha / eta of a case: alpha in {1/2, 1/4} on exact operands."""
    odd = (R_B.index(B) + R_A.index(A)) % 2
    if op in (DPP, DPPL):
        return (0.5, 2.0)
    if op == DPP_GREEDY:
        return (0.0,)
    return ((0.25 if odd else 0.5),) if kind == "int" else ((0.8 if odd else 0.9),)


def _pow2(n):
    return n & (n - 1) == 0


# ================================================================== no GPU
def test_the_chosen_third_reaches_every_listed_size():
    chosen = _launches()
    full = len(R_B) * len(R_A) * len(OPS) * len(SWITCHES)
    assert len(chosen) <= full // 3 + len(OPS) * len(SWITCHES)
    for op in OPS:
        mine = [l for l in chosen if l[2] == op]
        assert {l[0] for l in mine} == set(R_B) and {l[1] for l in mine} == set(R_A)
        assert {l[3] for l in mine if l[:2] == ALWAYS} == set(SWITCHES)
        for axis in range(3):
            assert {l[3][axis] for l in mine} == {0, 1}
    assert all(_switches(*s) for s in SHAPES)
    assert all(c_gate(B, A, op, op == DOUBLE_PAL, _params(B, A, op, "randn")[0] or 0.0) for B, A, op in SHAPES)
    # every exact case of >= 16 rows holds the planted rows; mean is exact at a power-of-two B
    assert sum(1 for B in R_B if _pow2(B) and B >= 16) >= 3


class _FakeTensor:
    def __init__(self, *shape, cuda=True, dtype=torch.float32, contiguous=True):
        self.shape, self.ndim, self.is_cuda, self.dtype, self._c = tuple(shape), len(shape), cuda, dtype, contiguous

    def is_contiguous(self):
        return self._c


def test_python_gate_admits_only_what_the_c_gate_admits():
    n = 0
    for B, A, op, with_no, param in itertools.product((0, 1, 4096, 10 ** 6), (0, 1, 64, 65), (-1,) + OPS + (6,),
                                                      (False, True), (0.9, 0.0, -1.0, float("inf"), float("nan"), 1e-60)):
        ts = [_FakeTensor(B, A)] * (4 if with_no else 3)
        if ops.dqn_operator_td_loss_supported(*ts, op=op, param=param) and with_no == (op == DOUBLE_PAL):
            n += 1
            assert c_gate(B, A, op, with_no, param), (B, A, op, with_no, param)
    assert n > 0
    ok = _FakeTensor(32, 18)
    assert ops.dqn_operator_td_loss_supported(ok, ok, ok, None, op="DPP", param=2.0)
    assert ops.dqn_operator_td_loss_supported(ok, ok, ok, ok, op="DoublePAL", param=0.9)
    assert not ops.dqn_operator_td_loss_supported(ok, ok, ok, op="DPP", param=0.0)
    assert not ops.dqn_operator_td_loss_supported(ok, ok, ok, op="DPPL", param=1e-60)        # fl32 -> 0
    assert not ops.dqn_operator_td_loss_supported(ok, ok, ok, op="AL", param=float("nan"))
    assert not ops.dqn_operator_td_loss_supported(ok, ok, ok, op="Expected", param=1.0)
    assert not ops.dqn_operator_td_loss_supported(_FakeTensor(32, 18, cuda=False), ok, ok)
    assert not ops.dqn_operator_td_loss_supported(ok, _FakeTensor(32, 18, dtype=torch.float64), ok)
    assert not ops.dqn_operator_td_loss_supported(ok, ok, _FakeTensor(32, 18, contiguous=False))
    assert not ops.dqn_operator_td_loss_supported(ok, ok, _FakeTensor(32, 17))
    assert not ops.dqn_operator_td_loss_supported(_FakeTensor(32, 18, 51), ok, ok)
    assert not ops.dqn_operator_td_loss_supported(*[_FakeTensor(32, 65)] * 3)
    assert set(ops.OPERATOR_TD_OPS) == set(OP_NAMES) and [ops.OPERATOR_TD_OPS[n] for n in OP_NAMES] == list(OPS)


@pytest.mark.parametrize("op", OPS, ids=OP_NAMES)
@pytest.mark.parametrize("shape", [(257, 18), (63, 64), (1000, 2), (64, 1)], ids=lambda s: "B%d-A%d" % s)
def test_float32_targets_are_what_float64_computes(op, shape):
    """The float32 restatement of every target against the float64 composite expression: within
    K_T u mag for the fixed sequences, within 2 E_t for the Boltzmann operators."""
    for param in _params(shape[0], shape[1], op, "randn"):
        c = _Case(*shape, "randn", op, param)
        t64, e_t = t_f64(c, op, param)
        err = (torch.from_numpy(t_f32(c, op, param)).double() - t64).abs()
        bound = e_t if op in FIXED else 2 * e_t
        assert bool((err <= bound).all()), float((err / bound).max())


@pytest.mark.parametrize("op", FIXED, ids=[OP_NAMES[o] for o in FIXED])
def test_closed_form_gradient_is_float64_autograds(op):
    """g w scale at the taken action, g = clamp(d, -1, 1) (Huber) or d (squared), against float64
    autograd through the agents' loss functions on the exact operands: difference 0.0."""
    c = _case(64, 6, "int", op, 0.5)
    for clip, mean, use_w in SWITCHES:
        r = _Ref(c, op, 0.5, clip, mean, use_w)
        assert torch.equal(closed_form_grad(c, r, clip), r.grad)
        need = {"delta %g" % d for d in DELTAS} | {"terminal", "action 0", "action A-1", "gap 0", "gap > next_adv",
                                                   "gap < next_adv", "gap == next_adv", "target tie", "online tie"}
        assert not need - c.planted(r), need - c.planted(r)


def test_host_agents_never_touch_the_fused_route(monkeypatch):
    """gpu=None: the predicate is False, the launch is never asked for, the teacher-forced losses
    hold at 1e-5 on the composite expression."""
    def boom(*a, **k):
        raise AssertionError("the fused route was taken on the host")

    monkeypatch.setattr(ops, "dqn_operator_td_loss", boom)
    monkeypatch.setattr(dqn.DQN, "_compute_loss_fused_operator", boom)
    for name, cls, kw in FAMILY:
        ag = _tf_agent(name, cls, kw, gpu=None)
        assert ag.fused_td_loss and not ag._fused_operator_loss_applicable()
        assert not ag._fused_td_loss_applicable()
        for k in (1, 50, 140):
            loss = ag._compute_loss(_tf_state(ag, name, k), errors_out=None)[0]
            want = float(_golden(name)["u%d_loss" % k])
            assert abs(float(loss.detach()) - want) <= 1e-5 * max(1.0, abs(want)), (name, k)


def test_export_header_and_integration_agree():
    name = "pfrl_dqn_operator_td_loss"
    assert name in _native.EXPORTS and "operator_td.hip" in _native.SOURCES
    header = open(os.path.join(ROOT, "include", "pfrl_amd.h")).read()
    assert "int %s(" % name in header
    for cite in ("pfrl/agents/al.py", "pal.py", "double_pal.py", "pfrl/agents/dpp.py:19-83,99-127", "pfrl/agents/dqn.py",
                 "pfrl/action_value.py:60-79"):
        assert cite in header, cite
    assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert len(_native.EXPORTS[name][1]) == 21


def test_family_is_the_one_of_the_traces():
    from test_agent_parity import DQN_FAMILY

    assert FAMILY == DQN_FAMILY
    assert [ops.OPERATOR_TD_OPS[cls] for _, cls, _ in FAMILY] == list(OPS)


# ================================================================== kernel, GPU
def _check_fixed(c, dev, op, param, switches):
    """Bit for bit t, y, |delta| and +0.0 off the action; on exact operands loss and gradient
    ``torch.equal``, on randn within the rounded bounds."""
    d = _to_dev(c, dev)
    ar = torch.arange(c.B)
    for clip, mean, use_w in switches:
        r = _Ref(c, op, param, clip, mean, use_w)
        got = _launch(c, dev, op, param, clip, mean, use_w, d=d)
        tag = "%s p%g clip%d mean%d w%d" % (c.tag(), param, clip, mean, use_w)
        t32 = torch.from_numpy(r.t32)
        assert torch.equal(_bits(got["t"]), _bits(t32)), tag
        assert torch.equal(_bits(got["y"]), _bits(c.q[ar, c.action])), tag
        assert torch.equal(_bits(got["delta"]), _bits((c.q[ar, c.action] - t32).abs())), tag
        assert _off_action_is_plus_zero(c, got["grad"]), tag
        grad = got["grad"].view(c.B, c.A)
        if c.kind == "int":
            total = float(r.terms.abs().sum())
            assert total < 2 ** 20 and 64 * total < 2 ** 24, total
            if c.B >= 16 and c.A >= 2:
                need = {"delta %g" % x for x in DELTAS} | {"terminal", "action 0", "action A-1", "gap 0", "gap > next_adv",
                                                           "gap < next_adv", "gap == next_adv", "target tie", "online tie"}
                assert not need - c.planted(r), (tag, need - c.planted(r))
            if not mean or _pow2(c.B):
                assert torch.equal(got["loss"].double().view(()), r.loss), tag
                assert torch.equal(grad.double(), r.grad), tag
                continue
        _within("operator_td grad fixed", tag, grad[ar, c.action], r.grad[ar, c.action], 4 * U * r.grad[ar, c.action].abs())
        _within("operator_td loss fixed", tag, got["loss"].view(()), r.loss,
                torch.tensor(2 * (c.B + 3) * U * r.sum_wl, dtype=torch.float64))


def _check_boltzmann(c, dev, op, param, switches):
    d = _to_dev(c, dev)
    ar = torch.arange(c.B)
    name = "operator_td %s" % OP_NAMES[op]
    for clip, mean, use_w in switches:
        r = _Ref(c, op, param, clip, mean, use_w)
        got = _launch(c, dev, op, param, clip, mean, use_w, d=d)
        tag = "%s eta%g clip%d mean%d w%d redrawn %d" % (c.tag(), param, clip, mean, use_w, c.redraws)
        assert torch.equal(_bits(got["y"]), _bits(c.q[ar, c.action])), tag
        assert _off_action_is_plus_zero(c, got["grad"]), tag
        _within(name + " t", tag, got["t"], r.t, 2 * r.e_t)
        _within(name + " delta", tag, got["delta"], r.d.abs(), 2 * r.e_d)
        ref_g = r.grad[ar, c.action]
        _within(name + " grad", tag, got["grad"].view(c.B, c.A)[ar, c.action], ref_g,
                4 * U * ref_g.abs() + 2 * r.e_t * r.wscale)
        _within(name + " loss", tag, got["loss"].view(()), r.loss,
                torch.tensor(2 * (c.B + 3) * U * r.sum_wl + 2 * r.e_loss, dtype=torch.float64))


@gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d-A%d-%s" % (s[0], s[1], OP_NAMES[s[2]]))
def test_operator_td_loss_over_the_envelope(shape):
    """The chosen third of B x A x op x clip_delta x mean x weights (all switches at (4096, 64)):
    ops 0, 1, 2, 5 on exact and on randn operands, ops 3 and 4 on randn with eta 0.5 and 2."""
    dev = _dev()
    B, A, op = shape
    sw = _switches(B, A, op)
    if op in FIXED:
        for kind in ("int", "randn"):
            param = _params(B, A, op, kind)[0]
            _check_fixed(_case(B, A, kind, op, param), dev, op, param, sw)
    else:
        for eta in _params(B, A, op, "randn"):
            _check_boltzmann(_case(B, A, "randn", op, eta), dev, op, eta, sw)


@gpu
@pytest.mark.parametrize("eta", [0.5, 2.0])
@pytest.mark.parametrize("op", [DPP, DPPL], ids=["DPP", "DPPL"])
def test_one_action_makes_the_boltzmann_operators_the_greedy_one(op, eta):
    """A = 1: softmax = 1 and logsumexp(eta x) / eta = x exactly (eta a power of two), so t equals
    DPPGreedy's bit for bit, and with it |delta|, loss and gradient."""
    dev = _dev()
    c = _Case(257, 1, "randn", DPP_GREEDY, 0.0)
    d = _to_dev(c, dev)
    want = _launch(c, dev, DPP_GREEDY, 0.0, 1, 0, 1, d=d)
    got = _launch(c, dev, op, eta, 1, 0, 1, d=d)
    assert torch.equal(_bits(want["t"]), _bits(torch.from_numpy(t_f32(c, DPP_GREEDY, 0.0))))
    for k in want:
        assert torch.equal(_bits(got[k]), _bits(want[k])), k


@gpu
@pytest.mark.parametrize("eta", [0.5, 2.0])
@pytest.mark.parametrize("A", [2, 64])
def test_dpp_on_rows_constant_over_the_actions_gives_the_constant(A, eta):
    """Q'(s) and Q'(s') constant over the actions (multiples of 1/2): every softmax weight is
    exactly 1 / A and the sum over increasing a of q / A is exact, L = q: t equals DPPGreedy's
    (whose L is the maximum, q) bit for bit."""
    dev = _dev()
    c = _Case(67, A, "int", DPP_GREEDY, 0.0)
    c.tc = (c.tc[:, :1] * 0.5).expand(-1, A).contiguous()
    c.tn = (c.tn[:, :1] * 0.5).expand(-1, A).contiguous()
    d = _to_dev(c, dev)
    want = _launch(c, dev, DPP_GREEDY, 0.0, 0, 0, 0, d=d)
    got = _launch(c, dev, DPP, eta, 0, 0, 0, d=d)
    assert torch.equal(_bits(want["t"]), _bits(torch.from_numpy(t_f32(c, DPP_GREEDY, 0.0))))
    for k in want:
        assert torch.equal(_bits(got[k]), _bits(want[k])), k


@gpu
@pytest.mark.parametrize("op", OPS, ids=OP_NAMES)
def test_operator_td_loss_is_deterministic(op):
    dev = _dev()
    param = _params(257, 18, op, "randn")[-1]
    c = _case(257, 18, "randn", op, param)
    d = _to_dev(c, dev)
    one, two = _launch(c, dev, op, param, 1, 1, 1, d=d), _launch(c, dev, op, param, 1, 1, 1, d=d)
    for k in one:
        assert torch.equal(_bits(one[k]), _bits(two[k])), k


@gpu
def test_operator_td_loss_refuses_what_its_gate_refuses():
    dev = _dev()
    lib = _native.lib()
    c = _Case(4, 3, "randn", PAL, 0.8)
    d = _to_dev(c, dev)
    out = _Guarded(1 << 16, dev)
    o = _p(out.t)
    operands = ["q", "tc", "tn", "no", "action", "r", "disc", "term", "w"]

    def call(B=4, A=3, op=PAL, param=0.8, null=(), with_no=None, outs=(o, o, o, o, o)):
        with_no = (op == DOUBLE_PAL) if with_no is None else with_no
        ptrs = [None if k in null or (k == "no" and not with_no) else _p(d[k]) for k in operands]
        return lib.pfrl_dqn_operator_td_loss(*ptrs, B, A, op, float(param), 1, 1, *outs, _stream())

    rcs = {"B = 0": call(B=0), "A = 0": call(A=0), "A = 65": call(A=65), "op = -1": call(op=-1), "op = 6": call(op=6),
           "op 2 without next_online": call(op=DOUBLE_PAL, with_no=False),
           "op 0 with next_online": call(op=AL, with_no=True),
           "eta = 0": call(op=DPP, param=0.0), "eta < 0": call(op=DPPL, param=-1.0),
           "eta nan": call(op=DPP, param=float("nan")), "alpha inf": call(op=AL, param=float("inf"))}
    for k in ("q", "tc", "tn", "action", "r", "disc", "term"):
        rcs["%s = NULL" % k] = call(null=(k,))
    for i in range(4):
        rcs["output %d = NULL" % i] = call(outs=tuple(None if j == i else o for j in range(5)))
    assert all(rc == PFRL_ERR_ARG for rc in rcs.values()), rcs
    torch.cuda.synchronize()
    out.untouched("an output of a refused call")
    # the two optional pointers
    full = _launch(c, dev, PAL, 0.8, 1, 0, True, d=d)
    no_w, no_t = _launch(c, dev, PAL, 0.8, 1, 0, False, d=d), _launch(c, dev, PAL, 0.8, 1, 0, True, want_t=False, d=d)
    r = _Ref(c, PAL, 0.8, 1, 0, False)
    assert abs(float(no_w["loss"]) - float(r.loss)) <= 2 * (c.B + 3) * U * r.sum_wl
    for k in ("loss", "grad", "y", "delta"):
        assert torch.equal(_bits(no_t[k]), _bits(full[k])), k
    # a non-positive alpha is an operand like any other
    assert call(op=AL, param=-0.5) == 0 and call(op=DPP_GREEDY, param=-1.0) == 0
    torch.cuda.synchronize()


@gpu
@pytest.mark.parametrize("op", [DOUBLE_PAL, DPP], ids=["DoublePAL", "DPP"])
def test_autograd_wrapper_hands_back_the_kernels_gradient(op):
    dev = _dev()
    param = 0.9 if op == DOUBLE_PAL else 2.0
    c = _case(33, 6, "randn", op, param)
    d = _to_dev(c, dev)
    raw = _launch(c, dev, op, param, 1, 1, 1, d=d)
    want = raw["grad"].view(c.B, c.A)
    for scale in (1.0, 3.0):
        q = d["q"].clone().requires_grad_()
        loss, y, delta = ops.dqn_operator_td_loss(q, d["tc"], d["tn"], d["no"] if op == DOUBLE_PAL else None, d["action"],
                                                  d["r"], d["disc"], d["term"], d["w"], op, param, True, True)
        assert loss.shape == () and y.shape == delta.shape == (c.B,)
        assert not y.requires_grad and not delta.requires_grad
        assert torch.equal(y.cpu(), raw["y"]) and torch.equal(delta.cpu(), raw["delta"])
        (loss * scale).backward()
        assert torch.equal(q.grad.cpu(), want * torch.tensor(scale))


# ================================================================== agents
FAMILY = [("al", "AL", dict(alpha=0.9)), ("pal", "PAL", dict(alpha=0.8)),
          ("double_pal", "DoublePAL", dict(alpha=0.9)), ("dpp", "DPP", dict(eta=2.0)),
          ("dppl", "DPPL", dict(eta=0.5)), ("dpp_greedy", "DPPGreedy", dict())]
FAMILY_IDS = [f[0] for f in FAMILY]


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


KERNEL = "pfrl_dqn_operator_td_loss"


def _tf_agent(name, cls, kw, gpu=0, base=None, n_actions=6, **agent_kw):
    """The agent of test_agent_parity._run (the configuration the fixtures were recorded with)."""
    from pfrl_amd import agents, explorers, replay_buffers
    from pfrl_amd.q_functions import DiscreteActionValueHead

    def phi(x):
        return np.asarray(x, dtype=np.float32) / 255

    q = torch.nn.Sequential(torch.nn.Flatten(), torch.nn.Linear(4 * 144, 32), torch.nn.ReLU(),
                            torch.nn.Linear(32, n_actions), DiscreteActionValueHead())
    opt = torch.optim.RMSprop(q.parameters(), lr=2.5e-4, alpha=0.95, eps=1e-2)
    rbuf = replay_buffers.ReplayBuffer(200, num_steps=1)
    ex = explorers.LinearDecayEpsilonGreedy(1.0, 0.1, 400, lambda: np.random.randint(6))
    if gpu is not None:
        agent_kw.setdefault("use_graphs", False)
    return (base or getattr(agents, cls))(q, opt, rbuf, 0.99, ex, gpu=gpu, replay_start_size=40, minibatch_size=8,
                                          update_interval=4, target_update_interval=60, phi=phi,
                                          batch_accumulator="sum", **dict(kw, **agent_kw))


@functools.lru_cache(maxsize=None)
def _golden(name):
    return np.load(os.path.join(GOLDEN, "teacher_forced_%s.npz" % name))


def _tf_state(ag, name, k):
    """Parameters and minibatch of update k of the recorded run, on the agent."""
    from test_teacher_forced_loss import _load_flat

    g = _golden(name)
    _load_flat(ag.model, g["u%d_params" % k])
    _load_flat(ag.target_model, g["u%d_target_params" % k])
    return _tf_batch(ag, name, k)


def _tf_batch(ag, name, k):
    g = _golden(name)
    batch = {}
    for key in ("state", "action", "reward", "next_state", "is_state_terminal", "discount"):
        a = g["u%d_%s" % (k, key)]
        if key in ("state", "next_state"):
            a = a.astype(np.float32) / 255
        batch[key] = torch.as_tensor(a).to(ag.device)
    return batch


@gpu
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "composite"])
@pytest.mark.parametrize("name,cls,kw", FAMILY, ids=FAMILY_IDS)
def test_teacher_forced_losses_take_the_expected_route(name, cls, kw, fused, recorder):
    """The recorded losses of updates 1, 50 and 140 at 1e-5, through pfrl_dqn_operator_td_loss
    exactly once per evaluation with ``fused_td_loss=True`` and not at all with False;
    ``_fused_td_loss_applicable`` stays False on both."""
    ag = _tf_agent(name, cls, kw, fused_td_loss=fused)
    assert ag._fused_operator_loss_applicable() == fused and not ag._fused_td_loss_applicable()
    for k in (1, 50, 140):
        batch = _tf_state(ag, name, k)
        del recorder.calls[:]
        errors = []
        loss, delta = ag._compute_loss(batch, errors_out=errors)
        assert recorder.calls.count(KERNEL) == (1 if fused else 0)
        assert "pfrl_dqn_td_loss" not in recorder.calls and "pfrl_dqn_head_td_loss" not in recorder.calls
        assert not ag._fused_td_loss_applicable()
        want, got = float(_golden(name)["u%d_loss" % k]), float(loss.detach().cpu())
        print("TEACHER FORCED %s update %d %s: %.9g (reference %.9g)" % (name, k, "fused" if fused else "composite", got, want))
        assert abs(got - want) <= 1e-5 * max(1.0, abs(want)), (name, k, got, want)
        assert len(errors) == 8 and np.allclose(errors, delta.cpu().numpy())
        assert ag._last_y.reshape(-1).shape == (8,)


def _overriding(base, method):
    def same(self, *a, **k):
        return getattr(super(sub, self), method)(*a, **k)

    sub = type("Own" + method, (base,), {method: same})
    return sub


@gpu
@pytest.mark.parametrize("name,cls,kw", FAMILY, ids=FAMILY_IDS)
def test_a_subclass_with_its_own_operator_keeps_the_composite_route(name, cls, kw, recorder):
    from pfrl_amd import agents

    base = getattr(agents, cls)
    own = "_gap_term" if cls in ("AL", "PAL", "DoublePAL") else "_l_operator"
    for method in (own, "_compute_target_values"):
        ag = _tf_agent(name, cls, kw, base=_overriding(base, method))
        assert ag.fused_td_loss and not ag._fused_operator_loss_applicable() and not ag._fused_td_loss_applicable()
        batch = _tf_state(ag, name, 50)
        del recorder.calls[:]
        loss = ag._compute_loss(batch, errors_out=None)[0]
        assert KERNEL not in recorder.calls
        want = float(_golden(name)["u50_loss"])
        assert abs(float(loss.detach().cpu()) - want) <= 1e-5 * max(1.0, abs(want))
    # a subclass that overrides nothing keeps the fused route of its family
    plain = type("Plain", (base,), {})
    ag = _tf_agent(name, cls, kw, base=plain)
    assert ag._fused_operator_loss_applicable()
    del recorder.calls[:]
    ag._compute_loss(_tf_state(ag, name, 50), errors_out=None)
    assert recorder.calls.count(KERNEL) == 1


@gpu
@pytest.mark.parametrize("name,cls,kw", [FAMILY[2], FAMILY[4]], ids=["double_pal", "dppl"])
def test_outside_the_gate_the_fused_route_finishes_on_the_composite_expression(name, cls, kw, recorder):
    """65 actions: the predicate holds, ``ops.dqn_operator_td_loss_supported`` does not; the launch
    is not made and loss and TD errors are the composite route's on the same parameters and
    minibatch (the same stock-PyTorch expression on the same passes)."""
    fused = _tf_agent(name, cls, kw, n_actions=65)
    plain = _tf_agent(name, cls, kw, n_actions=65, fused_td_loss=False)
    plain.model.load_state_dict(fused.model.state_dict())
    for ag in (fused, plain):
        ag.target_model.load_state_dict(fused.model.state_dict())
    assert fused._fused_operator_loss_applicable() and not plain._fused_operator_loss_applicable()
    batch = _tf_batch(fused, name, 50)
    out = {}
    for ag in (fused, plain):
        errors = []
        loss = ag._compute_loss(batch, errors_out=errors)[0]
        out[ag is fused] = (float(loss.detach().cpu()), np.asarray(errors))
    assert KERNEL not in recorder.calls
    assert abs(out[True][0] - out[False][0]) <= 1e-6 * max(1.0, abs(out[False][0]))
    np.testing.assert_allclose(out[True][1], out[False][1], rtol=1e-6, atol=1e-7)


def _float64_gradients(name, cls, kw, k):
    """The composite expression on a float64 CPU replica of the model, same state."""
    ag = _tf_agent(name, cls, kw, gpu=None)
    batch = _tf_state(ag, name, k)
    ag.model.double()
    ag.target_model.double()
    b = {key: (v.double() if v.is_floating_point() else v) for key, v in batch.items()}
    y, t = ag._compute_y_and_t(b)
    dqn.compute_value_loss(y, t, clip_delta=True, batch_accumulator="sum").backward()
    return [p.grad for p in ag.model.parameters()]


@gpu
@pytest.mark.parametrize("name,cls,kw", FAMILY, ids=FAMILY_IDS)
def test_fused_route_gradients_are_as_close_to_float64_as_the_composite_routes(name, cls, kw):
    """Every parameter's gradient after ``backward`` on both routes against a float64 CPU replica of
    the model on the same state.  Both routes are float32 evaluations of one expression: the fused
    route's largest error may be at most 4 times the composite route's, with floor 8 u max |ref|."""
    for k in (1, 50, 140):
        ref = _float64_gradients(name, cls, kw, k)
        errs = {}
        for fused in (True, False):
            ag = _tf_agent(name, cls, kw, fused_td_loss=fused)
            batch = _tf_state(ag, name, k)
            ag.model.zero_grad()
            ag._compute_loss(batch, errors_out=None)[0].backward()
            errs[fused] = max(float((p.grad.cpu().double() - r).abs().max()) for p, r in zip(ag.model.parameters(), ref))
        top = max(float(r.abs().max()) for r in ref)
        print("OPERATOR GRADIENT ERROR %s update %d: fused %.3e composite %.3e max|ref| %.3e"
              % (name, k, errs[True], errs[False], top))
        assert errs[True] <= max(4 * errs[False], 8 * U * top), (name, k, errs, top)


def _train(name, cls, kw, steps, prioritized=False, num_steps=1, **agent_kw):
    from test_agent_parity import _run

    return _run(name, prioritized, num_steps, False, gpu=0, agent_cls=cls, steps=steps, **dict(kw, **agent_kw))


@gpu
@pytest.mark.parametrize("name,cls,kw", FAMILY, ids=FAMILY_IDS)
def test_captured_fused_update_equals_the_eager_one(name, cls, kw, recorder):
    """Both fused: the captured update holds the kernel (seen by the proxy while capturing) and
    trains like the eager one: equal actions, losses and parameters within 1e-5."""
    eager = _train(name, cls, kw, 320, use_graphs=False)
    n_eager = recorder.calls.count(KERNEL)
    assert n_eager == len(eager["losses"]) > 20
    del recorder.calls[:]
    graph = _train(name, cls, kw, 320)
    assert graph["agent"].use_graphs and graph["agent"]._graphed is not None
    assert 1 <= recorder.calls.count(KERNEL) < n_eager             # captured, then replayed
    assert len(graph["losses"]) == len(eager["losses"])
    np.testing.assert_array_equal(graph["actions"], eager["actions"])
    np.testing.assert_allclose(graph["losses"], eager["losses"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(graph["final_params"], eager["final_params"], rtol=1e-5, atol=1e-5)


@gpu
@pytest.mark.parametrize("name,cls,kw", [FAMILY[1], FAMILY[3]], ids=["pal", "dpp"])
def test_whole_run_with_prioritized_n_step_replay_fused_equals_composite(name, cls, kw, recorder):
    """train_agent_batch with PER and 3-step returns: the fused and the composite route take equal
    actions over the first 40 updates and their losses agree within 1e-5 there."""
    runs = {}
    for fused in (True, False):
        del recorder.calls[:]
        runs[fused] = _train(name, cls, kw, 240, prioritized=True, num_steps=3, fused_td_loss=fused)
        assert (recorder.calls.count(KERNEL) > 0) == fused
        assert len(runs[fused]["losses"]) >= 40
    np.testing.assert_array_equal(runs[True]["actions"], runs[False]["actions"])
    np.testing.assert_allclose(runs[True]["losses"][:40], runs[False]["losses"][:40], rtol=1e-5, atol=1e-5)
