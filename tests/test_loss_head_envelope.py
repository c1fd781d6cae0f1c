"""The kernels that turn action values into a loss and a gradient -- csrc/tdloss.hip
(``pfrl_dqn_td_loss``, ``pfrl_dqn_head_td_loss``), csrc/c51.hip (``pfrl_c51_loss``), csrc/dueling.hip
(``pfrl_dueling_softmax_fwd/_bwd``) and ``k_dqn_act_head`` of csrc/qnet.hip -- over what their gates
admit, through the C ABI, against ``torch.float64`` / NumPy on the CPU.  The method of
tests/test_linear_envelope.py: (a) exact on operands chosen so that every intermediate is
representable (``torch.equal``), (b) rounded on randn operands within a bound derived below, with
``RATIO`` lines per case and ``MAX RATIO <entry>`` lines after the last test (``pytest -s``).  Every
output and slab buffer lies between two NaN guard zones of 4096 floats that must still be NaN after
the launch, and the payload must hold no NaN.

u = 2^-24 throughout.  Every bound carries a factor 2 over its first-order derivation.

1. ``pfrl_dqn_td_loss``.  y = q[b][a_b] is a load; t = r + (disc (1 - term)) next and d = y - t are
   IEEE operations in a fixed association, so y and |d| are compared bit for bit with the same
   float32 expression on the CPU, on integer AND randn operands.  Given d, the float64 reference is
   the header's expression.  g w scale is three roundings (g w, then scale, scale = 1 / B itself
   rounded): |err| <= 4 u |ref|.  A loss term is at most two roundings, times w one more, the sum over
   B rows B - 1, the final scale two: |err| <= 2 (B + 3) u sum_b |w_b L_b|.
   Exact operands: q, target_q, next_q_online integers in -4..4, reward multiples of 0.5, discount in
   {0, 0.5, 1}, terminal in {0, 1}, weights in {0.5, 1, 2}: d is a multiple of 1/2, every loss term a
   multiple of 1/16 (1/8 times the weight 1/2), so sums below 2^20 are exact; the case asserts both.

2. ``pfrl_dqn_head_td_loss``.  y = h[m] . W[a] + b[a] is a sum of K products in the kernel's own order:
       E_y = (K + 2) u sum_k |h w| + u |b|.
   t is fixed bit for bit by its operands (as in 1), so the reference takes the float32 t and
       E_d = E_y + u |d|                                   (the subtraction rounds once).
   Huber: L' = clamp(d, -1, 1) and g = clamp(d, -1, 1) are continuous at |d| = 1 with slope <= 1;
   quadratic: L' = d, g = d.  With L'max = min(|d| + E_d, 1) resp. |d| + E_d:
       E_L = L'max E_d + 2 u L,    E_g = E_d,
       E_gq = (E_g + 3 u |g|) w scale,        E_lt = (E_L + 3 u L) w scale,
       dh:  (E_gq + u |gq|) |W[a]|,
       slab dW: sum over the slab's rows of (E_gq + 4 u |gq|) |h|   (one product, three additions),
       slab db: sum of (E_gq + 3 u |gq|),   slab loss: sum of (E_lt + 3 u lt),
   the totals the sums of the slab bounds, the fold launch (S + 1) u sum |terms| on top.
   Rows whose |d| lies within 2 E_d of the Huber branch point get a new reward until none is left;
   the case asserts on the reference that none is, and no row is skipped.

3. ``pfrl_c51_loss``.  scale, Tz, both clamps, bj, floor, frac, wl, wu are IEEE operations and the
   projection a gather in increasing j (lower contribution, then upper), so t is reproduced bit for
   bit by a float32 loop on the CPU.  It is read out of the kernel through the gradient: with
   power-of-two entries in the taken row, no weights and mean = 0, grad = -t / y exactly.
   Given t:  delta = sum_z -t log(yc): the product rounds once, the sum Z - 1 times, and the
   device ``logf`` is ASSUMED accurate to 1 ulp (2 u relative; no accuracy table of the device math
   library is installed next to the compiler, so this is the stated assumption):
       E_delta = (Z + 4) u sum_z |t log yc|,    E_q = (Z + 2) u sum_z |y z|,
       E_loss = sum_b E_delta |coef| + (B + 3) u sum_b |delta coef|,
       gradient -t / yc coef with coef = w / B: four roundings, 4 u |ref| (8 u with the factor 2).
   The greedy action: on the float64 reference the best and second-best sum_z p z of every row differ
   by more than 2 (Z + 2) u sum_z |p z| (rows that do not are redrawn; asserted), except rows built
   as exact ties -- two actions with the identical ``next_select`` row and different ``next_dist``
   rows -- where the first must win.

4. ``pfrl_dueling_softmax``.  x = (ya - mean) + ys with mean = (sum_a ya) / A:
       E_x = u (A mean|ya| + 3 (|ya| + mean|ya| + |ys|))
   (the A - 1 additions and the division of the mean, then three roundings on the operands' sizes).
   With m the row maximum, eps_z = E_x + u |x_z - m| (the subtraction; the softmax does not depend on
   m itself), ``expf`` assumed 1 ulp, the sum Z - 1 roundings and the division one:
       |dq_z| <= q_z (eps_z + sum_z' q_z' eps_z' + (Z + 4) u)  + 2^-126
   (the last term: results below the smallest normal float may be flushed).
   Backward from the kernel's own q:  gl = q (g - sum_z g q):
       E_gl = (Z + 3) u q (|g| + sum_z |g q|) =: (Z + 3) u G,
       g_ys = sum_a gl:  (Z + A + 2) u sum_a G,
       g_ya = gl - g_ys / A:  (Z + 4) u G + (Z + A + 4) u (sum_a G) / A,
   each plus the underflow allowance 2^-126 (Z + 1 + |g| + sum_z |g q|) per gl (the logits over +-60
   give subnormal q, where a relative bound says nothing: a flushed operand or product).

5. ``pfrl_dqn_act_head``: q bit-identical to ``pfrl_linear_small_fwd``; on integer operands q and the
   greedy action equal the float64 reference (first maximum, rows with ties planted).

Not tested, on purpose: NaN operands and actions outside [0, A) (the kernels do not check ``action``;
an out-of-range index is a wild read).  ``k_dqn_td_loss``, ``k_dqn_head_td_rows`` and ``k_c51_loss``
select with ``v > best``, which never ranks a NaN as the maximum, while ``k_dqn_act_head`` does
(``c != c && bv == bv``), as torch / numpy argmax: the two families differ on NaN action values.
"""
import ctypes
import functools
import itertools

import numpy as np
import pytest
import torch

from pfrl_amd import _native, ops
from pfrl_amd.nn import mfma_trunk as mt

gpu = pytest.mark.gpu

GUARD = 4096
U = 2.0 ** -24
TINY = 2.0 ** -126
PFRL_ERR_ARG = -2
LARGEST = 4096 * 512            # floats in the largest buffer of any case
F32 = np.float32
_p, _stream, _cd = mt._p, mt._stream, mt._ceil_div


# ------------------------------------------------------------------ helpers (copies of test_linear_envelope's)
class _Guarded:
    """n floats between two guard zones, everything NaN until a kernel writes it."""

    def __init__(self, n, dev):
        assert n <= LARGEST
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


class _GuardedI64:
    """The same for int64 outputs: a sentinel no kernel writes instead of NaN."""
    MARK = -(1 << 62)

    def __init__(self, n, dev):
        self.n = n
        self.full = torch.full((n + 2 * GUARD,), self.MARK, dtype=torch.int64, device=dev)
        self.t = self.full[GUARD:GUARD + n]

    def done(self, what=""):
        assert bool((self.full[:GUARD] == self.MARK).all()) and bool((self.full[GUARD + self.n:] == self.MARK).all()), \
            "guard zone round %s was written" % what
        assert not bool((self.t == self.MARK).any()), "%s: payload not fully written" % what
        return self.t

    def untouched(self, what=""):
        assert bool((self.full == self.MARK).all()), "%s was written" % what


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


def _same(name, tag, out, want):
    out = out.detach().cpu().reshape(want.shape)
    assert out.dtype == want.dtype, (name, out.dtype, want.dtype)
    if not torch.equal(out, want):
        bad = (out != want).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError("%s %s: %d elements differ, first at %s: got %r, want %r" % (
            name, tag, len(bad), i, float(out[i]), float(want[i])))


def _fold(tasks):
    """pfrl_splitk_reduce itself (no two-level pre-fold): tasks (part, out, stride, n, splits)."""
    n = len(tasks)
    arr = lambda ty, vals: (ty * n)(*vals)      # noqa: E731
    rc = _native.lib().pfrl_splitk_reduce(
        n, arr(ctypes.c_void_p, [t[0].data_ptr() for t in tasks]), arr(ctypes.c_void_p, [t[1].data_ptr() for t in tasks]),
        arr(ctypes.c_void_p, [0] * n), arr(ctypes.c_int64, [t[2] for t in tasks]), arr(ctypes.c_int32, [t[3] for t in tasks]),
        arr(ctypes.c_int32, [t[4] for t in tasks]), arr(ctypes.c_int32, [4] * n), arr(ctypes.c_int32, [0] * n), _stream())
    mt.check(rc, "splitk_reduce")


def _dev():
    return torch.device("cuda:0")


# ------------------------------------------------------------------ TD operands, shared by sections 1 and 2
DELTAS = [0.0, 0.5, -0.5, 1.0, -1.0, 1.5, -1.5]
SENTINEL_MIN_B = 16             # the planted rows need 9 rows; cases with fewer rows carry none
SWITCHES = list(itertools.product((0, 1), (0, 1), (False, True)))      # clip_delta, mean, weights


def required_kinds(A):
    need = {"delta %+.1f" % v for v in DELTAS} | {"terminal", "action 0", "action A-1"}
    return need | ({"tie"} if A >= 2 else set())


def _draw_td(g, B, A, double, kind):
    o = {}
    if kind == "int":
        def ri(lo, hi, *s):
            return torch.randint(lo, hi + 1, s, generator=g).float()
        o["tq"], o["sel"] = ri(-4, 4, B, A), (ri(-4, 4, B, A) if double else None)
        o["r"] = ri(-4, 4, B) * 0.5
        o["disc"] = torch.tensor([0.0, 0.5, 1.0])[torch.randint(0, 3, (B,), generator=g)]
        o["term"] = ri(0, 1, B)
        o["w"] = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (B,), generator=g)]
    else:
        def rn(*s):
            return torch.randn(s, generator=g)
        o["tq"], o["sel"], o["r"] = rn(B, A), (rn(B, A) if double else None), rn(B)
        o["disc"] = torch.tensor(0.99) ** torch.randint(1, 4, (B,), generator=g).float()
        o["term"] = (torch.rand(B, generator=g) < 0.2).float()
        o["w"] = torch.rand(B, generator=g) + 0.5
    o["action"] = torch.randint(0, A, (B,), generator=g)
    if kind == "int" and B >= SENTINEL_MIN_B:
        n = len(DELTAS)
        o["action"][0], o["action"][1] = 0, A - 1
        o["disc"][:n] = 1.0
        o["term"][:n] = (torch.arange(n) % 2).float()
        o["term"][n + 1] = 1.0
        if A >= 2:
            s = o["sel"] if double else o["tq"]
            i, j = (0 if A == 2 else 1), A - 1
            s[n] = s[n].clamp(max=3.0)
            s[n, i] = s[n, j] = 4.0
            if double:
                o["tq"][n, i], o["tq"][n, j] = 2.0, -3.0
    return o


def td_targets_f32(o):
    """-> (greedy index, next value, t) with the kernel's loads and float32 association:
    first maximum of the selection values, t = r + (disc * (1 - term)) * next."""
    tq = o["tq"].numpy()
    s = tq if o["sel"] is None else o["sel"].numpy()
    best = s.argmax(1)                                   # numpy: the first maximum
    nxt = tq[np.arange(tq.shape[0]), best]
    coef = o["disc"].numpy() * (F32(1.0) - o["term"].numpy())
    t = o["r"].numpy() + coef * nxt
    assert t.dtype == np.float32
    return best, nxt, t


def _plant_rewards(o, y):
    """Rows 0..6 get the reward that makes y - t exactly DELTAS[i] (discount 1 there)."""
    n = len(DELTAS)
    nxt = torch.from_numpy(td_targets_f32(o)[1])
    o["r"][:n] = y[:n].float() - (1.0 - o["term"][:n]) * nxt[:n] - torch.tensor(DELTAS)


def td_kinds(o, d, A):
    """Which sentinel rows the operands hold, read off the reference."""
    kinds = {"delta %+.1f" % v for v in DELTAS if bool((d == v).any())}
    if bool((o["term"] == 1).any()):
        kinds.add("terminal")
    if bool((o["action"] == 0).any()):
        kinds.add("action 0")
    if bool((o["action"] == A - 1).any()):
        kinds.add("action A-1")
    s = o["tq"] if o["sel"] is None else o["sel"]
    top = s.max(1, keepdim=True).values
    hit = s == top
    first = hit.float().argmax(1)
    last = (A - 1) - hit.flip(1).float().argmax(1)
    tie = (hit.sum(1) >= 2) & (first < A - 1)
    if o["sel"] is not None:            # Double DQN: the tie must matter -- another value at the later maximum
        ar = torch.arange(s.shape[0])
        tie &= o["tq"][ar, first] != o["tq"][ar, last]
    if bool(tie.any()):
        kinds.add("tie")
    return kinds


def td_terms(d, w, B, clip, mean):
    """float64: (loss terms w L(d), not yet scaled; g w scale; scale) from d = y - t."""
    ad = d.abs()
    scale = 1.0 / B if mean else 1.0
    if clip:
        loss = torch.where(ad < 1, 0.5 * ad * ad, ad - 0.5)
        g = torch.where(ad < 1, d, torch.sign(d))
    else:
        loss, g = 0.5 * d * d, d
    return loss * w, g * w * scale, scale


def _selection_gap_holds(o):
    s = o["tq"] if o["sel"] is None else o["sel"]
    if s.shape[1] < 2:
        return True
    top = s.double().topk(2, dim=1).values
    return bool((top[:, 0] > top[:, 1]).all())


# ================================================================== 1. pfrl_dqn_td_loss
TD_B = [1, 2, 63, 64, 255, 256, 257, 1000, 4096]
TD_A = [1, 2, 6, 18, 64]


def _td_shapes():
    return [(B, A) for i, B in enumerate(TD_B) for j, A in enumerate(TD_A) if (i + j) % 3 == 0]


class _TDCase:
    def __init__(self, B, A, double, kind):
        g = torch.Generator().manual_seed(7919 * B + 31 * A + 2 * int(double) + (kind == "int"))
        self.B, self.A, self.double, self.kind = B, A, double, kind
        self.q = (torch.randint(-4, 5, (B, A), generator=g).float() if kind == "int"
                  else torch.randn(B, A, generator=g))
        self.o = o = _draw_td(g, B, A, double, kind)
        ar = torch.arange(B)
        self.y = self.q[ar, o["action"]]
        if kind == "int" and B >= SENTINEL_MIN_B:
            _plant_rewards(o, self.y)
        self.t = torch.from_numpy(td_targets_f32(o)[2])
        self.d = self.y - self.t                      # float32, IEEE: the kernel's __fsub_rn
        assert self.d.dtype == torch.float32
        if kind == "int":
            assert bool((self.d * 2 == (self.d * 2).round()).all())
            if B >= SENTINEL_MIN_B:
                missing = required_kinds(A) - td_kinds(o, self.d, A)
                assert not missing, missing
        else:
            assert _selection_gap_holds(o)            # loads, not sums: the greedy action cannot depend on rounding

    def tag(self):
        return "B%d-A%d-%s" % (self.B, self.A, "double" if self.double else "plain")


@functools.lru_cache(maxsize=4)
def _td_case(B, A, double, kind):
    return _TDCase(B, A, double, kind)


def _to(dev, o, *extra):
    d = {k: (v.to(dev) if v is not None else None) for k, v in o.items()}
    return (d,) + tuple(t.to(dev).contiguous() for t in extra)


def _run_td(c, d, q, clip, mean, use_w):
    dev = q.device
    B, A = c.B, c.A
    out = {"loss": _Guarded(1, dev), "grad": _Guarded(B * A, dev), "y": _Guarded(B, dev), "ad": _Guarded(B, dev)}
    mt.check(_native.lib().pfrl_dqn_td_loss(
        _p(q), _p(d["action"]), _p(d["tq"]), _p(d["sel"]), _p(d["r"]), _p(d["disc"]), _p(d["term"]),
        _p(d["w"]) if use_w else None, B, A, clip, mean, _p(out["loss"].t), _p(out["grad"].t), _p(out["y"].t),
        _p(out["ad"].t), _stream()), "td loss")
    return {k: v.done(k) for k, v in out.items()}


def test_td_matrix_reaches_every_listed_size_and_its_exact_cases_hold_every_sentinel_row():
    """No GPU.  The pruned matrix keeps every B and A of the lists (B = 4096 and the sizes round the
    256-thread stride among them), the exact cases with mean have a power-of-two B, and every exact
    case of 16 rows or more holds the sentinel rows -- the constructor asserts it; here it is run."""
    shapes = _td_shapes()
    assert {B for B, _ in shapes} == set(TD_B) and {A for _, A in shapes} == set(TD_A)
    assert len(shapes) * 3 <= len(TD_B) * len(TD_A) + 2
    assert {1, 255, 256, 257, 4096} <= {B for B, _ in shapes} and 1 in {A for _, A in shapes}
    assert {B for B, _ in shapes if B & (B - 1) == 0} >= {1, 2, 64, 256, 4096}
    seen = 0
    for B, A in shapes:
        for double in (False, True):
            c = _TDCase(B, A, double, "int")
            if B >= SENTINEL_MIN_B:
                assert td_kinds(c.o, c.d, A) >= required_kinds(A)
                seen += 1
    assert seen >= 16
    assert "tie" in required_kinds(2) and "tie" not in required_kinds(1)
    assert {"delta +1.0", "delta -1.0", "delta +0.0", "delta +1.5", "delta -1.5", "delta +0.5", "delta -0.5"} \
        <= required_kinds(1)


@pytest.mark.parametrize("shape", [(64, 6), (257, 18)], ids=str)
def test_td_float32_targets_are_what_float64_computes(shape):
    """No GPU: on the exact operands the float32 expression of t and d equals float64 bit for bit,
    on randn it is within three roundings."""
    B, A = shape
    for kind in ("int", "randn"):
        c = _TDCase(B, A, True, kind)
        o = c.o
        best, nxt, t = td_targets_f32(o)
        assert np.array_equal(best, o["sel"].double().numpy().argmax(1))
        t64 = o["r"].double() + (o["disc"].double() * (1 - o["term"].double())) * torch.from_numpy(nxt).double()
        if kind == "int":
            assert torch.equal(torch.from_numpy(t).double(), t64)
            assert torch.equal(c.d.double(), c.y.double() - t64)
        else:
            mag = o["r"].double().abs() + (o["disc"].double() * torch.from_numpy(nxt).double()).abs()
            assert bool(((torch.from_numpy(t).double() - t64).abs() <= 4 * U * mag).all())


@gpu
@pytest.mark.parametrize("kind", ["int", "randn"])
@pytest.mark.parametrize("shape", _td_shapes(), ids=lambda s: "B%d-A%d" % s)
def test_td_loss_matches_float64(shape, kind):
    dev = _dev()
    B, A = shape
    for double in (False, True):
        c = _td_case(B, A, double, kind)
        d, q = _to(dev, c.o, c.q)
        ar = torch.arange(B)
        for clip, mean, use_w in SWITCHES:
            if kind == "int" and mean and B & (B - 1):
                continue                                 # 1 / B must be exact
            tag = "%s-clip%d-mean%d-w%d" % (c.tag(), clip, mean, use_w)
            got = _run_td(c, d, q, clip, mean, use_w)
            _same("td y", tag, got["y"], c.y)
            _same("td |delta|", tag, got["ad"], c.d.abs())
            w = c.o["w"].double() if use_w else torch.ones(B, dtype=torch.float64)
            terms, gq, scale = td_terms(c.d.double(), w, B, clip, mean)
            grad = torch.zeros(B, A, dtype=torch.float64)
            grad[ar, c.o["action"]] = gq
            if kind == "int":
                assert bool((terms * 16 == (terms * 16).round()).all()) and float(terms.abs().sum()) < 2 ** 20
                _same("td loss", tag, got["loss"], (terms.sum() * scale).float().reshape(1))
                _same("td grad", tag, got["grad"], grad.float())
            else:
                _within("dqn_td_loss grad", tag, got["grad"], grad, 4 * U * grad.abs())
                _within("dqn_td_loss loss", tag, got["loss"], (terms.sum() * scale).reshape(1),
                        (2 * (B + 3) * U * terms.abs().sum() * scale).reshape(1))


@gpu
def test_td_loss_refuses_an_empty_batch():
    dev = _dev()
    lib = _native.lib()
    buf, out = torch.zeros(64, device=dev), _Guarded(64, dev)
    act = torch.zeros(8, dtype=torch.int64, device=dev)
    p, o = _p(buf), _p(out.t)
    rcs = [lib.pfrl_dqn_td_loss(p, _p(act), p, None, p, p, p, None, B, A, 1, 0, o, o, o, o, _stream())
           for B, A in ((0, 4), (4, 0))]
    assert rcs == [PFRL_ERR_ARG] * 2, rcs
    torch.cuda.synchronize()
    out.untouched("an output of a refused call")


# ================================================================== 2. pfrl_dqn_head_td_loss
HEAD_B = [1, 2, 3, 4, 5, 7, 8, 9, 33]
HEAD_BIG = [(2, 512, 4096), (5, 256, 4096)]         # slab buffers of 1024 x (A K + 32) <= LARGEST floats
H_SPLITS = [1, 2, 7, 8, 9, 16, 17]
DH_SCALES = [1.0, 0.5, 1.0 / 3.0]


def _head_cases():
    """(A, K, B): every instantiation once, the batch sizes spread over them, then the two at 4096."""
    inst = [(A, K) for A in range(1, 17) for K in (256, 512)]
    return [(A, K, HEAD_B[i % len(HEAD_B)]) for i, (A, K) in enumerate(inst)] + HEAD_BIG


def head_c_gate(B, K, A):
    """PFRL_CHECK_ARG of pfrl_dqn_head_td_loss, restated."""
    return B >= 1 and 1 <= A <= 16 and K in (256, 512)


class _HeadCase:
    def __init__(self, A, K, B, double, kind):
        g = torch.Generator().manual_seed(104729 * A + 13 * K + 1009 * B + 2 * int(double) + (kind == "int"))
        self.A, self.K, self.B, self.double, self.kind = A, K, B, double, kind
        if kind == "int":
            def draw(a, keep, *shape):
                return torch.randint(-a, a + 1, shape, generator=g).float() * (torch.rand(shape, generator=g) < keep)
            self.h = draw(2, 5.0 / 6.0, B, K)            # a fifth drawn zero, a sixth cleared: a third zero
            # (W in -2..2; at 4096 rows seven eighths of it zero, so that the loss sum stays exact)
            self.w, self.b = draw(2, 1.0 if B <= 33 else 0.125, A, K), draw(4, 1.0, A)
        else:
            self.h = torch.randn(B, K, generator=g)
            self.w, self.b = torch.randn(A, K, generator=g) / K ** 0.5, torch.randn(A, generator=g)
        self.h[0, 0], self.h[0, 1], self.h[0, 2] = 0.0, -0.0, -1.0
        assert torch.signbit(self.h[0, 1]) and not torch.signbit(self.h[0, 0])
        self.o = o = _draw_td(g, B, A, double, kind)
        ar = torch.arange(B)
        act = o["action"]
        H, W, Bi = self.h.double(), self.w.double(), self.b.double()
        self.y = (H @ W.t() + Bi)[ar, act]
        yabs = (H.abs() @ W.abs().t())[ar, act]
        self.E_y = (K + 2) * U * yabs + U * Bi.abs()[act]
        if kind == "int":
            assert float((yabs + Bi.abs()[act]).max()) < 2 ** 24
            if B >= SENTINEL_MIN_B:
                _plant_rewards(o, self.y)
        for _ in range(200):
            self.t = torch.from_numpy(td_targets_f32(o)[2])
            self.d = self.y - self.t.double()
            self.E_d = self.E_y + U * self.d.abs()
            near = ((self.d.abs() - 1).abs() <= 2 * self.E_d) if kind == "randn" else torch.zeros(B, dtype=torch.bool)
            if not bool(near.any()):
                break
            o["r"][near] = torch.randn(int(near.sum()), generator=g)
        if kind == "int":
            assert bool((self.d * 2 == (self.d * 2).round()).all())
            if B >= SENTINEL_MIN_B:
                missing = required_kinds(A) - td_kinds(o, self.d, A)
                assert not missing, missing
        else:
            assert _selection_gap_holds(o)
            assert not bool(((self.d.abs() - 1).abs() <= 2 * self.E_d).any())     # no row at the Huber branch point

    def tag(self):
        return "A%d-K%d-B%d-%s" % (self.A, self.K, self.B, "double" if self.double else "plain")

    def ref(self, clip, mean, use_w):
        """float64 results and first-order error bounds (without the factor 2), per slab and in total."""
        A, K, B = self.A, self.K, self.B
        S = _cd(B, 4)
        d, E = self.d, self.E_d
        ad = d.abs()
        w = self.o["w"].double() if use_w else torch.ones(B, dtype=torch.float64)
        terms, gq, scale = td_terms(d, w, B, clip, mean)
        lt = terms * scale
        g = gq / (w * scale)
        lmax = (ad + E).clamp(max=1.0) if clip else ad + E
        E_l = lmax * E + 2 * U * (terms / w)
        E_gq = (E + 3 * U * g.abs()) * w * scale
        E_lt = (E_l + 3 * U * (terms / w)) * w * scale
        act = self.o["action"]
        H, Wa = self.h.double(), self.w.double()[act]
        idx = (torch.arange(B) // 4) * A + act
        sidx = torch.arange(B) // 4

        def slabs(rows, n, index):
            z = torch.zeros((n,) + tuple(rows.shape[1:]), dtype=torch.float64)
            return z.index_add_(0, index, rows)
        r = {"scale": scale, "S": S,
             "dh": gq[:, None] * Wa, "E_dh": (E_gq + U * gq.abs())[:, None] * Wa.abs(),
             "dWs": slabs(gq[:, None] * H, S * A, idx).view(S, A * K),
             "E_dWs": slabs((E_gq + 4 * U * gq.abs())[:, None] * H.abs(), S * A, idx).view(S, A * K),
             "A_dWs": slabs(gq.abs()[:, None] * H.abs(), S * A, idx).view(S, A * K),
             "dbs": slabs(gq, S * A, idx).view(S, A), "E_dbs": slabs(E_gq + 3 * U * gq.abs(), S * A, idx).view(S, A),
             "A_dbs": slabs(gq.abs(), S * A, idx).view(S, A),
             "ls": slabs(lt, S, sidx), "E_ls": slabs(E_lt + 3 * U * lt, S, sidx), "lt": lt}
        if self.kind == "int":
            # the premise of the exact check: loss terms multiples of scale / 16 with a sum below 2^20 of
            # them x 16, weight-gradient terms multiples of scale / 4 with column sums below 2^22
            assert bool((terms * 16 == (terms * 16).round()).all()) and float(terms.abs().sum()) < 2 ** 20
            assert float(r["A_dWs"].sum(0).max()) / scale < 2 ** 22
        return r


@functools.lru_cache(maxsize=4)
def _head_case(A, K, B, double, kind):
    return _HeadCase(A, K, B, double, kind)


def _run_head(c, d, h, w, b, clip, mean, use_w, fold=None, dh_scale=None):
    """fold = (h_part, h_splits, h_stride, h_bias): the h_part route.  dh_scale: ask for dh_masked."""
    dev = w.device
    A, K, B = c.A, c.K, c.B
    S, stride = _cd(B, 4), A * K + 32
    out = {"y": _Guarded(B, dev), "ad": _Guarded(B, dev), "dh": _Guarded(B * K, dev), "part": _Guarded(S * stride, dev)}
    if fold is not None:
        out["h_out"] = _Guarded(B * K, dev)
    if dh_scale is not None:
        out["dhm"] = _Guarded(B * K, dev)
    fa = (_p(fold[0]), fold[1], fold[2], _p(fold[3]), _p(out["h_out"].t)) if fold is not None else (None, 0, 0, None, None)
    mt.check(_native.lib().pfrl_dqn_head_td_loss(
        _p(h), _p(w), _p(b), _p(d["action"]), _p(d["tq"]), _p(d["sel"]), _p(d["r"]), _p(d["disc"]), _p(d["term"]),
        _p(d["w"]) if use_w else None, B, K, A, clip, mean, _p(out["y"].t), _p(out["ad"].t), _p(out["dh"].t),
        _p(out["part"].t), *fa, _p(out["dhm"].t) if dh_scale is not None else None,
        float(dh_scale if dh_scale is not None else 1.0), _stream()), "head td loss")
    return {k: v.done(k) for k, v in out.items()}


def _fold_head(part, c):
    dev = part.device
    A, K, S = c.A, c.K, _cd(c.B, 4)
    stride = A * K + 32
    dw, db, loss = _Guarded(A * K, dev), _Guarded(A, dev), _Guarded(1, dev)
    _fold([(part, dw.t, stride, A * K, S), (part[A * K:], db.t, stride, A, S), (part[A * K + 16:], loss.t, stride, 1, S)])
    return dw.done("dw"), db.done("db"), loss.done("loss")


def _check_head(c, dev, switches):
    A, K, B = c.A, c.K, c.B
    S, AK = _cd(B, 4), A * K
    d, h, w, b = _to(dev, c.o, c.h, c.w, c.b)
    exact = c.kind == "int"
    for clip, mean, use_w in switches:
        if exact and mean and B & (B - 1):
            continue
        tag = "%s-clip%d-mean%d-w%d" % (c.tag(), clip, mean, use_w)
        r = c.ref(clip, mean, use_w)
        got = _run_head(c, d, h, w, b, clip, mean, use_w)
        pv = got["part"].view(S, AK + 32).cpu()
        # the layout: nothing between db and the loss, nothing after it
        assert not bool(pv[:, AK + A:AK + 16].any()) and not bool(pv[:, AK + 17:].any()), tag
        dw, db, loss = _fold_head(got["part"], c)
        tot = {"dw": r["dWs"].sum(0), "db": r["dbs"].sum(0), "loss": r["ls"].sum(0, keepdim=True)}
        if exact:
            _same("head y", tag, got["y"], c.y.float())
            _same("head |delta|", tag, got["ad"], c.d.abs().float())
            _same("head dh", tag, got["dh"], r["dh"].float().view(-1))
            # slab i holds rows 4i..4i+3 and nothing else; absent rows of the last slab add nothing
            _same("head slab dW", tag, pv[:, :AK], r["dWs"].float())
            _same("head slab db", tag, pv[:, AK:AK + A], r["dbs"].float())
            _same("head slab loss", tag, pv[:, AK + 16], r["ls"].float())
            for key, folded, lo, hi in (("dw", dw, 0, AK), ("db", db, AK, AK + A), ("loss", loss, AK + 16, AK + 17)):
                _same("head folded " + key, tag, folded, tot[key].float())
                _same("head slab sum " + key, tag, pv[:, lo:hi].sum(0), tot[key].float())
            continue
        name = "dqn_head_td_loss"
        _within(name + " y", tag, got["y"], c.y, 2 * c.E_y)
        _within(name + " |delta|", tag, got["ad"], c.d.abs(), 2 * c.E_d)
        _within(name + " dh", tag, got["dh"], r["dh"].view(-1), 2 * r["E_dh"].view(-1))
        _within(name + " slab dW", tag, pv[:, :AK], r["dWs"], 2 * r["E_dWs"])
        _within(name + " slab db", tag, pv[:, AK:AK + A], r["dbs"], 2 * r["E_dbs"])
        _within(name + " slab loss", tag, pv[:, AK + 16], r["ls"], 2 * r["E_ls"])
        E = {"dw": r["E_dWs"].sum(0), "db": r["E_dbs"].sum(0), "loss": r["E_ls"].sum(0, keepdim=True)}
        Ab = {"dw": r["A_dWs"].sum(0), "db": r["A_dbs"].sum(0), "loss": r["lt"].abs().sum(0, keepdim=True)}
        for key, folded, lo, hi in (("dw", dw, 0, AK), ("db", db, AK, AK + A), ("loss", loss, AK + 16, AK + 17)):
            _within(name + " slab sum " + key, tag, pv[:, lo:hi].double().sum(0), tot[key], 2 * E[key])
            _within(name + " folded " + key, tag, folded, tot[key], 2 * (E[key] + (S + 1) * U * Ab[key]))


def test_head_matrix_reaches_every_instantiation_and_the_listed_sizes():
    """No GPU: 16 widths x 2 depths, every listed B, B = 4096 inside the buffer limit, the h_splits
    list round the eight-at-a-time fold, the exact cases of 16 rows or more with their sentinel rows."""
    cases = _head_cases()
    assert {(A, K) for A, K, _ in cases} == {(A, K) for A in range(1, 17) for K in (256, 512)}
    assert len({(A, K) for A, K, _ in cases}) == 32
    assert {B for _, _, B in cases} == {1, 2, 3, 4, 5, 7, 8, 9, 33, 4096}
    assert all(_cd(B, 4) * (A * K + 32) <= LARGEST and B * K <= LARGEST for A, K, B in cases)
    assert {K for _, K, B in cases if B == 4096} == {256, 512}
    assert set(H_SPLITS) >= {1, 2, 7, 8, 9, 16, 17} and DH_SCALES == [1.0, 0.5, 1.0 / 3.0]
    assert {s % 8 for s in H_SPLITS} >= {0, 1, 7}        # a multiple of eight, one past it, one short of it
    seen = 0
    for A, K, B in cases:
        if 16 <= B <= 64:
            for double in (False, True):
                c = _HeadCase(A, K, B, double, "int")
                assert td_kinds(c.o, c.d, A) >= required_kinds(A)
                seen += 1
    assert seen >= 6
    assert all(head_c_gate(B, K, A) for A, K, B in cases)


class _FakeTensor:
    """What ops.*_supported reads of a tensor, without a device."""
    is_cuda = True

    def __init__(self, *shape, dtype=torch.float32):
        self.shape, self.dtype, self.ndim = shape, dtype, len(shape)

    def dim(self):
        return len(self.shape)

    def is_contiguous(self):
        return True


def test_python_gates_admit_only_what_the_c_gates_admit(monkeypatch):
    """ops.dqn_head_td_loss_supported and ops.dueling_softmax_supported lie inside PFRL_CHECK_ARG of their
    entries (restated: head_c_gate; the dueling entries want A > 0 and 1 <= Z <= 64)."""
    monkeypatch.setattr(_native, "available", lambda: True)
    n = 0
    for B in (0, 1, 32, 4096, 4097):
        for K in (64, 128, 256, 384, 512, 1024):
            for A in range(0, 19):
                if ops.dqn_head_td_loss_supported(_FakeTensor(B, K), _FakeTensor(A, K), _FakeTensor(A)):
                    n += 1
                    assert head_c_gate(B, K, A), (B, K, A)
    assert n == 3 * 2 * 16
    assert not ops.dqn_head_td_loss_supported(_FakeTensor(32, 512), _FakeTensor(6, 512), None)
    admitted = [Z for Z in range(-1, 70) if ops.dueling_softmax_supported(_FakeTensor(4, 6 * max(Z, 1)), Z)]
    assert admitted == list(range(1, 65))
    assert [Z for Z in range(0, 70) if ops.c51_loss_supported(_FakeTensor(32, 6, Z))] == list(range(2, 65))
    assert ops.c51_loss_supported(_FakeTensor(4096, 6, 51)) and not ops.c51_loss_supported(_FakeTensor(4097, 6, 51))


@gpu
@pytest.mark.parametrize("kind", ["int", "randn"])
@pytest.mark.parametrize("case_", _head_cases(), ids=lambda c: "A%d-K%d-B%d" % c)
def test_head_td_loss_matches_float64(case_, kind):
    dev = _dev()
    A, K, B = case_
    for double in (False, True):
        # (at 4096 rows the four switch settings that differ most; the rest all eight)
        sw = [(1, 0, True), (0, 1, False), (1, 1, True), (0, 0, False)] if B == 4096 else SWITCHES
        _check_head(_head_case(A, K, B, double, kind), dev, sw)


def fold_h_f32(slabs, bias):
    """h = relu(((0 + s0) + s1 + ...) + bias) in float32, the order the header promises."""
    acc = torch.zeros_like(slabs[0])
    for s in range(slabs.shape[0]):
        acc = acc + slabs[s]
    return torch.maximum(acc + bias, torch.zeros_like(acc))


def _h_slabs(g, splits, B, K, kind):
    if kind == "int":
        slabs = torch.randint(-1, 2, (splits, B, K), generator=g).float()
        bias = torch.randint(-2, 3, (K,), generator=g).float()
    else:
        slabs = torch.randn(splits, B, K, generator=g) / splits ** 0.5
        bias = torch.randn(K, generator=g) * 0.1
    # pre-activation exactly 0; every operand -0.0 (the fold starts from +0.0, so it gives +0.0); negative
    slabs[:, 0, 0], bias[0] = 0.0, 0.0
    slabs[:, 0, 1], bias[1] = -0.0, -0.0
    slabs[:, 0, 2], bias[2] = -1.0, -0.5
    if splits >= 2:                       # ... and an exact cancellation
        slabs[:, 0, 3], bias[3] = 0.0, 0.0
        slabs[0, 0, 3], slabs[splits - 1, 0, 3] = 1.5, -1.5
    return slabs, bias


@pytest.mark.parametrize("splits", H_SPLITS)
def test_float32_fold_of_h_is_what_float64_computes(splits):
    """No GPU: fold_h_f32 against float64 -- exact on integer slabs, within (S + 1) u sum |.| on randn."""
    g = torch.Generator().manual_seed(splits)
    for kind in ("int", "randn"):
        slabs, bias = _h_slabs(g, splits, 5, 256, kind)
        got = fold_h_f32(slabs, bias)
        ref = (slabs.double().sum(0) + bias.double()).clamp(min=0)
        assert not bool(torch.signbit(got[0, :4]).any()) and bool((got[0, :3] == 0).all())
        if kind == "int":
            assert torch.equal(got.double(), ref)
        else:
            mag = slabs.double().abs().sum(0) + bias.double().abs()
            assert bool(((got.double() - ref).abs() <= (splits + 1) * U * mag).all())


@gpu
@pytest.mark.parametrize("kind", ["int", "randn"])
@pytest.mark.parametrize("splits", H_SPLITS)
def test_head_td_loss_folds_the_hidden_layers_slabs_in_the_promised_order(splits, kind):
    """The h_part route: h_out bit for bit the float32 loop, everything downstream bit-identical to
    a second launch given that h_out as plain h; slab stride B K and B K + 64 with NaN padding; h
    itself a NaN-filled buffer (documented as ignored)."""
    dev = _dev()
    for (A, K, B), pad in itertools.product([(3, 256, 5), (6, 512, 9), (16, 256, 2)], (0, 64)):
        c = _head_case(A, K, B, True, kind)
        g = torch.Generator().manual_seed(31 * splits + A + pad)
        slabs, bias = _h_slabs(g, splits, B, K, kind)
        want = fold_h_f32(slabs, bias)
        assert bool((want[0, :3] == 0).all()) and float(want.max()) > 0
        stride = B * K + pad
        stage = torch.full((splits, stride), float("nan"))
        stage[:, :B * K] = slabs.view(splits, B * K)
        d, w, b, hp, hb = _to(dev, c.o, c.w, c.b, stage, bias)
        h_nan = torch.full((B, K), float("nan"), device=dev)
        for clip, mean, use_w in ((1, 0, True), (0, 1, False)):
            tag = "%s-S%d-pad%d" % (c.tag(), splits, pad)
            one = _run_head(c, d, h_nan, w, b, clip, mean, use_w, fold=(hp, splits, stride, hb), dh_scale=0.5)
            assert torch.equal(one["h_out"].cpu().view(B, K).view(torch.int32), want.view(torch.int32)), tag
            two = _run_head(c, d, one["h_out"].clone(), w, b, clip, mean, use_w, dh_scale=0.5)
            for key in ("y", "ad", "dh", "part", "dhm"):
                _same("h_part route " + key, tag, one[key].cpu(), two[key].cpu())
            assert bool(torch.isnan(h_nan).all())


@gpu
@pytest.mark.parametrize("kind", ["int", "randn"])
@pytest.mark.parametrize("scale", DH_SCALES, ids=["1", "0.5", "third"])
def test_head_td_loss_masked_dh_is_the_relu_mask_times_the_scale(scale, kind):
    """dh_masked = where(h > 0, fl(dh * scale), 0) from the kernel's own dh; h = +0.0, -0.0 and
    negative give 0; asking for it leaves dh (and every other output) as it was."""
    dev = _dev()
    for A, K, B in ((4, 512, 7), (11, 256, 33), (1, 256, 1)):
        c = _head_case(A, K, B, False, kind)
        d, h, w, b = _to(dev, c.o, c.h, c.w, c.b)
        for clip, mean, use_w in ((1, 0, True), (0, 1, True)):
            tag = "%s-scale%.3f" % (c.tag(), scale)
            plain = _run_head(c, d, h, w, b, clip, mean, use_w)
            got = _run_head(c, d, h, w, b, clip, mean, use_w, dh_scale=scale)
            for key in ("y", "ad", "dh", "part"):
                _same("dh_masked leaves " + key, tag, got[key].cpu(), plain[key].cpu())
            dh = got["dh"].cpu().view(B, K)
            scaled = dh if scale == 1.0 else dh * torch.tensor(scale, dtype=torch.float32)
            want = torch.where(c.h > 0, scaled, torch.zeros_like(dh))
            _same("dh_masked", tag, got["dhm"].view(B, K), want)
            m = got["dhm"].cpu().view(B, K)
            assert c.h[0, 0] == 0 and torch.signbit(c.h[0, 1]) and c.h[0, 2] < 0 and bool((m[0, :3] == 0).all())
            assert bool((m[c.h <= 0] == 0).all()) and bool((c.h > 0).any())


@gpu
def test_head_td_loss_refuses_what_its_gate_refuses():
    dev = _dev()
    lib = _native.lib()
    buf, out = torch.zeros(1 << 16, device=dev), _Guarded(1 << 16, dev)
    act = torch.zeros(64, dtype=torch.int64, device=dev)
    p, o, a = _p(buf), _p(out.t), _p(act)

    def call(B, K, A, fold):
        return lib.pfrl_dqn_head_td_loss(p, p, p, a, p, None, p, p, p, None, B, K, A, 1, 0, o, o, o, o, *fold,
                                         None, 1.0, _stream())
    none = (None, 0, 0, None, None)
    rcs = {"A = 0": call(4, 256, 0, none), "A = 17": call(4, 256, 17, none), "K = 128": call(4, 128, 4, none),
           "K = 384": call(4, 384, 4, none), "B = 0": call(0, 256, 4, none),
           "h_splits = 0": call(4, 256, 4, (p, 0, 1024, p, o)), "h_out = NULL": call(4, 256, 4, (p, 2, 1024, p, None)),
           "h_bias = NULL": call(4, 256, 4, (p, 2, 1024, None, o)),
           "h_stride < B K": call(4, 256, 4, (p, 2, 1023, p, o))}
    assert all(rc == PFRL_ERR_ARG for rc in rcs.values()), rcs
    torch.cuda.synchronize()
    out.untouched("an output of a refused call")


# ================================================================== 3. pfrl_c51_loss
C51_B = [1, 15, 16, 17, 33, 500, 4096]
C51_A = [1, 2, 7, 8, 9, 16, 17, 18]
C51_Z = [2, 3, 51, 63, 64]
C51_BIG = [(4096, 8, 64), (4096, 9, 51), (4096, 1, 2), (4096, 2, 3)]


def _c51_shapes():
    out = [(B, A, Z) for i, B in enumerate(C51_B) for j, A in enumerate(C51_A) for k, Z in enumerate(C51_Z)
           if (i + j + k) % 4 == 0 and B * A * Z <= LARGEST]
    return out + [s for s in C51_BIG if s not in out]


def c51_project_f32(p, z, rew, disc, term):
    """The categorical projection with the kernel's float32 operations: p [B][Z] (the greedy action's
    target distribution), z [Z]; -> t [B][Z], accumulated over j increasing, lower contribution then upper."""
    p, z, rew, disc, term = (np.ascontiguousarray(a, dtype=np.float32) for a in (p, z, rew, disc, term))
    B, Z = p.shape
    v_min, v_max, dz = z[0], z[Z - 1], z[1] - z[0]
    scale = (F32(1.0) - term) * disc
    tz = rew[:, None] + scale[:, None] * z[None, :]
    tz = np.minimum(np.maximum(tz, v_min), v_max)
    bj = (tz - v_min) / dz
    bj = np.minimum(np.maximum(bj, F32(0.0)), F32(Z - 1))
    lo, up = np.floor(bj), np.ceil(bj)
    frac = bj - lo
    wl, wu = p * (F32(1.0) - frac), p * frac
    assert all(a.dtype == np.float32 for a in (scale, tz, bj, frac, wl, wu))
    lo, up = lo.astype(np.int64), up.astype(np.int64)
    t = np.zeros((B, Z), dtype=np.float32)
    ar = np.arange(B)
    for j in range(Z):
        t[ar, lo[:, j]] = t[ar, lo[:, j]] + wl[:, j]
        t[ar, up[:, j]] = t[ar, up[:, j]] + wu[:, j]
    return t, lo, up


def c51_project_f64(p, z, rew, disc, term):
    """The same in float64 (scatter-add form of the reference)."""
    p, z, rew, disc, term = (np.asarray(a, dtype=np.float64) for a in (p, z, rew, disc, term))
    B, Z = p.shape
    tz = np.clip(rew[:, None] + ((1.0 - term) * disc)[:, None] * z[None, :], z[0], z[-1])
    bj = np.clip((tz - z[0]) / (z[1] - z[0]), 0, Z - 1)
    lo, up = np.floor(bj).astype(np.int64), np.ceil(bj).astype(np.int64)
    t = np.zeros((B, Z))
    rows = np.repeat(np.arange(B), Z)
    np.add.at(t, (rows, lo.ravel()), (p * (1.0 - (bj - lo))).ravel())
    np.add.at(t, (rows, up.ravel()), (p * (bj - lo)).ravel())
    return t


def _softmax_rows(g, *shape):
    return torch.softmax(torch.randn(shape, generator=g, dtype=torch.float64) * 1.5, -1).float()


class _C51Case:
    def __init__(self, B, A, Z, flavor):
        g = torch.Generator().manual_seed(15485863 % (B + 7) + 613 * A + 7 * Z + (flavor == "integer") + 1000 * B)
        self.B, self.A, self.Z, self.flavor = B, A, Z, flavor
        if flavor == "random":
            self.z = torch.linspace(-10, 10, Z)
            self.disc = torch.tensor(0.99) ** torch.randint(1, 4, (B,), generator=g).float()
            self.r = torch.randn(B, generator=g) * 3
            self.term = (torch.rand(B, generator=g) < 0.2).float()
            if B >= 15:
                # the whole support clamped to either end (+-25: 25 - 0.99 * 10 > 10) and most of it
                # (+-15); terminal with the reward on an atom / between two
                self.r[0], self.r[1], self.r[4], self.r[5] = 25.0, -25.0, 15.0, -15.0
                self.term[0] = self.term[1] = self.term[4] = self.term[5] = 0.0
                self.term[2] = self.term[3] = 1.0
                self.r[2], self.r[3] = self.z[Z // 2], (self.z[0] + self.z[1]) / 2
        else:
            self.z = torch.arange(Z).float() - Z // 2           # integer atoms: bj integral, lo == up
            self.disc = torch.tensor([0.5, 1.0])[torch.randint(0, 2, (B,), generator=g)]
            self.r = torch.randint(-3, 4, (B,), generator=g).float()
            self.term = (torch.rand(B, generator=g) < 0.2).float()
        self.action = torch.randint(0, A, (B,), generator=g)
        self.w = torch.rand(B, generator=g) + 0.5
        ar = torch.arange(B)
        self.q_soft = _softmax_rows(g, B, A, Z)
        self.q_pow = self.q_soft.clone()
        self.q_pow[ar, self.action] = 2.0 ** -torch.randint(0, 21, (B, Z), generator=g).float()
        self.nd = self._settled(g)
        self.sel = self._settled(g)
        self.tie_rows = torch.zeros(B, dtype=torch.bool)
        if A >= 2:
            Q = self._values(self.sel)[0]
            for b in range(3, B, 7):
                i = int(Q[b].argmax())
                j = (i + 1) % A
                self.sel[b, j] = self.sel[b, i]
                assert not torch.equal(self.nd[b, i], self.nd[b, j])
                self.tie_rows[b] = True
        self.greedy, self.t, self.lo_eq_up = {}, {}, {}
        for use_sel in (False, True):
            dist = self.sel if use_sel else self.nd
            Q, thr = self._values(dist)
            gr = torch.from_numpy(Q.numpy().argmax(1))               # numpy: the first maximum
            if A >= 2:
                top = Q.topk(min(3, A), dim=1).values
                gap = top[:, 0] - top[:, 1]
                tied = self.tie_rows if use_sel else torch.zeros(B, dtype=torch.bool)
                assert bool((gap[~tied] > thr[~tied]).all())
                assert bool((gap[tied] == 0).all())
                if A >= 3:
                    assert bool(((top[:, 0] - top[:, 2])[tied] > thr[tied]).all())
                if bool(tied.any()):                                # the tie is between gr and a LATER action
                    later = (Q[tied] == Q[tied].max(1, keepdim=True).values).float().flip(1).argmax(1)
                    assert bool(((A - 1 - later) > gr[tied]).all())
            self.greedy[use_sel] = gr
            t, lo, up = c51_project_f32(self.nd[ar, gr].numpy(), self.z.numpy(), self.r.numpy(), self.disc.numpy(),
                                        self.term.numpy())
            self.t[use_sel] = torch.from_numpy(t)
            self.lo_eq_up[use_sel] = float((lo == up).mean())

    def _values(self, dist):
        z = self.z.double()
        Q = (dist.double() * z).sum(-1)
        thr = 2 * (self.Z + 2) * U * (dist.double() * z.abs()).sum(-1).max(1).values
        return Q, thr

    def _settled(self, g):
        """A [B][A][Z] tensor of distributions whose best and second-best expected value differ by more
        than the bound in every row: rows that do not are drawn again."""
        dist = _softmax_rows(g, self.B, self.A, self.Z)
        for _ in range(100):
            if self.A < 2:
                break
            Q, thr = self._values(dist)
            top = Q.topk(2, dim=1).values
            bad = (top[:, 0] - top[:, 1]) <= thr
            if not bool(bad.any()):
                break
            dist[bad] = _softmax_rows(g, int(bad.sum()), self.A, self.Z)
        return dist

    def tag(self):
        return "B%d-A%d-Z%d-%s" % (self.B, self.A, self.Z, self.flavor)

    def ref(self, q, use_sel, use_w, mean):
        """float64 results given the bit-exact t, and first-order bounds (without the factor 2)."""
        B, Z = self.B, self.Z
        ar = torch.arange(B)
        t = self.t[use_sel].double()
        y32 = q[ar, self.action]
        lo32 = torch.tensor(1e-10, dtype=torch.float32)
        y = y32.double()
        yc = y.clamp(float(lo32), 1.0)
        terms = -t * torch.log(yc)
        delta = terms.sum(-1)
        E_delta = (Z + 4) * U * terms.abs().sum(-1)
        z = self.z.double()
        coef = (self.w.double() if use_w else torch.ones(B, dtype=torch.float64)) * (1.0 / B if mean else 1.0)
        inb = (y32 >= lo32) & (y32 <= 1.0)
        grow = torch.where(inb, -t / yc * coef[:, None], torch.zeros_like(t))
        grad = torch.zeros(B, self.A, Z, dtype=torch.float64)
        grad[ar, self.action] = grow
        return {"delta": delta, "E_delta": E_delta, "q": (y * z).sum(-1), "E_q": (Z + 2) * U * (y * z).abs().sum(-1),
                "loss": (delta * coef).sum().reshape(1),
                "E_loss": ((E_delta * coef).sum() + (B + 3) * U * (delta * coef).abs().sum()).reshape(1),
                "grad": grad, "E_grad": 4 * U * grad.abs(), "inb": inb}


@functools.lru_cache(maxsize=2)
def _c51_case(B, A, Z, flavor):
    return _C51Case(B, A, Z, flavor)


def _run_c51(c, d, q, use_sel, use_w, mean):
    dev = q.device
    B, A, Z = c.B, c.A, c.Z
    out = {"loss": _Guarded(1, dev), "grad": _Guarded(B * A * Z, dev), "q": _Guarded(B, dev), "delta": _Guarded(B, dev)}
    mt.check(_native.lib().pfrl_c51_loss(
        _p(q), _p(d["action"]), _p(d["nd"]), _p(d["sel"]) if use_sel else None, _p(d["z"]), _p(d["r"]), _p(d["disc"]),
        _p(d["term"]), _p(d["w"]) if use_w else None, B, A, Z, int(mean), _p(out["loss"].t), _p(out["grad"].t),
        _p(out["q"].t), _p(out["delta"].t), _stream()), "c51 loss")
    return {k: v.done(k) for k, v in out.items()}


def _c51_dev(c, dev):
    return {k: getattr(c, k).to(dev).contiguous() for k in ("action", "nd", "sel", "z", "r", "disc", "term", "w")}


def _check_c51_rounded(c, got, r, tag):
    name = "c51_loss"
    _within(name + " delta", tag, got["delta"], r["delta"], 2 * r["E_delta"])
    _within(name + " q", tag, got["q"], r["q"], 2 * r["E_q"])
    _within(name + " loss", tag, got["loss"], r["loss"], 2 * r["E_loss"])
    _within(name + " grad", tag, got["grad"], r["grad"], 2 * r["E_grad"])


def test_c51_matrix_reaches_every_listed_size():
    """No GPU: every B, A and Z of the lists is kept -- B = 4096 (kMaxBatch, 16 waves striding the
    batch) and the boundaries 8, 9, 16, 17 of the eight-at-a-time action loads among them."""
    shapes = _c51_shapes()
    assert {s[0] for s in shapes} == set(C51_B) and {s[1] for s in shapes} == set(C51_A)
    assert {s[2] for s in shapes} == set(C51_Z)
    assert {8, 9, 16, 17} <= {s[1] for s in shapes} and 4096 in {s[0] for s in shapes}
    assert {Z for B, _, Z in shapes if B == 4096} >= {2, 64} and {A for B, A, _ in shapes if B == 4096} >= {1, 8, 9}
    assert all(B * A * Z <= LARGEST for B, A, Z in shapes)
    assert len(shapes) * 3 <= len(C51_B) * len(C51_A) * len(C51_Z)
    for A in (8, 9, 16, 17):           # each boundary at a small and a full-wave Z and with more rows than waves
        assert {Z for _, AA, Z in shapes if AA == A} & {2, 3} and {Z for _, AA, Z in shapes if AA == A} & {63, 64}
        assert max(B for B, AA, _ in shapes if AA == A) > 16


@pytest.mark.parametrize("shape", [(33, 7, 51), (17, 9, 2), (16, 2, 64), (15, 18, 3)], ids=str)
def test_c51_float32_projection_is_what_float64_computes(shape):
    """No GPU: the float32 loop against the float64 scatter-add -- a distribution again (sum 1), within
    rounding of the float64 projection; on the integer support many bj are integral (lo == up) and
    the projection of such a row is exact.  The planted rows and exact ties are where they should be."""
    B, A, Z = shape
    for flavor in ("random", "integer"):
        c = _C51Case(B, A, Z, flavor)
        ar = torch.arange(B)
        for use_sel in (False, True):
            p = c.nd[ar, c.greedy[use_sel]]
            t64 = c51_project_f64(p.numpy(), c.z.numpy(), c.r.numpy(), c.disc.numpy(), c.term.numpy())
            t32 = c.t[use_sel].double().numpy()
            assert np.abs(t32.sum(1) - p.double().sum(1).numpy()).max() < 4 * Z * U
            if flavor == "integer":
                assert c.lo_eq_up[use_sel] > 0.25
                whole = ((c.disc == 1.0) | (c.term == 1.0)).numpy()
                assert whole.any() and np.abs(t32 - t64)[whole].max() < 2 * Z * U
            else:
                # (bj is rounded before frac is taken: the weights move by u |bj| <= Z u per source atom)
                assert np.abs(t32 - t64).max() < 8 * Z * U
                assert c.t[use_sel][0, Z - 1] > 0.999 and c.t[use_sel][1, 0] > 0.999      # clamped to either end
                assert c.t[use_sel][2, Z // 2] > 0.999                                    # terminal, on an atom
                assert abs(float(c.t[use_sel][3, 0]) - 0.5) < 1e-3 and abs(float(c.t[use_sel][3, 1]) - 0.5) < 1e-3
        assert bool(c.tie_rows.any()) and bool((c.greedy[True][c.tie_rows] < A).all())


@gpu
@pytest.mark.parametrize("shape", _c51_shapes(), ids=lambda s: "B%d-A%d-Z%d" % s)
def test_c51_loss_projects_bit_for_bit_and_matches_float64(shape):
    dev = _dev()
    B, A, Z = shape
    ar = torch.arange(B)
    for flavor in ("random", "integer"):
        c = _c51_case(B, A, Z, flavor)
        d = _c51_dev(c, dev)
        q_pow, q_soft = c.q_pow.to(dev), c.q_soft.to(dev)
        for use_sel in (False, True):
            tag = "%s-sel%d" % (c.tag(), use_sel)
            # (a) the projected target, read out through the gradient: -grad * y == t, bit for bit
            got = _run_c51(c, d, q_pow, use_sel, False, 0)
            grad = got["grad"].cpu().view(B, A, Z)
            taken = torch.zeros(B, A, dtype=torch.bool)
            taken[ar, c.action] = True
            assert not bool(grad[~taken].any()), tag                  # the other actions' rows: zero
            _same("c51 projected target", tag, -grad[ar, c.action] * c.q_pow[ar, c.action], c.t[use_sel])
            _check_c51_rounded(c, got, c.ref(c.q_pow, use_sel, False, 0), tag + "-pow2")
            # (b) rounded, on softmax rows, every weights / mean setting
            for use_w, mean in ((False, 0), (True, 1), (True, 0), (False, 1)):
                got = _run_c51(c, d, q_soft, use_sel, use_w, mean)
                assert not bool(got["grad"].cpu().view(B, A, Z)[~taken].any()), tag
                _check_c51_rounded(c, got, c.ref(c.q_soft, use_sel, use_w, mean), "%s-w%d-mean%d" % (tag, use_w, mean))


@gpu
@pytest.mark.parametrize("shape", [(33, 3, 51), (17, 9, 2), (16, 1, 64)], ids=str)
def test_c51_loss_at_both_clamp_edges(shape):
    """Entries of the taken row equal to 0, float32(1e-10), the float below it, 1.0, the float above
    1 and 1.5: the gradient is 0 strictly outside [1e-10, 1] and -t / yc coef at and between the bounds."""
    dev = _dev()
    B, A, Z = shape
    lo = np.float32(1e-10)
    edges = torch.tensor([0.0, float(lo), float(np.nextafter(lo, F32(0))), 1.0, float(np.nextafter(F32(1), F32(2))),
                          1.5, 0.25], dtype=torch.float32)
    ar = torch.arange(B)
    for flavor in ("random", "integer"):
        c = _c51_case(B, A, Z, flavor)
        q = c.q_soft.clone()
        q[ar, c.action] = edges[(torch.arange(B)[:, None] + torch.arange(Z)[None, :]) % len(edges)]
        d = _c51_dev(c, dev)
        for use_sel, use_w, mean in ((False, False, 0), (True, True, 1), (True, True, 0)):
            tag = "%s-edges-sel%d-w%d-mean%d" % (c.tag(), use_sel, use_w, mean)
            r = c.ref(q, use_sel, use_w, mean)
            y = q[ar, c.action]
            outside = (y < lo) | (y > 1.0)
            assert bool((r["inb"] == ~outside).all()) and bool(outside.any()) and bool((~outside).any())
            assert bool((c.t[use_sel][outside] > 0).any()) and bool((c.t[use_sel][y == float(lo)] > 0).any() or Z == 2)
            got = _run_c51(c, d, q.to(dev), use_sel, use_w, mean)
            grow = got["grad"].cpu().view(B, A, Z)[ar, c.action]
            assert not bool(grow[outside].any()), tag
            assert bool((grow[~outside][c.t[use_sel][~outside] > 0] != 0).all()), tag
            _check_c51_rounded(c, got, r, tag)


@gpu
def test_c51_loss_runs_at_4096_rows_and_refuses_what_its_gate_refuses():
    dev = _dev()
    lib = _native.lib()
    buf, out = torch.full((1 << 16,), 0.5, device=dev), _Guarded(1 << 16, dev)
    act = torch.zeros(4200, dtype=torch.int64, device=dev)
    p, o, a = _p(buf), _p(out.t), _p(act)
    rcs = {(B, A, Z): lib.pfrl_c51_loss(p, a, p, None, p, p, p, p, None, B, A, Z, 0, o, o, o, o, _stream())
           for B, A, Z in ((4097, 2, 4), (0, 2, 4), (4, 2, 1), (4, 2, 65), (4, 0, 4))}
    assert all(rc == PFRL_ERR_ARG for rc in rcs.values()), rcs
    torch.cuda.synchronize()
    out.untouched("an output of a refused call")
    assert (4096, 8, 64) in _c51_shapes()            # B = 4096 itself runs in the matrix test


# ================================================================== 4. pfrl_dueling_softmax_fwd / _bwd
DUEL_B = [1, 3, 4, 5, 257]
DUEL_A = [1, 7, 8, 9, 16, 17]
DUEL_Z = [1, 2, 51, 63, 64]


def _duel_shapes():
    return [(B, A, Z) for i, B in enumerate(DUEL_B) for j, A in enumerate(DUEL_A) for k, Z in enumerate(DUEL_Z)
            if (i + j + k) % 3 == 0]


def test_dueling_matrix_reaches_every_listed_size():
    shapes = _duel_shapes()
    assert {s[0] for s in shapes} == set(DUEL_B) and {s[1] for s in shapes} == set(DUEL_A)
    assert {s[2] for s in shapes} == set(DUEL_Z)
    assert {7, 8, 9, 16, 17} <= {s[1] for s in shapes} and {1, 64} <= {s[2] for s in shapes}
    assert {B % 4 for B, _, _ in shapes} == {0, 1, 3} and any(A == 1 for _, A, _ in shapes)
    for A in (8, 9, 16, 17):
        assert {Z for _, AA, Z in shapes if AA == A} & {63, 64} and {Z for _, AA, Z in shapes if AA == A} & {1, 2}
    assert len(shapes) * 3 <= len(DUEL_B) * len(DUEL_A) * len(DUEL_Z)


def dueling_fwd_ref(ya, ys):
    """float64 softmax of (ya - mean_a ya) + ys and its bound (factor 2 included)."""
    A, Z = ya.shape[1], ya.shape[2]
    ya, ys = ya.double(), ys.double()[:, None, :]
    mean_abs = ya.abs().mean(1, keepdim=True)
    x = (ya - ya.mean(1, keepdim=True)) + ys
    q = torch.softmax(x, -1)
    E_x = U * (A * mean_abs + 3 * (ya.abs() + mean_abs + ys.abs()))
    eps = E_x + U * (x - x.max(-1, keepdim=True).values).abs()
    return q, 2 * q * (eps + (q * eps).sum(-1, keepdim=True) + (Z + 4) * U) + TINY


def dueling_bwd_ref(q, gq):
    A, Z = q.shape[1], q.shape[2]
    q, gq = q.double(), gq.double()
    gl = q * (gq - (gq * q).sum(-1, keepdim=True))
    G = q * (gq.abs() + (gq * q).abs().sum(-1, keepdim=True))
    g_ys = gl.sum(1)
    g_ya = gl - g_ys[:, None, :] / A
    GA = G.sum(1)
    # below the smallest normal float the relative model does not hold: a subnormal q (or product) may be
    # flushed, which moves the dot product by at most Z 2^-126 and gl by 2^-126 (1 + |g| + sum |g q|)
    under = TINY * (Z + 1 + gq.abs() + (gq * q).abs().sum(-1, keepdim=True))
    UA = under.sum(1)
    return (g_ya, 2 * ((Z + 4) * U * G + (Z + A + 4) * U * GA[:, None, :] / A) + under + UA[:, None, :] / A,
            g_ys, 2 * (Z + A + 2) * U * GA + UA)


def _duel_fwd(ya, ys):
    B, A, Z = ya.shape
    q = _Guarded(B * A * Z, ya.device)
    mt.check(_native.lib().pfrl_dueling_softmax_fwd(_p(ya), _p(ys), _p(q.t), B, A, Z, _stream()), "dueling fwd")
    return q.done("q").view(B, A, Z)


def _duel_bwd(gq, q):
    B, A, Z = q.shape
    g_ya, g_ys = _Guarded(B * A * Z, q.device), _Guarded(B * Z, q.device)
    mt.check(_native.lib().pfrl_dueling_softmax_bwd(_p(gq), _p(q), _p(g_ya.t), _p(g_ys.t), B, A, Z, _stream()),
             "dueling bwd")
    return g_ya.done("g_ya").view(B, A, Z), g_ys.done("g_ys").view(B, Z)


@gpu
@pytest.mark.parametrize("shape", _duel_shapes(), ids=lambda s: "B%d-A%d-Z%d" % s)
def test_dueling_softmax_matches_float64(shape):
    dev = _dev()
    B, A, Z = shape
    g = torch.Generator().manual_seed(977 * B + 31 * A + Z)
    tag = "B%d-A%d-Z%d" % shape
    for spread in (False, True):
        ya, ys = 2 * torch.randn(B, A, Z, generator=g), 2 * torch.randn(B, Z, generator=g)
        if spread:                      # logits over +-60: without the max subtraction expf overflows
            ys = (torch.rand(B, Z, generator=g) * 2 - 1) * 60
            ys[:, 0] = 60.0
        q = _duel_fwd(ya.to(dev), ys.to(dev))
        ref, bound = dueling_fwd_ref(ya, ys)
        _within("dueling_softmax_fwd", tag + ("-spread" if spread else ""), q, ref, bound)
        if Z == 1:
            assert bool((q == 1.0).all())
        gq = torch.randn(B, A, Z, generator=g)
        g_ya, g_ys = _duel_bwd(gq.to(dev), q.contiguous())
        r_ya, b_ya, r_ys, b_ys = dueling_bwd_ref(q.cpu(), gq)
        _within("dueling_softmax_bwd g_ya", tag, g_ya, r_ya, b_ya)
        _within("dueling_softmax_bwd g_ys", tag, g_ys, r_ys, b_ys)
        if A == 1:
            assert not bool(g_ya.any())            # gl - gl / 1: a bit-exact zero
    if Z & (Z - 1) == 0:
        # logits constant over the atoms: every exponent is exp(0), the sum is Z, the quotient 1 / Z
        ya = torch.randn(B, A, 1, generator=g).expand(B, A, Z).contiguous()
        ys = torch.randn(B, 1, generator=g).expand(B, Z).contiguous()
        q = _duel_fwd(ya.to(dev), ys.to(dev))
        assert bool((q == 1.0 / Z).all()), tag


@gpu
def test_dueling_softmax_with_an_empty_batch_writes_nothing_and_refuses_bad_sizes():
    dev = _dev()
    lib = _native.lib()
    buf, out = torch.zeros(4096, device=dev), _Guarded(4096, dev)
    p, o = _p(buf), _p(out.t)
    assert lib.pfrl_dueling_softmax_fwd(p, p, o, 0, 4, 8, _stream()) == 0
    assert lib.pfrl_dueling_softmax_bwd(p, p, o, o, 0, 4, 8, _stream()) == 0
    rcs = [lib.pfrl_dueling_softmax_fwd(p, p, o, 4, A, Z, _stream()) for A, Z in ((0, 8), (4, 0), (4, 65))]
    rcs += [lib.pfrl_dueling_softmax_bwd(p, p, o, o, 4, A, Z, _stream()) for A, Z in ((0, 8), (4, 0), (4, 65))]
    assert rcs == [PFRL_ERR_ARG] * 6, rcs
    torch.cuda.synchronize()
    out.untouched("an output of a call that launches nothing")


# ================================================================== 5. pfrl_dqn_act_head
ACT_MK = [(1, 1), (5, 96), (37, 512), (256, 1500)]
ACT_OUTPUTS = [c for c in itertools.product((False, True), repeat=3) if any(c)]        # q, greedy, action wanted


def _act_case(M, K, N, kind, g):
    if kind == "int":
        h = torch.randint(-3, 4, (M, K), generator=g).float()
        w = torch.randint(-2, 3, (N, K), generator=g).float()
        b = torch.randint(-4, 4, (N,), generator=g).float()          # -4..3
        h[::3] = 0.0                       # q = the bias there: the planted tie decides
        if N >= 2:
            b[0 if N == 2 else 1] = b[N - 1] = 4.0
    else:
        h, w, b = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g), torch.randn(N, generator=g)
    choice = torch.where(torch.rand(M, generator=g) < 0.3, torch.randint(0, N, (M,), generator=g),
                         torch.full((M,), -1)).to(torch.int32)
    return h, w, b, choice


def test_act_head_cases_cover_every_width_and_output_combination():
    assert len(ACT_OUTPUTS) == 7 and len(ACT_MK) == 4
    g = torch.Generator().manual_seed(0)
    for N in range(2, 17):
        for M, K in ACT_MK:
            h, w, b, _ = _act_case(M, K, N, "int", g)
            q = h.double() @ w.double().t() + b.double()
            tie = (q == q.max(1, keepdim=True).values).sum(1) >= 2
            assert bool(tie.any()) and float((h.abs().double() @ w.abs().double().t()).max()) < 2 ** 24
            first = q[tie].numpy().argmax(1)
            assert (first < N - 1).all()


@gpu
@pytest.mark.parametrize("kind", ["int", "randn"])
@pytest.mark.parametrize("N", range(1, 17))
def test_act_head_every_width_equals_the_small_forward_and_picks_the_first_maximum(N, kind):
    dev = _dev()
    lib = _native.lib()
    g = torch.Generator().manual_seed(1000 + N)
    for M, K in ACT_MK:
        h, w, b, choice = _act_case(M, K, N, kind, g)
        hd, wd, bd, cd = h.to(dev), w.to(dev), b.to(dev), choice.to(dev)
        for bias in (True, False):
            tag = "M%d-K%d-N%d-bias%d" % (M, K, N, bias)
            y = _Guarded(M * N, dev)
            mt.check(lib.pfrl_linear_small_fwd(_p(hd), _p(wd), _p(bd) if bias else None, _p(y.t), M, K, N, _stream()),
                     "small fwd")
            q_small = y.done("y").cpu().view(M, N)
            q64 = h.double() @ w.double().t() + (b.double() if bias else 0.0)
            if kind == "int":
                _same("act head: small forward", tag, q_small, q64.float())
                want_greedy = torch.from_numpy(q64.numpy().argmax(1))          # first maximum of the reference
                if N >= 2:
                    assert bool(((q64 == q64.max(1, keepdim=True).values).sum(1) >= 2).any())
            else:
                ab = h.double().abs() @ w.double().abs().t() + (b.double().abs() if bias else 0.0)
                _within("dqn_act_head q", tag, q_small, q64, 2 * (K + 2) * U * ab)
                want_greedy = torch.from_numpy(q_small.numpy().argmax(1))      # loads of the kernel's own q
            for (want_q, want_g, want_a), use_choice in itertools.product(ACT_OUTPUTS, (False, True)):
                q = _Guarded(M * N, dev) if want_q else None
                gr = _GuardedI64(M, dev) if want_g else None
                ac = _GuardedI64(M, dev) if want_a else None
                mt.check(lib.pfrl_dqn_act_head(
                    _p(hd), _p(wd), _p(bd) if bias else None, _p(cd) if use_choice else None, _p(q.t) if q else None,
                    _p(gr.t) if gr else None, _p(ac.t) if ac else None, M, K, N, _stream()), "act head")
                if q:
                    _same("act head q", tag, q.done("q").cpu().view(M, N), q_small)
                if gr:
                    _same("act head greedy", tag, gr.done("greedy"), want_greedy)
                if ac:
                    want = torch.where(choice >= 0, choice.long(), want_greedy) if use_choice else want_greedy
                    _same("act head action", tag, ac.done("action"), want)
    out, outi = _Guarded(64, dev), _GuardedI64(64, dev)
    rcs = [lib.pfrl_dqn_act_head(_p(hd), _p(wd), None, None, None, None, None, 4, 4, 4, _stream()),
           lib.pfrl_dqn_act_head(_p(hd), _p(wd), None, None, _p(out.t), _p(outi.t), _p(outi.t), 1, 1, 17, _stream()),
           lib.pfrl_dqn_act_head(_p(hd), _p(wd), None, None, _p(out.t), _p(outi.t), _p(outi.t), 1, 1, 0, _stream())]
    assert rcs == [PFRL_ERR_ARG] * 3, rcs
    torch.cuda.synchronize()
    out.untouched("q of a refused call")
    outi.untouched("greedy / action of a refused call")
