"""The TD3 / DDPG launches of ``csrc/td3.hip`` -- ``pfrl_td3_smooth_action``, ``pfrl_td3_critic_loss``,
``pfrl_td3_critic_loss_bwd``, ``pfrl_neg_mean`` -- through the C ABI, against references evaluated on
the CPU only.  Method, helpers and guard zones of tests/test_actor_critic_envelope.py (COVERAGE rows
a24-a29): bit for bit where the arithmetic is a fixed sequence of IEEE operations, a derived bound
elsewhere, every output between NaN guard zones of 4096 floats.

u = 2^-24.  Every rounded bound is first order and is asserted with a factor 2.

1. ``pfrl_td3_smooth_action``: fl(sigma z), a clamp, fl(a + e), a clamp -- no freedom: bit for bit the
   NumPy float32 restatement ``smooth_f32``, itself pinned to ``default_target_policy_smoothing_func``
   on torch CPU float32.  Planted: fl(sigma z) == +-c, the nearest products float32 reaches on either
   side of +-c (for sigma = 0.7, c = 0.1 the products of consecutive z step by more than one ulp of c,
   so "the float next to c" itself is not always a product; the nearest ones on each side are), sums
   exactly at lo / hi and the floats next to them, +-0.0, a NaN in noise and one in action.

2. ``pfrl_td3_critic_loss``.  t = fl(r + fl(fl(d fl(1 - term)) nq)): bit for bit ``target_f32``.  With
   diff = fl(t - pred) (u |diff| against the exact difference of the float32 operands t and pred):
       unit_g = -fl(fl(2 diff) fl(1 / B)):  u (diff) + u (1 / B) + u (product) = 3 u |g|   (2 diff exact);
       term = fl(diff diff):  2 u + u = 3 u term, so p = 3 in the fold bound of row a25:
       |loss - mean| <= (ceil(B / 256) + 9 + 3) u sum(terms) / B
   (ceil(B / 256) - 1 lane-strided additions, 6 butterfly steps, 2 fold steps, the division, p).
   The reference is float64 torch autograd of ``F.mse_loss(target, pred)`` on the float32 target (which
   is verified bit for bit on its own).
   Exact cases: integer Q values in -4 .. 4, rewards multiples of 1/2, discounts in {0, 1/2, 1}, B a
   power of two: every diff is a multiple of 1/2 below 16, every term a multiple of 1/4, and as long
   as sum(terms) < 2^22 (asserted) every partial sum is a float32, the division by B and the
   gradient's scaling are exact.
   ``_bwd``: g_pred = -fl(g fl(fl(2 diff) fl(1 / B))) = fl(g unit_g): one more rounding, u |g unit_g|;
   g = 1 reproduces unit_g's bits, g = 1/2 is exact.

3. ``pfrl_neg_mean``: terms are the operands themselves (p = 0):
       |loss + mean(q)| <= (ceil(B / 256) + 9) u sum |q| / B;
   exact on multiples of 1/16 below 8 with B a power of two (sum |q| < 2^19 <= 2^20, asserted).
   unit_g_q = -fl(1 / B) = fl(-1 / B): bit for bit ``np.float32(-1) / np.float32(B)``.

``test_bounds_hold_for_a_float32_emulation`` (no GPU) runs the kernels' reduction order in float32
NumPy (lane-strided sums, butterfly, four-way fold) and asserts the bounds of 2 and 3 on these very
operands before the GPU tests rely on them.
"""
import functools
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from pfrl_amd import _native
from pfrl_amd.nn import mfma_trunk as mt
from test_actor_critic_envelope import (F32, F64, PFRL_ERR_ARG, U, _cd, _dev, _f, _Guarded, _p, _ptrs,
                                        _red_bound, _same, _stream, _within)

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pfrl_td3_smooth_action", "pfrl_td3_critic_loss", "pfrl_td3_critic_loss_bwd", "pfrl_neg_mean")

SMOOTH_N = [1, 3, 255, 256, 257, 4099 * 17]
SMOOTH_CFG = [(_f(0.2), 0.5, -1.0, 1.0), (_f(0.7), _f(0.1), -2.0, 0.5), (0.0, 0.5, -1.0, 1.0)]
LOSS_B = [1, 63, 64, 255, 256, 257, 1000, 4099, 65536]
POW2_B = [B for B in LOSS_B if B & (B - 1) == 0]


@pytest.fixture(scope="module", autouse=True)
def _ratio_summary():
    """``_within`` notes every err / bound in the helper module's table; this file's maxima at the end."""
    import test_actor_critic_envelope as env

    yield
    for name in sorted(env._RATIO):
        if any(k in name for k in ("td3_", "neg_mean")):
            print("MAX RATIO %s %.4f" % (name, env._RATIO[name]))


def test_case_lists_are_the_ones_the_kernels_were_specified_for():
    assert SMOOTH_N == [1, 3, 255, 256, 257, 69683]
    assert LOSS_B == [1, 63, 64, 255, 256, 257, 1000, 4099, 65536] and POW2_B == [1, 64, 256, 65536]
    assert {_cd(B, 256) for B in LOSS_B} == {1, 2, 4, 17, 256}
    assert len(_critic_variants()) == 16


def _same_bits(name, tag, out, want):
    """float32, NaN where ``want`` is NaN, the same bits (signed zeros included) elsewhere."""
    got = out.detach().cpu().numpy().reshape(want.shape)
    assert got.dtype == want.dtype == np.float32, (name, got.dtype, want.dtype)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), "%s %s: NaNs not where expected" % (name, tag)
    a, b = got[~nan].view(np.int32), want[~nan].view(np.int32)
    assert np.array_equal(a, b), "%s %s: %d elements differ" % (name, tag, int((a != b).sum()))


# ================================================================== 1. smoothing
def _clamp_f32(x, lo, hi):
    y = np.where(x < lo, lo, x)             # (a NaN fails both comparisons and passes through)
    return np.where(y > hi, hi, y)


def smooth_f32(action, noise, sigma, c, lo, hi):
    e = _clamp_f32(F32(sigma) * noise, F32(-c), F32(c))
    out = _clamp_f32(action + e, F32(lo), F32(hi))
    assert out.dtype == np.float32
    return out


def _step(x, k):
    x = F32(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, F32(np.inf) if k > 0 else F32(-np.inf))
    return x


def _products_round_c(sigma, c):
    """(z with fl(sigma z) == c, largest z with fl(sigma z) < c, smallest z with fl(sigma z) > c)"""
    s, c = F32(sigma), F32(c)
    zs = [_step(c / s, k) for k in range(-8, 9)]
    eq = [z for z in zs if s * z == c]
    below = [z for z in zs if s * z < c]
    above = [z for z in zs if s * z > c]
    assert eq and below and above, (sigma, c)
    return eq[0], max(below), min(above)


@functools.lru_cache(maxsize=None)
def _smooth_operands(n, cfg):
    """-> (action, noise, {what: index}) with the planted elements in the first 20 (n permitting)"""
    sigma, c, lo, hi = cfg
    g = torch.Generator().manual_seed(7919 * n + int(1000 * sigma))
    a = (1.5 * torch.rand(n, generator=g) * 2 - 1.5).numpy()
    z = (3 * torch.randn(n, generator=g)).numpy()
    plant = []
    if sigma > 0:
        eq, below, above = _products_round_c(sigma, c)
        for sign in (1, -1):
            plant += [("product == %+dc" % sign, 0.25, sign * eq), ("product inside %+dc" % sign, 0.25, sign * below),
                      ("product past %+dc" % sign, 0.25, sign * above)]
    for name, bound in (("lo", lo), ("hi", hi)):
        plant += [("sum == " + name, bound, 0.0), ("sum below " + name, _step(bound, -1), 0.0),
                  ("sum above " + name, _step(bound, 1), 0.0)]
    plant += [("-0 + -0", -0.0, -0.0), ("+0 + -0", 0.0, -0.0), ("NaN noise", 0.25, np.nan),
              ("NaN action", np.nan, 0.5)]
    where = {}
    for i, (name, av, zv) in enumerate(plant[:n]):
        a[i], z[i], where[name] = av, zv, i
    return a.astype(np.float32), z.astype(np.float32), where


def test_planted_smoothing_elements_are_what_they_claim():
    for cfg in SMOOTH_CFG:
        sigma, c, lo, hi = cfg
        a, z, where = _smooth_operands(257, cfg)
        out = smooth_f32(a, z, *cfg)
        prod = F32(sigma) * z
        if sigma > 0:
            for sign in (1, -1):
                assert prod[where["product == %+dc" % sign]] == F32(sign * c)
                assert abs(prod[where["product inside %+dc" % sign]]) < F32(c)
                assert abs(prod[where["product past %+dc" % sign]]) > F32(c)
                # at and past the bound the clamp gives the bound, inside the product itself
                assert out[where["product == %+dc" % sign]] == F32(0.25) + F32(sign * c)
                assert out[where["product past %+dc" % sign]] == F32(0.25) + F32(sign * c)
                assert out[where["product inside %+dc" % sign]] == F32(0.25) + prod[where["product inside %+dc" % sign]]
        assert out[where["sum == lo"]] == F32(lo) and out[where["sum below lo"]] == F32(lo)
        assert out[where["sum above lo"]] == _step(lo, 1)
        assert out[where["sum == hi"]] == F32(hi) and out[where["sum above hi"]] == F32(hi)
        assert out[where["sum below hi"]] == _step(hi, -1)
        assert np.signbit(out[where["-0 + -0"]]) and out[where["-0 + -0"]] == 0
        assert not np.signbit(out[where["+0 + -0"]]) and out[where["+0 + -0"]] == 0
        nan = np.isnan(out)
        assert nan.sum() == 2 and nan[where["NaN noise"]] and nan[where["NaN action"]]


def test_smoothing_restatement_is_the_default_function_on_torch_cpu():
    """``default_target_policy_smoothing_func`` (sigma 0.2, c 0.5, [-1, 1]) on the same draw:
    ``torch.equal``; the draw is recovered by seeding the generator again."""
    from pfrl_amd.agents.td3 import default_target_policy_smoothing_func

    for n, A in ((1, 1), (257, 3), (4099, 17)):
        a = (torch.rand(n, A, generator=torch.Generator().manual_seed(n)) * 3 - 1.5)
        a[0, 0] = 1.0
        torch.manual_seed(99 + n)
        want = default_target_policy_smoothing_func(a)
        torch.manual_seed(99 + n)
        z = torch.randn_like(a)
        got = torch.from_numpy(smooth_f32(a.numpy(), z.numpy(), _f(0.2), 0.5, -1.0, 1.0))
        assert want.dtype == torch.float32 and torch.equal(got, want)
        assert bool((want == 1).any()) and bool((want == -1).any()) or n == 1
    # ... and on the planted elements, NaNs and signed zeros included
    a, z, _ = _smooth_operands(257, SMOOTH_CFG[0])
    ta, tz = torch.from_numpy(a), torch.from_numpy(z)
    want = torch.clamp(ta + torch.clamp(0.2 * tz, -0.5, 0.5), -1, 1)
    _same_bits("torch clamp expression", "planted", want, smooth_f32(a, z, *SMOOTH_CFG[0]))


@gpu
@pytest.mark.parametrize("n", SMOOTH_N)
def test_smooth_action_is_the_float32_restatement_bit_for_bit(n):
    dev, L = _dev(), _native.lib()
    for cfg in SMOOTH_CFG:
        a, z, _ = _smooth_operands(n, cfg)
        want = smooth_f32(a, z, *cfg)
        ad, zd = torch.from_numpy(a).to(dev), torch.from_numpy(z).to(dev)
        tag = "n%d-%s" % (n, cfg)
        out = _Guarded(n, dev)
        mt.check(L.pfrl_td3_smooth_action(_p(ad), _p(zd), *cfg, _p(out.t), n, _stream()), "smooth")
        torch.cuda.synchronize()
        _same_bits("td3_smooth_action", tag, out.guards("out"), want)
        assert np.array_equal(zd.cpu().numpy().view(np.int32), z.view(np.int32)), "noise was written"
        inplace = _Guarded(n, dev)
        inplace.t.copy_(zd)
        mt.check(L.pfrl_td3_smooth_action(_p(ad), _p(inplace.t), *cfg, _p(inplace.t), n, _stream()), "smooth")
        torch.cuda.synchronize()
        _same_bits("td3_smooth_action in place", tag, inplace.guards("noise / out"), want)


@gpu
def test_smooth_action_gates():
    dev, L = _dev(), _native.lib()
    x = torch.zeros(8, device=dev)
    out = _Guarded(8, dev)
    ok = [_p(x), _p(x), 0.2, 0.5, -1.0, 1.0, _p(out.t), 8, _stream()]
    bad = []
    for i, v in ((7, 0), (7, -1), (2, -0.1), (2, float("nan")), (3, -0.1), (3, float("nan")), (0, None),
                 (1, None), (6, None)):
        b = list(ok)
        b[i] = v
        bad.append(b)
    b = list(ok)
    b[4], b[5] = 1.0, 0.5                                   # low > high
    bad.append(b)
    b = list(ok)
    b[4] = float("nan")
    bad.append(b)
    assert [L.pfrl_td3_smooth_action(*b) for b in bad] == [PFRL_ERR_ARG] * len(bad)
    b = list(ok)
    b[4], b[5], b[2], b[3] = 0.5, 0.5, 0.0, 0.0             # the edges themselves are admitted
    assert L.pfrl_td3_smooth_action(*b) == 0
    torch.cuda.synchronize()
    assert torch.equal(out.done("low == high"), torch.full((8,), 0.5, device=dev))
    out2 = _Guarded(8, dev)
    for b in bad:
        if b[6] is not None:
            b[6] = _p(out2.t)
            assert L.pfrl_td3_smooth_action(*b) == PFRL_ERR_ARG
    torch.cuda.synchronize()
    out2.untouched("the output of a refused call")


# ================================================================== 2. critic target and loss
def target_f32(r, d, term, nqs):
    """``d``: the float32 discount column or ``np.float32(gamma)``"""
    nq = nqs[0] if len(nqs) == 1 else np.minimum(nqs[0], nqs[1])      # (NaN-propagating, as torch.min)
    out = r + (d * (F32(1) - term)) * nq
    assert out.dtype == np.float32
    return out


def unit_grad_f32(t, pred, B):
    return -((F32(2) * (t - pred)) * (F32(1) / F32(B)))


GAMMA = _f(0.99)


@functools.lru_cache(maxsize=None)
def _critic_operands(B, kind):
    """kind: "integer" (the exact case), "randn", "nan" (randn with a NaN planted in one next_q).
    Rows 0 .. 4 (B permitting): next_q equal, critic 0 smaller, critic 1 smaller, terminal, NaN."""
    g = torch.Generator().manual_seed(31 * B + len(kind))
    if kind == "integer":
        r = torch.randint(-8, 9, (B,), generator=g).float() / 2
        nq = [torch.randint(-4, 5, (B,), generator=g).float() for _ in range(2)]
        pred = [torch.randint(-4, 5, (B,), generator=g).float() for _ in range(2)]
        d = torch.randint(0, 3, (B,), generator=g).float() / 2
    else:
        r = torch.randn(B, generator=g)
        nq = [3 * torch.randn(B, generator=g) for _ in range(2)]
        pred = [3 * torch.randn(B, generator=g) for _ in range(2)]
        d = GAMMA ** torch.randint(1, 4, (B,), generator=g).float()
    term = (torch.rand(B, generator=g) < 0.2).float()
    rows = {}
    if B >= 5:
        nq[1][0] = nq[0][0]
        nq[0][1], nq[1][1] = -1.0, 2.0
        nq[0][2], nq[1][2] = 2.0, -1.0
        term[:3] = 0.0
        term[3] = 1.0
        rows = {"equal": 0, "first smaller": 1, "second smaller": 2, "terminal": 3}
        if kind == "nan":
            nq[1][4] = float("nan")
            term[4] = 0.0
            rows["nan"] = 4
    # (the scalar that stands in for the column: 1/2 keeps the integer case exact)
    o = {"r": r, "d": d, "term": term, "nq0": nq[0], "nq1": nq[1], "p0": pred[0], "p1": pred[1],
         "gamma": torch.tensor(0.5 if kind == "integer" else GAMMA)}
    return {k: v.numpy().astype(np.float32) for k, v in o.items()}, rows


def _critic_variants():
    """(n_q, discount column?, target_q present?, unit_g_pred present?)"""
    return [(n_q, col, tq, ug) for n_q in (1, 2) for col in (True, False) for tq in (True, False)
            for ug in (True, False)]


def _want_target(o, n_q, col):
    return target_f32(o["r"], o["d"] if col else F32(o["gamma"]), o["term"], [o["nq%d" % k] for k in range(n_q)])


@functools.lru_cache(maxsize=None)
def _critic_reference(B, kind, n_q, col):
    """float64 autograd of F.mse_loss on the float32 target, and the bounds of section 2 (no factor 2)"""
    o, _ = _critic_operands(B, kind)
    t32 = _want_target(o, n_q, col)
    t = torch.from_numpy(t32).double()
    out = []
    for k in range(n_q):
        p = torch.from_numpy(o["p%d" % k]).double().requires_grad_(True)
        loss = Fn.mse_loss(t, p)
        (gp,) = torch.autograd.grad(loss, p)
        terms = (t - p.detach()) ** 2
        out.append({"loss": loss.detach().reshape(1), "g": gp, "E_g": 3 * U * gp.abs(),
                    "E_loss": (_red_bound(B, 3, terms.sum()) / B).reshape(1), "terms": terms})
    return t32, out


def _block_sum_f32(x):
    """The reduction order of ``block_sum`` behind a lane-strided loop, in float32 NumPy."""
    x = np.asarray(x, dtype=np.float32)
    rows = np.zeros((_cd(len(x), 256) * 256,), dtype=np.float32)
    rows[:len(x)] = x
    s = np.zeros(256, dtype=np.float32)
    for row in rows.reshape(-1, 256):
        s = s + row
    v = s.reshape(4, 64)
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lane ^ off]
    w = v[:, 0]
    out = (w[0] + w[1]) + (w[2] + w[3])
    assert out.dtype == np.float32
    return out


def _emulate_critic(o, n_q, col, B):
    t = _want_target(o, n_q, col)
    res = []
    for k in range(n_q):
        diff = t - o["p%d" % k]
        res.append((np.array([_block_sum_f32(diff * diff) / F32(B)]), unit_grad_f32(t, o["p%d" % k], B)))
    return t, res


def _check_rounded(name, tag, loss, grad, r):
    _within(name + " loss", tag, torch.as_tensor(loss), r["loss"], 2 * r["E_loss"] + 1e-300)
    if grad is not None:
        _within(name + " unit_g_pred", tag, torch.as_tensor(grad), r["g"], 2 * r["E_g"] + 1e-300)


def _exact_reference(o, n_q, col, B):
    """the float64 closed form of the exact case and its exactness conditions"""
    t = torch.from_numpy(_want_target(o, n_q, col)).double()
    out = []
    for k in range(n_q):
        diff = t - torch.from_numpy(o["p%d" % k]).double()
        terms = diff * diff
        assert bool((terms * 4 == (terms * 4).round()).all()) and float(terms.sum()) < 2 ** 22
        loss, g = terms.sum() / B, -2 * diff / B
        assert float(loss.float().double()) == float(loss) and torch.equal(g.float().double(), g)
        out.append((loss.float().reshape(1), g.float()))
    return out


@pytest.mark.parametrize("B", LOSS_B)
def test_bounds_hold_for_a_float32_emulation(B):
    for n_q in (1, 2):
        for col in (True, False):
            o, _ = _critic_operands(B, "randn")
            _, refs = _critic_reference(B, "randn", n_q, col)
            _, got = _emulate_critic(o, n_q, col, B)
            for k in range(n_q):
                _check_rounded("emulated td3_critic_loss", "B%d-nq%d-col%d-k%d" % (B, n_q, col, k), got[k][0], got[k][1], refs[k])
            if B in POW2_B:
                o, _ = _critic_operands(B, "integer")
                _, got = _emulate_critic(o, n_q, col, B)
                for (loss, g), (el, eg) in zip(_exact_reference(o, n_q, col, B), got):
                    assert torch.equal(torch.from_numpy(el), loss) and torch.equal(torch.from_numpy(eg), g)
    q = _neg_mean_operands(B, "randn")
    got = np.array([-(_block_sum_f32(q) / F32(B))])
    _within("emulated neg_mean", "B%d" % B, torch.from_numpy(got), -torch.from_numpy(q).double().mean().reshape(1),
            (2 * _red_bound(B, 0, torch.from_numpy(q).double().abs().sum()) / B).reshape(1))


def test_float32_restatements_agree_with_float64_to_their_operation_counts():
    for B in (257, 4099):
        o, _ = _critic_operands(B, "randn")
        for n_q in (1, 2):
            for col in (True, False):
                d = o["d"].astype(np.float64) if col else float(o["gamma"])
                nq = o["nq0"].astype(np.float64) if n_q == 1 else np.minimum(o["nq0"], o["nq1"]).astype(np.float64)
                prod = d * (1.0 - o["term"]) * nq
                want = o["r"] + prod
                # 1 - term exact (term in {0, 1}); the two products and the sum: u each
                bound = 2 * (2 * U * np.abs(prod) + U * np.abs(want))
                assert (np.abs(_want_target(o, n_q, col) - want) <= bound).all()
    for cfg in SMOOTH_CFG:
        a, z, _ = _smooth_operands(4099, cfg)
        sigma, c, lo, hi = cfg
        e = np.clip(sigma * z.astype(np.float64), -c, c)
        want = np.clip(a + e, lo, hi)
        got = smooth_f32(a, z, *cfg)
        ok = ~np.isnan(want)
        # the product and the sum: u each (a clamp to a float32 bound adds nothing)
        assert (np.abs(got[ok] - want[ok]) <= 2 * (U * np.abs(e[ok]) + U * np.abs(a[ok] + e[ok]))).all()


def test_closed_form_gradients_are_what_float64_autograd_computes():
    for B in (1, 63, 257):
        o, _ = _critic_operands(B, "randn")
        t32, refs = _critic_reference(B, "randn", 2, True)
        for k in range(2):
            want = -2 * (t32.astype(np.float64) - o["p%d" % k].astype(np.float64)) / B
            assert np.abs(refs[k]["g"].numpy() - want).max() <= 1e-14 * (1 + np.abs(want).max())
        q = torch.randn(B, 1, dtype=F64, requires_grad=True)
        (g,) = torch.autograd.grad(-torch.mean(q), q)
        assert torch.equal(g, torch.full_like(g, -1.0 / B))
        for gl in (0.5, 3.0):
            p = torch.from_numpy(o["p0"]).double().requires_grad_(True)
            (gp,) = torch.autograd.grad(Fn.mse_loss(torch.from_numpy(t32).double(), p), p, torch.tensor(gl, dtype=F64))
            assert float((gp - gl * refs[0]["g"]).abs().max()) <= 1e-14


def _launch_critic(dev, o, n_q, col, with_tq, with_unit, B):
    L = _native.lib()
    d = {k: torch.from_numpy(v).to(dev) for k, v in o.items()}
    tq, loss, unit = _Guarded(B, dev), _Guarded(n_q, dev), _Guarded(n_q * B, dev)
    mt.check(L.pfrl_td3_critic_loss(
        _p(d["r"]), _p(d["d"]) if col else None, 123.0 if col else float(o["gamma"]), _p(d["term"]),
        _ptrs(*[d["nq%d" % k] for k in range(n_q)]), _ptrs(*[d["p%d" % k] for k in range(n_q)]), n_q,
        _p(tq.t) if with_tq else None, _ptrs(*[loss.t[k:] for k in range(n_q)]),
        _ptrs(*[unit.t[k * B:] for k in range(n_q)]) if with_unit else None, B, _stream()), "td3_critic_loss")
    torch.cuda.synchronize()
    if not with_tq:
        tq.untouched("target_q")
    if not with_unit:
        unit.untouched("unit_g_pred")
    return d, tq, loss, unit


@gpu
@pytest.mark.parametrize("B", LOSS_B)
def test_critic_loss_target_bits_loss_and_gradient(B):
    dev = _dev()
    for n_q, col, with_tq, with_unit in _critic_variants():
        tag = "B%d-nq%d-col%d-tq%d-unit%d" % (B, n_q, col, with_tq, with_unit)
        # the target: bit for bit on integer, randn and NaN-planted operands
        for kind in ("integer", "randn", "nan"):
            if not with_tq or (kind == "nan" and with_unit):
                continue
            o, rows = _critic_operands(B, kind)
            want = _want_target(o, n_q, col)
            if B >= 5:
                assert want[rows["terminal"]] == o["r"][rows["terminal"]]
                if kind == "nan":
                    assert np.isnan(want).sum() == (1 if n_q == 2 else 0)
            _, tq, loss, _ = _launch_critic(dev, o, n_q, col, True, with_unit, B)
            _same_bits("td3_critic_loss target_q", tag + "-" + kind, tq.guards("target_q"), want)
            loss.guards("loss")
        # rounded: loss and unit gradient against float64 autograd
        o, _ = _critic_operands(B, "randn")
        t32, refs = _critic_reference(B, "randn", n_q, col)
        _, tq, loss, unit = _launch_critic(dev, o, n_q, col, with_tq, with_unit, B)
        lv = loss.done("loss").cpu()
        uv = unit.done("unit_g_pred").view(n_q, B).cpu() if with_unit else None
        for k in range(n_q):
            _check_rounded("td3_critic_loss", tag + "-k%d" % k, lv[k:k + 1], uv[k] if with_unit else None, refs[k])
            if with_unit:
                _same("td3_critic_loss unit_g_pred restated", tag, uv[k], torch.from_numpy(unit_grad_f32(t32, o["p%d" % k], B)))
        # exact: power-of-two B on the integer operands
        if B in POW2_B:
            o, _ = _critic_operands(B, "integer")
            _, tq, loss, unit = _launch_critic(dev, o, n_q, col, with_tq, with_unit, B)
            lv = loss.done("loss").cpu()
            for k, (el, eg) in enumerate(_exact_reference(o, n_q, col, B)):
                _same("td3_critic_loss exact loss", tag, lv[k:k + 1], el)
                if with_unit:
                    _same("td3_critic_loss exact gradient", tag, unit.done("unit").view(n_q, B)[k], eg)


@gpu
@pytest.mark.parametrize("B", LOSS_B)
def test_critic_loss_bwd_and_repeatability(B):
    dev, L = _dev(), _native.lib()
    o, _ = _critic_operands(B, "randn")
    for n_q in (1, 2):
        tag = "B%d-nq%d" % (B, n_q)
        d, tq, loss, unit = _launch_critic(dev, o, n_q, True, True, True, B)
        _, tq2, loss2, unit2 = _launch_critic(dev, o, n_q, True, True, True, B)
        assert torch.equal(tq.t, tq2.t) and torch.equal(loss.t, loss2.t) and torch.equal(unit.t, unit2.t), \
            "two launches on the same operands differ"
        uv = unit.done("unit").view(n_q, B).cpu()
        preds = _ptrs(*[d["p%d" % k] for k in range(n_q)])
        for gl in (1.0, 0.5, 3.0):
            gld = torch.full((2,), gl, device=dev)
            gp = _Guarded(n_q * B, dev)
            mt.check(L.pfrl_td3_critic_loss_bwd(_ptrs(*[gld[k:] for k in range(n_q)]), _p(tq.t), preds,
                                                _ptrs(*[gp.t[k * B:] for k in range(n_q)]), n_q, B, _stream()), "bwd")
            torch.cuda.synchronize()
            got = gp.done("g_pred").view(n_q, B).cpu()
            if gl == 1.0:
                _same("td3_critic_loss_bwd g = 1 is unit_g_pred", tag, got, uv)
            else:
                want = gl * uv.double()
                _within("td3_critic_loss_bwd g = %g" % gl, tag, got, want, 2 * U * want.abs() + 1e-300)
        # a NULL g_loss entry: zeros for that critic, the other as before
        gld = torch.full((2,), 3.0, device=dev)
        gp = _Guarded(n_q * B, dev)
        ptrs = [None] + [gld[k:] for k in range(1, n_q)]
        mt.check(L.pfrl_td3_critic_loss_bwd(_ptrs(*ptrs), _p(tq.t), preds,
                                            _ptrs(*[gp.t[k * B:] for k in range(n_q)]), n_q, B, _stream()), "bwd")
        torch.cuda.synchronize()
        gz = gp.done("g_pred").view(n_q, B).cpu()
        _same("td3_critic_loss_bwd NULL g_loss", tag, gz[0], torch.zeros(B))
        if n_q == 2:
            _same("td3_critic_loss_bwd beside a NULL g_loss", tag, gz[1], got[1])


@gpu
def test_critic_loss_gates():
    dev, L = _dev(), _native.lib()
    B = 8
    x = torch.zeros(B, device=dev)
    outs = [_Guarded(2 * B, dev) for _ in range(3)]
    tq, loss, unit = outs

    def fwd(**kw):
        a = dict(reward=_p(x), discount=_p(x), gamma=0.5, terminal=_p(x), next_q=_ptrs(x, x), pred=_ptrs(x, x),
                 n_q=2, target_q=_p(tq.t), loss=_ptrs(loss.t, loss.t[1:]), unit=_ptrs(unit.t, unit.t[B:]), B=B)
        a.update(kw)
        return L.pfrl_td3_critic_loss(a["reward"], a["discount"], a["gamma"], a["terminal"], a["next_q"], a["pred"],
                                      a["n_q"], a["target_q"], a["loss"], a["unit"], a["B"], _stream())

    def bwd(**kw):
        a = dict(g_loss=_ptrs(x, x), target_q=_p(x), pred=_ptrs(x, x), g_pred=_ptrs(unit.t, unit.t[B:]), n_q=2, B=B)
        a.update(kw)
        return L.pfrl_td3_critic_loss_bwd(a["g_loss"], a["target_q"], a["pred"], a["g_pred"], a["n_q"], a["B"], _stream())

    rcs = [fwd(B=0), fwd(B=65537), fwd(B=-1), fwd(n_q=0), fwd(n_q=3), fwd(reward=None), fwd(terminal=None),
           fwd(next_q=None), fwd(pred=None), fwd(loss=None), fwd(next_q=_ptrs(None, x)), fwd(next_q=_ptrs(x, None)),
           fwd(pred=_ptrs(None, x)), fwd(pred=_ptrs(x, None)), fwd(loss=_ptrs(None, loss.t)),
           fwd(loss=_ptrs(loss.t, None)), fwd(n_q=1, next_q=_ptrs(None), pred=_ptrs(x), loss=_ptrs(loss.t)),
           bwd(B=0), bwd(B=65537), bwd(n_q=0), bwd(n_q=3), bwd(g_loss=None), bwd(target_q=None), bwd(pred=None),
           bwd(g_pred=None), bwd(pred=_ptrs(x, None)), bwd(g_pred=_ptrs(unit.t, None)),
           L.pfrl_neg_mean(_p(x), _p(loss.t), _p(unit.t), 0, _stream()),
           L.pfrl_neg_mean(_p(x), _p(loss.t), _p(unit.t), 65537, _stream()),
           L.pfrl_neg_mean(None, _p(loss.t), _p(unit.t), B, _stream()),
           L.pfrl_neg_mean(_p(x), None, _p(unit.t), B, _stream())]
    assert rcs == [PFRL_ERR_ARG] * len(rcs), rcs
    torch.cuda.synchronize()
    for t in outs:
        t.untouched("an output of a refused call")
    # what is optional may be NULL: the discount column, target_q, unit_g_pred (array or entry)
    assert fwd(discount=None, target_q=None, unit=_ptrs(None, unit.t[B:])) == 0
    torch.cuda.synchronize()
    tq.untouched("target_q")
    assert bool(torch.isnan(unit.t[:B]).all()) and not bool(torch.isnan(unit.t[B:]).any())


# ================================================================== 3. -mean(q)
@functools.lru_cache(maxsize=None)
def _neg_mean_operands(B, kind):
    g = torch.Generator().manual_seed(17 * B + len(kind))
    if kind == "dyadic":
        return (torch.randint(-127, 128, (B,), generator=g).float() / 16).numpy()
    return (2 * torch.randn(B, generator=g) + 0.5).numpy()


@gpu
@pytest.mark.parametrize("B", LOSS_B)
def test_neg_mean(B):
    dev, L = _dev(), _native.lib()
    for kind in ("dyadic", "randn"):
        q = _neg_mean_operands(B, kind)
        q64 = torch.from_numpy(q).double()
        tag = "B%d-%s" % (B, kind)
        for with_unit in (True, False):
            loss, unit = _Guarded(1, dev), _Guarded(B, dev)
            qd = torch.from_numpy(q).to(dev)
            mt.check(L.pfrl_neg_mean(_p(qd), _p(loss.t), _p(unit.t) if with_unit else None, B, _stream()), "neg_mean")
            torch.cuda.synchronize()
            if with_unit:
                _same("neg_mean unit_g_q", tag, unit.done("unit_g_q"), torch.full((B,), float(F32(-1) / F32(B))))
            else:
                unit.untouched("unit_g_q")
            if kind == "dyadic" and B in POW2_B:
                assert float(q64.abs().sum()) < 2 ** 20 and bool((q64 * 16 == (q64 * 16).round()).all())
                want = -(q64.sum() / B)
                assert float(want.float().double()) == float(want)
                _same("neg_mean exact", tag, loss.done("loss"), want.float().reshape(1))
            else:
                _within("neg_mean", tag, loss.done("loss"), -q64.mean().reshape(1),
                        (2 * _red_bound(B, 0, q64.abs().sum()) / B).reshape(1))
    l1, l2 = _Guarded(1, dev), _Guarded(1, dev)
    for l in (l1, l2):
        mt.check(L.pfrl_neg_mean(_p(qd), _p(l.t), None, B, _stream()), "neg_mean")
    torch.cuda.synchronize()
    assert torch.equal(l1.t, l2.t), "two launches on the same operands differ"


# ================================================================== the autograd nodes on the entry points
@gpu
def test_nodes_return_what_the_entry_points_write_and_fall_back_outside_the_gate():
    from pfrl_amd.agents import _td3_losses as T

    dev = _dev()
    B = 257
    o, _ = _critic_operands(B, "randn")
    d = {k: torch.from_numpy(v).to(dev) for k, v in o.items()}
    one = T.unit_grad(dev)
    for n_q, disc in ((2, d["d"]), (1, GAMMA)):
        preds = [d["p%d" % k].clone().requires_grad_(True) for k in range(n_q)]
        nqs = [d["nq%d" % k].view(B, 1) for k in range(n_q)]
        losses, target = T.critic_losses(d["r"], disc, d["term"], nqs, preds, with_target=True)
        assert all(T.is_loss_node(l) and l.dim() == 0 for l in losses) and not target.requires_grad
        _, tq, lraw, uraw = _launch_critic(dev, o, n_q, n_q == 2, True, True, B)
        assert torch.equal(target, tq.t) and torch.equal(torch.stack(list(losses)).detach(), lraw.t)
        torch.autograd.backward(list(losses), [one] * n_q, retain_graph=True)
        assert all(torch.equal(p.grad, uraw.t[k * B:(k + 1) * B]) for k, p in enumerate(preds))
        for p in preds:
            p.grad = None
        losses[0].backward()                        # (a fresh ones tensor: the _bwd launch)
        assert torch.equal(preds[0].grad, uraw.t[:B])
        if n_q == 2:
            assert preds[1].grad is None or not bool(preds[1].grad.any())
        # outside the gate: float64, strided, on the CPU -> the torch expression, no node
        for conv in (lambda t: t.double(), lambda t: t.cpu(),
                     lambda t: torch.stack([t, t], -1).reshape(t.shape + (2,))[..., 0]):
            dd = conv(disc) if torch.is_tensor(disc) else disc
            ps = [conv(p.detach()).requires_grad_(True) for p in preds]
            ls, tg = T.critic_losses(conv(d["r"]), dd, conv(d["term"]), [conv(n) for n in nqs], ps, with_target=True)
            assert not any(T.is_loss_node(l) for l in ls)
            assert torch.allclose(torch.stack(ls).detach().cpu().float(), lraw.t.cpu(), rtol=1e-5, atol=1e-6)
    q = d["p0"].view(B, 1).clone().requires_grad_(True)
    loss = T.neg_mean(q)
    assert T.is_loss_node(loss)
    loss.backward(one, retain_graph=True)
    assert torch.equal(q.grad, torch.full_like(q, float(F32(-1) / F32(B))))
    q.grad = None
    loss.backward(torch.tensor(3.0, device=dev))
    assert torch.allclose(q.grad, torch.full_like(q, -3.0 / B), rtol=1e-6)
    assert not T.is_loss_node(T.neg_mean(q.double())) and not T.is_loss_node(T.neg_mean(q.detach().cpu().requires_grad_(True)))
    big = torch.zeros(65537, device=dev, requires_grad=True)
    assert not T.is_loss_node(T.neg_mean(big))
    a, z, _ = _smooth_operands(257, SMOOTH_CFG[0])
    ad, zd = torch.from_numpy(a).to(dev), torch.from_numpy(z).to(dev)
    want = smooth_f32(a, z, *SMOOTH_CFG[0])
    _same_bits("smooth_action", "node", T.smooth_action(ad, zd, *SMOOTH_CFG[0]), want)
    buf = zd.clone()
    assert T.smooth_action(ad, buf, *SMOOTH_CFG[0], out=buf) is buf
    _same_bits("smooth_action in place", "node", buf, want)
    _same_bits("smooth_action float64 route", "node", T.smooth_action(ad.double(), zd.double(), 0.25, 0.5, -1, 1).float(),
               np.clip(a.astype(np.float64) + np.clip(0.25 * z.astype(np.float64), -0.5, 0.5), -1, 1).astype(np.float32))


# ================================================================== header, exports, documents
def test_header_exports_and_integration_doc_agree_on_the_four_entry_points():
    header = open(os.path.join(ROOT, "include", "pfrl_amd.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    declared = set(re.findall(r"\b(pfrl_[a-z0-9_]+)\s*\(", header))
    for name in NAMES:
        assert name in declared and name in _native.EXPORTS and name in doc, name
    assert "td3.hip" in _native.SOURCES
    assert _native.EXPORTS["pfrl_td3_critic_loss"][1].count("p") == 9      # 8 pointers and the stream
