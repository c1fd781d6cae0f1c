"""The actor-critic half of the hot path -- PPO's categorical kernels of csrc/rollout.hip
(``pfrl_ppo_loss``, ``pfrl_ppo_head_loss``, ``pfrl_ppo_act_head``, ``pfrl_adv_stats``,
``pfrl_ppo_minibatch`` / ``_f32act``) and the SAC / TD3 helpers of csrc/actor.hip
(``pfrl_squashed_gaussian_fwd/_bwd``, ``pfrl_squashed_head_fwd/_bwd``, ``pfrl_sac_target_q``,
``pfrl_half_mse_*``, ``pfrl_sac_policy_loss_*``, ``pfrl_sac_temperature_loss/_step``) -- over what
their gates admit, through the C ABI, against references on the CPU: float64 torch with autograd on
the reference's own expressions (``PPO._lossfun`` on ``Categorical(logits=...)``;
``TransformedDistribution(Independent(Normal), [TanhTransform])`` behind the example head
``chunk / clamp / exp(2 .) / sqrt`` or ``exp``), or a float32 NumPy expression where the kernel's
arithmetic is a fixed sequence of IEEE operations (the library is built with ``-ffp-contract=off
-fno-fast-math``, ``_native.HIPCC_FLAGS``; a CPU test asserts it).  The method and helpers of
tests/test_loss_head_envelope.py: ``torch.equal`` where the arithmetic is fixed, a derived bound
elsewhere, ``RATIO`` lines per case, ``MAX RATIO <entry>`` lines after the last test (``pytest -s``),
every output / slab / workspace buffer between NaN guard zones of 4096 elements (int64 outputs between
sentinel zones).

u = 2^-24.  Every rounded bound below is first order and is asserted with a factor 2.

ASSUMPTIONS on the device math library (no accuracy table is installed with the compiler):
``expf`` / ``logf`` 1 ulp = 2 u relative (as rows a21-a24 assume), ``tanhf`` and ``log1pf`` 2 ulp = 4 u,
``sqrtf`` and the float32 / float64 division correctly rounded, ``expf(0) == 1`` and ``logf(1) == 0``.
The single-function cases (section 6) measure ``tanhf`` and ``log1pf(expf(.))`` on their own and
print the figure as ``MAX RATIO mathlib ...`` in ulp (observed on an MI355X: ``tanhf`` 0.93 ulp, the composite
1 ulp; the assumptions stand).

1. One row of ``PPO._lossfun`` (``ppo_loss_row``).  Logits z_j carry E_z,j (0 for ``pfrl_ppo_loss``;
   for the head kernels E_z = (K + 2) u sum_k |h w| + u |b|, row a24's E_y), v carries E_v likewise.
   With d_j = z_j - max, p = softmax(z), the relative error of e_j = expf(d_j) is
       eps_e,j = (2 + |d_j|) u + E_z,j          (1 ulp, the subtraction, the operand)
   (the maximum itself cancels in p and in the log-sum-exp), of the sum
       eps_S = sum_j p_j eps_e,j + (A - 1) u,
       E_lse = eps_S + 2 u |log sum| + u |lse|,     E_lp,j = E_z,j + E_lse + u |lp_j|,
       eps_p,j = eps_e,j + eps_S + u,
       E_H = sum_j p_j ((eps_p,j + u) |lp_j| + E_lp,j) + (A - 1) u sum_j p_j |lp_j|.
   Surrogate: x = lp_a - lp_old, ratio = expf(x) with eps_r = E_lp,a + u |x| + 2 u;
       E_surr = |adv| (ratio (eps_r + u) + 4 u)
   (the product; the clamp is continuous with slope <= 1, its bounds 1 -+ eps round once, the clipped
   product once more with rc < 2).  g_lpa = -(1 / M) ds ratio: eps_r + 3 u relative (1 / M rounds, two
   products), ds being exact away from the branch points.  The gradient
       g_j = g_lpa (1[j = a] - p_j) + (c_ent / M) p_j (lp_j + H):
       E_g,j = |g_lpa| ((eps_r + 5 u) |1[j = a] - p_j| + p_j eps_p,j)
             + (c_ent / M) p_j ((eps_p,j + 5 u) |lp_j + H| + E_lp,j + E_H) + u |g_j|.
   Value: d1 = v - vt, E_d1 = E_v + u |d1|, E_l1 = 2 |d1| E_d1 + u l1; clipped: vc = clip(v, vo -+ eps_vf),
   E_vc = E_v inside and u |vc| outside (the bound rounds once), E_d2 = E_vc + u |d2|,
   E_l2 = 2 |d2| E_d2 + u l2; E_gv = 2 max(E_d1, E_d2); dvalue = (c_vf / M) gv: |c_vf / M| (E_gv + 3 u |gv|).
   The three sums are float64 per workgroup and per launch: n 2^-53 relative, nothing measurable, so
   the partials are compared in float64 against sum E_row alone and the means carry only their cast:
       E_pol = mean E_surr + u |pol|, E_val = mean E_lv + u |val|, E_ent = mean E_H + u |ent|,
       E_loss = E_pol + c_vf (E_val + u val) + u |pol + c_vf val| + c_ent (E_ent + u |ent|) + u |loss|.
   Branch points: ratio within 2 (ratio eps_r + 2 u) of 1 -+ eps; v within 2 (E_v + u |bound|) of a value
   clip bound; v outside the clip range with |l2 - l1| <= 2 (E_l1 + E_l2).  Rows there are redrawn
   (lp_old, resp. v_old and v_teacher) until none is left; asserted on the reference, no row skipped.
   Exact cases: (i) v, v_old, v_teacher multiples of 1/2, eps_vf = 1/2, c_vf = 1/2, M a power of two --
   dvalue and out4[2] ``torch.equal``, with rows planted ON both clip bounds, inside, outside on both
   sides, on the equal-loss tie outside the range, and eps_vf = 0 with v == v_old (dL/dv(v = v_old = 1,
   vt = 3) = -2.5 c_vf / M: min(max()) halves twice); (ii) A = 1, lp_old = 0: dlogits zero, policy loss
   -mean(adv) on integer advantages, entropy 0, also with eps = 0 (ratio on both bounds at once).

2. ``pfrl_ppo_head_loss``: 1. with E_z, E_v; gg = (g_0 .. g_A-1, dvalue):
       dh: sum_j (E_gg,j + (A + 2) u |gg_j|) |w_j|,
       slab dW: sum over the slab's rows of (E_gg + (rpb + 4) u |gg|) |h|, db the same without h
   (fma chains per wave and the four waves' fold), the slab sums the sums of the slab bounds, the fold
   launch (S + 1) u sum |terms| on top.

3. ``pfrl_ppo_act_head``: value E_z, entropy E_H, log_prob E_lp,a of 1.  The draw compares u sum with
   the running sums of e: in units of the total, |cum_j / sum - cdf_j| <= 2 sum_k p_k eps_e,k + 2 (A + 2) u
   =: E_cdf; u is set to the middle of the target action's cdf interval (probability > 1e-3), whose
   half-width must exceed 2 E_cdf (asserted), so the action is determined for every row.

4. ``pfrl_adv_stats``: float64 sums, so integer operands give float32(mean) and
   float32(sqrt(max(b / n - mean^2, 0))) of the NumPy float64 expression bit for bit.  On randn, with
   at most 48 float64 additions per path: E_mean = u |mean| + 48 2^-53 mean|x|,
   E_var = 64 2^-53 (mean x^2 + mean^2), E_std = u std + min(E_var / (2 std), sqrt(E_var)).

5. Squashed Gaussian forward.  x = l + e s: E_xr = u |e s| + u |x|, E_x = E_xr + |e s| eps_s with
   eps_s = 0 for a given scale and 2 u for the head's s = sqrt(expf(2 c)) or expf(c).
       action: (1 - y^2) E_x + 4 u |y|                                  (tanhf 2 ulp)
       q = (x - l)^2 / (2 s^2) = e^2 / 2 (s cancels): E_q = |e| (E_xr + u |e s|) / s + 3 u q,
       E_nlp = E_q + 2 u |log s| + eps_s + u |q + log s| + u |nlp| + u c,
       sp = softplus(-2 x): sigma(-2 x) 2 E_x + 6 u sp (+ e^-z past the switch z > 20)
            (expf 1 ulp enters with sigma <= sp, log1pf 2 ulp),
       t = 2 (ln 2 - x - sp): E_t = 2 (E_x + u (ln 2 + |ln 2 - x|) + E_sp + u |ln 2 - x - sp|),
       logp: sum_a (E_t + E_nlp) + (ceil(A / 64) + 6) u sum_a (|t| + |nlp|) + u |logp|.
   Backward of ``k_squashed_gaussian_bwd`` is IEEE arithmetic on the kernel's own action: bit for bit a
   float32 NumPy restatement (itself checked against float64 autograd on the CPU).  The head's g_x
   passes through expf / sqrtf: with E_y the action bound, t = ga (1 - y^2),
       E_t = |ga| (2 |y| E_y + u) + 2 u |t|,   E_gloc = E_t + |gl| (2 E_y + 2 u |y|) + u |g_loc|,
       E_gs = |e| E_t + u |t e| + |gl| (2 |e| E_y + 2 u |y e| + (eps_s + u) / s + u |2 y e - 1 / s|) + u |g_s|,
       E_gc = s E_gs + 6 u |g_c|.
   The clamp mask is exact: log-scales at lo, hi and the floats next to them.

6. Single-function cases.  ``action`` at eps = 0 is tanhf(loc); ``logp`` at A = 1, eps = 0, scale = 1 is
   -2 (ln 2 - x - sp) - c in IEEE operations round sp = log1pf(expf(-2 x)) (or -2 x past the switch):
   the float32 restatement is evaluated at float32(sp64) +- k ulp and the smallest |k| that reproduces
   the kernel's bits is the observed error of the composite (expf 1 + log1pf 2 = 3 ulp assumed); one
   must match for every argument, which also pins the chain bit for bit.

7. SAC losses.  target_q, the MSE / policy gradients and the unit gradients are IEEE with a numeric
   temperature: bit for bit float32 NumPy.  A reduction is lane-strided (ceil(B / 256) - 1 additions),
   a butterfly (6), a four-way fold (2) and a division: with p roundings per term
       |err| <= (ceil(B / 256) + 9 + p) u sum |terms|;
   exact on terms that are multiples of 2^-4 with sums below 2^20 (both asserted).  With
   ``log_temperature`` the temperature is expf(.): 2 u relative, except expf(0) = 1.
   ``pfrl_sac_temperature_step``: loss bit for bit ``pfrl_sac_temperature_loss``; the state update bit
   for bit a NumPy restatement with double scalars and float32 element operations, itself pinned against
   ``torch.optim.Adam`` on the CPU.

Not tested, on purpose: NaN operands and actions outside [0, A) (a wild read).  The two largest
``pfrl_ppo_head_loss`` shapes run ``blocks`` in {1, the rule} only: M or M + 3 slabs of (A + 1) K floats
would be five times the largest buffer of the file.
"""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch
from torch.distributions import Categorical, Independent, Normal, TransformedDistribution
from torch.distributions.transforms import TanhTransform

from pfrl_amd import _native, ops
from pfrl_amd.nn import mfma_trunk as mt

gpu = pytest.mark.gpu

GUARD = 4096
U = 2.0 ** -24
PFRL_ERR_ARG = -2
LARGEST = 4099 * 512            # elements in the largest guarded buffer of any case
F32 = np.float32
F64 = torch.float64
_p, _stream, _cd = mt._p, mt._stream, mt._ceil_div
LN2, HALF_LOG_2PI = 0.6931471805599453, 0.9189385332046727
TANH_ULP, LOG1P_ULP, EXP_ULP = 2.0, 2.0, 1.0        # the assumptions (1 ulp = 2 u relative)
SOFTPLUS_ULP = LOG1P_ULP + EXP_ULP


# ------------------------------------------------------------------ helpers (copies of test_loss_head_envelope's)
class _Guarded:
    """n elements between two guard zones, everything NaN until a kernel writes it."""

    def __init__(self, n, dev, dtype=torch.float32):
        assert n <= LARGEST
        self.n, self.lo = n, GUARD
        self.full = torch.full((n + 2 * GUARD + 4,), float("nan"), dtype=dtype, device=dev)
        assert self.full.data_ptr() % 16 == 0
        self.t = self.full[self.lo:self.lo + n]

    def guards(self, what=""):
        assert bool(torch.isnan(self.full[:self.lo]).all()), "guard zone before %s was written" % what
        assert bool(torch.isnan(self.full[self.lo + self.n:]).all()), "guard zone after %s was written" % what
        return self.t

    def done(self, what=""):
        self.guards(what)
        assert not bool(torch.isnan(self.t).any()), "%s: payload not fully written" % what
        return self.t

    def untouched(self, what=""):
        assert bool(torch.isnan(self.full).all()), "%s was written" % what


class _GuardedInt:
    """The same for integer outputs: a sentinel no kernel writes instead of NaN."""

    def __init__(self, n, dev, dtype=torch.int64):
        self.n = n
        self.MARK = -(1 << 62) if dtype == torch.int64 else -(1 << 30)
        self.full = torch.full((n + 2 * GUARD,), self.MARK, dtype=dtype, device=dev)
        self.t = self.full[GUARD:GUARD + n]

    def guards(self, what=""):
        assert bool((self.full[:GUARD] == self.MARK).all()) and bool((self.full[GUARD + self.n:] == self.MARK).all()), \
            "guard zone round %s was written" % what
        return self.t

    def done(self, what=""):
        self.guards(what)
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


def _note(name, tag, ratio):
    _RATIO[name] = max(_RATIO.get(name, 0.0), ratio)
    print("RATIO %s %s %.4f" % (name, tag, ratio))


def _within(name, tag, out, ref, bound):
    """|out - ref| <= bound per element (bound already carries the factor 2)."""
    ref = ref.detach()
    out = out.detach().cpu().double().reshape(ref.shape)
    bound = bound.detach().expand_as(ref)
    err = (out - ref).abs()
    ratio = float((err / bound.clamp(min=1e-300)).max()) if ref.numel() else 0.0
    _note(name, tag, ratio)
    assert bool((err <= bound).all()), "%s %s: err / bound = %.3f" % (name, tag, ratio)


def _same(name, tag, out, want):
    out = out.detach().cpu().reshape(want.shape)
    assert out.dtype == want.dtype, (name, out.dtype, want.dtype)
    if not torch.equal(out, want):
        bad = (out != want).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError("%s %s: %d elements differ, first at %s: got %r, want %r" % (
            name, tag, len(bad), i, float(out[i]), float(want[i])))


def _dev():
    return torch.device("cuda:0")


def _f(x):
    """A Python float that float32 holds exactly: what the kernel receives IS what the reference uses."""
    return float(F32(x))


def _np(t):
    return t.detach().cpu().numpy()


def _spread(first, second):
    return [(a, b) for i, a in enumerate(first) for j, b in enumerate(second) if (i + j) % 3 == 0]


def _ulp32(x64):
    """Spacing of float32 at |x| (float64 tensor)."""
    a = x64.abs().clamp(min=2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 23)


# ================================================================== 1. one row of PPO._lossfun
CE = _f(0.2)
VF = _f(0.7)
PPO_SWITCHES = [(cev, ec) for cev in (None, _f(0.2), 0.5) for ec in (0.0, _f(0.02))]


def lossfun64(z, v, o, ce, cev, vf, ec):
    """PPO._lossfun on Categorical(logits=z) in float64 + autograd.  -> dict: out4, dz, dv and the rows'
    three terms (-surrogate, value loss, entropy)."""
    z = z.detach().clone().requires_grad_(True)
    v = v.detach().clone().requires_grad_(True)
    dist = Categorical(logits=z)
    lpa, ent = dist.log_prob(o["action"]), dist.entropy()
    lpo, adv, vo, vt = (o[k].double() for k in ("lpo", "adv", "vo", "vt"))
    ratio = torch.exp(lpa - lpo)
    surr = torch.min(ratio * adv, torch.clamp(ratio, 1 - ce, 1 + ce) * adv)
    pol = -torch.mean(surr)
    if cev is None:
        lv = (v - vt) ** 2
    else:
        vc = torch.min(torch.max(v, vo - cev), vo + cev)
        lv = torch.max((v - vt) ** 2, (vc - vt) ** 2)
    val, entm = torch.mean(lv), torch.mean(ent)
    loss = pol + vf * val + ec * (-entm)
    dz, dv = torch.autograd.grad(loss, [z, v])
    return {"out4": torch.stack([loss, pol, val, entm]).detach(), "dz": dz, "dv": dv,
            "rows": torch.stack([-surr, lv, ent], 1).detach()}


def ppo_bounds(z, v, o, ce, cev, vf, ec, r, Ez=None, Ev=None):
    """First-order bounds of section 1 (without the factor 2) and the rows near a branch point."""
    z, v = z.detach(), v.detach()
    M, A = z.shape
    Ez = torch.zeros_like(z) if Ez is None else Ez
    Ev = torch.zeros_like(v) if Ev is None else Ev
    ar = torch.arange(M)
    a = o["action"]
    lpo, adv, vo, vt = (o[k].double() for k in ("lpo", "adv", "vo", "vt"))
    mx = z.max(1, keepdim=True).values
    lse = torch.logsumexp(z, 1, keepdim=True)
    lp = z - lse
    p = lp.exp()
    eps_e = (2 + (z - mx).abs()) * U + Ez
    eps_S = (p * eps_e).sum(1, keepdim=True) + (A - 1) * U
    E_lse = eps_S + 2 * U * (lse - mx).abs() + U * lse.abs()
    E_lp = Ez + E_lse + U * lp.abs()
    eps_p = eps_e + eps_S + U
    H = -(p * lp).sum(1, keepdim=True)
    E_H = (p * ((eps_p + U) * lp.abs() + E_lp)).sum(1, keepdim=True) + (A - 1) * U * (p * lp.abs()).sum(1, keepdim=True)
    x = lp[ar, a] - lpo
    ratio = x.exp()
    eps_r = E_lp[ar, a] + U * x.abs() + 2 * U
    E_surr = adv.abs() * (ratio * (eps_r + U) + 4 * U)
    near_r = torch.zeros(M, dtype=torch.bool)
    for b in (1 - ce, 1 + ce):
        near_r |= (ratio - b).abs() <= 2 * (ratio * eps_r + 2 * U)
    inside = (ratio >= 1 - ce) & (ratio <= 1 + ce)
    s1, s2 = ratio * adv, ratio.clamp(1 - ce, 1 + ce) * adv
    ds = torch.where(inside | (s1 < s2), adv, torch.zeros_like(adv))
    g_lpa = -ds * ratio / M
    oh = torch.zeros_like(z)
    oh[ar, a] = 1.0
    ge = ec / M
    E_g = (g_lpa.abs()[:, None] * ((eps_r[:, None] + 5 * U) * (oh - p).abs() + p * eps_p)
           + ge * p * ((eps_p + 5 * U) * (lp + H).abs() + E_lp + E_H) + U * r["dz"].abs())
    d1 = v - vt
    E_d1 = Ev + U * d1.abs()
    l1 = d1 * d1
    E_l1 = 2 * d1.abs() * E_d1 + U * l1
    near_v = torch.zeros(M, dtype=torch.bool)
    if cev is None:
        E_lv, E_gv = E_l1, 2 * E_d1
    else:
        vlo, vhi = vo - cev, vo + cev
        vc = torch.min(torch.max(v, vlo), vhi)
        ins = (v > vlo) & (v < vhi)
        E_vc = torch.where(ins, Ev, U * vc.abs())
        d2 = vc - vt
        E_d2 = E_vc + U * d2.abs()
        l2 = d2 * d2
        E_l2 = 2 * d2.abs() * E_d2 + U * l2
        E_lv = torch.where(l2 > l1, E_l2, E_l1)
        E_gv = 2 * torch.max(E_d1, E_d2)
        near_v = ((v - vlo).abs() <= 2 * (Ev + U * vlo.abs())) | ((v - vhi).abs() <= 2 * (Ev + U * vhi.abs()))
        near_v |= ~ins & ((l2 - l1).abs() <= 2 * (E_l1 + E_l2))
    c = vf / M
    gv = r["dv"] / c
    E_dv = c * (E_gv + 3 * U * gv.abs())
    o4 = r["out4"]
    E_pol = E_surr.mean() + U * o4[1].abs()
    E_val = E_lv.mean() + U * o4[2].abs()
    E_ent = E_H.mean() + U * o4[3].abs()
    E_loss = (E_pol + vf * (E_val + U * o4[2].abs()) + U * (o4[1] + vf * o4[2]).abs()
              + ec * (E_ent + U * o4[3].abs()) + U * o4[0].abs())
    return {"dz": E_g, "dv": E_dv, "rows": torch.stack([E_surr, E_lv, E_H[:, 0]], 1),
            "out4": torch.stack([E_loss, E_pol, E_val, E_ent]), "near_r": near_r, "near_v": near_v,
            "lp_a": E_lp[ar, a], "H": E_H[:, 0], "eps_e": eps_e, "p": p}


def _draw_ppo(g, M, A):
    return {"action": torch.randint(0, A, (M,), generator=g), "adv": torch.randn(M, generator=g),
            "lpo": torch.zeros(M), "vo": torch.randn(M, generator=g), "vt": torch.randn(M, generator=g)}


def _settle(g, z, v, o, Ez=None, Ev=None):
    """Redraw lp_old / v_old / v_teacher of the rows near a branch point of ANY switch setting until none
    is left; the reference itself says so at the end."""
    M = z.shape[0]
    ar = torch.arange(M)
    lpa = (z - torch.logsumexp(z, 1, keepdim=True))[ar, o["action"]]
    o["lpo"] = (lpa + 0.3 * torch.randn(M, generator=g, dtype=F64)).float()
    o["vo"] = (v + 0.3 * torch.randn(M, generator=g, dtype=F64)).float()
    for _ in range(100):
        near_r, near_v = torch.zeros(M, dtype=torch.bool), torch.zeros(M, dtype=torch.bool)
        for cev in (None, _f(0.2), 0.5):
            r = lossfun64(z, v, o, CE, cev, VF, 0.0)
            b = ppo_bounds(z, v, o, CE, cev, VF, 0.0, r, Ez, Ev)
            near_r |= b["near_r"]
            near_v |= b["near_v"]
        if not bool(near_r.any() | near_v.any()):
            return
        nr, nv = int(near_r.sum()), int(near_v.sum())
        o["lpo"][near_r] = (lpa[near_r] + 0.3 * torch.randn(nr, generator=g, dtype=F64)).float()
        o["vo"][near_v] = (v[near_v] + 0.3 * torch.randn(nv, generator=g, dtype=F64)).float()
        o["vt"][near_v] = torch.randn(nv, generator=g)
    raise AssertionError("rows near a branch point remain")


def _dev_o(o, dev):
    return {k: t.to(dev).contiguous() for k, t in o.items()}


# ================================================================== 1a. pfrl_ppo_loss
LOSS_M = [1, 2, 63, 64, 255, 256, 257, 1000]
LOSS_A = list(range(1, 32))


def _loss_shapes():
    return _spread(LOSS_M, LOSS_A) + [(4099, 6), (4099, 31)]


class _LossCase:
    def __init__(self, M, A):
        g = torch.Generator().manual_seed(104729 * M + A)
        self.M, self.A = M, A
        self.z32 = 2 * torch.randn(M, A, generator=g)
        self.v32 = torch.randn(M, generator=g)
        self.z, self.v = self.z32.double(), self.v32.double()
        self.o = _draw_ppo(g, M, A)
        _settle(g, self.z, self.v, self.o)


def _run_loss(dev, z, v, o, M, A, ce, cev, vf, ec):
    nb = _cd(M, 256)
    out = {"dz": _Guarded(M * A, dev), "dv": _Guarded(M, dev), "ws": _Guarded(3 * nb, dev, F64), "out4": _Guarded(4, dev)}
    mt.check(_native.lib().pfrl_ppo_loss(
        _p(z), _p(v), _p(o["action"]), _p(o["adv"]), _p(o["lpo"]), _p(o["vo"]) if cev is not None else None,
        _p(o["vt"]), M, A, ce, -1.0 if cev is None else cev, vf, ec, _p(out["dz"].t), _p(out["dv"].t),
        _p(out["ws"].t), _p(out["out4"].t), _stream()), "ppo_loss")
    return {k: t.done(k) for k, t in out.items()}


def test_ppo_loss_case_lists_reach_every_instantiation():
    """No GPU: the pruned matrix holds all 31 widths and every M of the list, both big shapes; the switch
    list both value-loss forms and both entropy settings."""
    shapes = _loss_shapes()
    assert {A for _, A in shapes} == set(range(1, 32))
    assert {M for M, _ in shapes} == set(LOSS_M) | {4099}
    assert (4099, 6) in shapes and (4099, 31) in shapes
    assert {cev for cev, _ in PPO_SWITCHES} == {None, _f(0.2), 0.5} and {ec for _, ec in PPO_SWITCHES} == {0.0, _f(0.02)}


def test_redraw_leaves_no_row_near_a_branch_point():
    """No GPU: after the redraw loop the reference reports no row near 1 -+ eps, a value clip bound or an
    equal-loss tie, for every switch setting; well under 1 % of randn rows had to be redrawn."""
    c = _LossCase(1000, 6)
    for cev, ec in PPO_SWITCHES:
        r = lossfun64(c.z, c.v, c.o, CE, cev, VF, ec)
        b = ppo_bounds(c.z, c.v, c.o, CE, cev, VF, ec, r)
        assert not bool(b["near_r"].any()) and not bool(b["near_v"].any())


@gpu
@pytest.mark.parametrize("shape", _loss_shapes(), ids=lambda s: "M%d-A%d" % s)
def test_ppo_loss_matches_float64(shape):
    dev = _dev()
    M, A = shape
    c = _LossCase(M, A)
    z, v, o = c.z32.to(dev), c.v32.to(dev), _dev_o(c.o, dev)
    nb = _cd(M, 256)
    for cev, ec in PPO_SWITCHES:
        tag = "M%d-A%d-vf%s-ent%g" % (M, A, cev, ec)
        r = lossfun64(c.z, c.v, c.o, CE, cev, VF, ec)
        b = ppo_bounds(c.z, c.v, c.o, CE, cev, VF, ec, r)
        assert not bool(b["near_r"].any()) and not bool(b["near_v"].any())
        got = _run_loss(dev, z, v, o, M, A, CE, cev, VF, ec)
        _within("ppo_loss dlogits", tag, got["dz"], r["dz"], 2 * b["dz"])
        _within("ppo_loss dvalue", tag, got["dv"], r["dv"], 2 * b["dv"])
        _within("ppo_loss out4", tag, got["out4"], r["out4"], 2 * b["out4"])
        idx = torch.arange(M) // 256
        want = torch.zeros(nb, 3, dtype=F64).index_add_(0, idx, r["rows"])
        E = torch.zeros(nb, 3, dtype=F64).index_add_(0, idx, b["rows"])
        _within("ppo_loss partials", tag, got["ws"].view(nb, 3), want, 2 * E + 1e-300)


VALUE_KINDS = ["on lower bound", "on upper bound", "inside", "below", "above", "equal losses outside"]


def _value_case(M, zero_clip):
    """Operands of exact case (i): multiples of 1/2, the planted rows first."""
    g = torch.Generator().manual_seed(31 * M + int(zero_clip))

    def half(n):
        return torch.randint(-6, 7, (n,), generator=g).float() * 0.5
    v, vo, vt = half(M), half(M), half(M)
    if zero_clip:
        plant = [(1.0, 1.0, 3.0), (1.0, 1.0, -2.0), (1.5, 1.0, 3.0), (0.5, 1.0, 0.5)]
    else:
        plant = [(0.5, 1.0, 3.0), (1.5, 1.0, 3.0), (1.0, 1.0, 3.0), (-0.5, 1.0, 3.0), (3.0, 1.0, -1.0),
                 (2.5, 0.0, 1.5), (-2.5, 0.0, -1.5), (1.0, 1.5, 1.0), (1.0, 0.5, -1.0)]
    for i, (a, b, c) in enumerate(plant[:M]):
        v[i], vo[i], vt[i] = a, b, c
    o = _draw_ppo(g, M, 2)
    o["vo"], o["vt"] = vo, vt
    return 2 * torch.randn(M, 2, generator=g), v, o


def value_kinds(v, o, cev):
    v, vo, vt = v.double(), o["vo"].double(), o["vt"].double()
    vc = torch.min(torch.max(v, vo - cev), vo + cev)
    out = (v < vo - cev) | (v > vo + cev)
    kinds = {"on lower bound": v == vo - cev, "on upper bound": v == vo + cev, "inside": (v > vo - cev) & (v < vo + cev),
             "below": v < vo - cev, "above": v > vo + cev,
             "equal losses outside": out & ((vc - vt) ** 2 == (v - vt) ** 2) & (v != vt)}
    return {k for k, m in kinds.items() if bool(m.any())}


def test_exact_value_cases_hold_every_planted_row_and_the_measured_gradients():
    """No GPU: the planted rows are present, and float64 autograd gives them the gradients this file's
    header quotes: -2.5 c / M for eps_vf = 0 with v = v_old = 1, vt = 3 (two halvings), d1 c / M on the
    equal-loss tie outside the range, 1.5 (v - vt) c / M on a clip bound when both losses are equal there."""
    for M in (16, 64):
        z, v, o = _value_case(M, False)
        assert value_kinds(v, o, 0.5) == set(VALUE_KINDS)
        r = lossfun64(z.double(), v.double(), o, CE, 0.5, 0.5, 0.0)
        c = 0.5 / M
        # row 0: v on the lower bound, vc = v: both losses equal, dvc = 1/2: 1/2 2 d1 + 1/2 2 d1 1/2 = 1.5 d1
        assert float(r["dv"][0]) == c * 1.5 * (0.5 - 3.0) and float(r["dv"][1]) == c * 1.5 * (1.5 - 3.0)
        assert float(r["dv"][2]) == c * 2 * (1.0 - 3.0)
        assert float(r["dv"][5]) == c * (2.5 - 1.5)         # tie outside: half of 2 d1, the clipped branch has no slope
        z, v, o = _value_case(M, True)
        assert bool(((v == o["vo"]).sum() >= 2)) and bool((v != o["vo"]).any())
        r = lossfun64(z.double(), v.double(), o, CE, 0.0, 0.5, 0.0)
        assert float(r["dv"][0]) == c * -2.5 and float(r["dv"][1]) == c * 2.5 * 1.5


@gpu
@pytest.mark.parametrize("zero_clip", [False, True], ids=["eps_vf-0.5", "eps_vf-0"])
@pytest.mark.parametrize("M", [1, 16, 64, 1024])
def test_ppo_loss_value_path_is_exact_on_half_integers(M, zero_clip):
    dev = _dev()
    cev = 0.0 if zero_clip else 0.5
    z, v, o = _value_case(M, zero_clip)
    if M >= 16 and not zero_clip:
        assert value_kinds(v, o, cev) == set(VALUE_KINDS)
    r = lossfun64(z.double(), v.double(), o, CE, cev, 0.5, 0.0)
    got = _run_loss(dev, z.to(dev), v.to(dev), _dev_o(o, dev), M, 2, CE, cev, 0.5, 0.0)
    tag = "M%d-eps_vf%g" % (M, cev)
    _same("ppo_loss exact dvalue", tag, got["dv"], r["dv"].float())
    _same("ppo_loss exact value loss", tag, got["out4"][2:3], r["out4"][2:3].float())


@gpu
@pytest.mark.parametrize("ce", [CE, 0.0], ids=["eps0.2", "eps0"])
@pytest.mark.parametrize("M", [1, 64, 257])
def test_ppo_loss_with_one_action_is_exact(M, ce):
    dev = _dev()
    g = torch.Generator().manual_seed(M)
    z, v = 3 * torch.randn(M, 1, generator=g), torch.randn(M, generator=g)
    o = _draw_ppo(g, M, 1)
    o["adv"] = torch.randint(-4, 5, (M,), generator=g).float()
    r = lossfun64(z.double(), v.double(), o, ce, None, VF, _f(0.02))
    assert not bool(r["dz"].any()) and float(r["out4"][1]) == -float(o["adv"].double().mean()) and float(r["out4"][3]) == 0
    got = _run_loss(dev, z.to(dev), v.to(dev), _dev_o(o, dev), M, 1, ce, None, VF, _f(0.02))
    _same("ppo_loss A=1 dlogits", "M%d" % M, got["dz"], torch.zeros(M))
    _same("ppo_loss A=1 policy loss", "M%d" % M, got["out4"][1:2], r["out4"][1:2].float())
    _same("ppo_loss A=1 entropy", "M%d" % M, got["out4"][3:4], torch.zeros(1))


# ================================================================== 2. pfrl_ppo_head_loss
HEAD_M = [1, 2, 3, 4, 5, 7, 8, 9, 33, 37]
HEAD_BIG = [(4099, 256, 4), (2048, 512, 9)]


def _head_cases():
    inst = [(A, K) for A in range(1, 10) for K in (256, 512)]
    return [(HEAD_M[i % len(HEAD_M)], K, A) for i, (A, K) in enumerate(inst)] + HEAD_BIG


def _head_blocks(M, big):
    rule = min(512, (M + 7) // 8)
    return sorted({1, rule} if big else {1, rule, M, M + 3})


class _HeadCase:
    def __init__(self, M, K, A):
        g = torch.Generator().manual_seed(7919 * M + 31 * A + K)
        self.M, self.K, self.A = M, K, A
        self.h = torch.randn(M, K, generator=g)
        self.w = torch.randn(A + 1, K, generator=g) * (2.0 / math.sqrt(K))
        self.b = torch.randn(A + 1, generator=g)
        H, W, Bi = self.h.double(), self.w.double(), self.b.double()
        zz = H @ W.t() + Bi
        Ezz = (K + 2) * U * (H.abs() @ W.abs().t()) + U * Bi.abs()
        self.z, self.v, self.Ez, self.Ev = zz[:, :A].contiguous(), zz[:, A].contiguous(), Ezz[:, :A], Ezz[:, A]
        self.o = _draw_ppo(g, M, A)
        _settle(g, self.z, self.v, self.o, self.Ez, self.Ev)


def _run_head_loss(dev, t, M, K, A, blocks, cev, ec, h=None, dh=None, vo="given"):
    """t: device operands.  -> the guarded buffers (not yet checked)."""
    NO = A + 1
    stride = NO * K + (NO + 3) // 4 * 4
    out = {"dh": _Guarded(M * K, dev), "part": _Guarded(max(blocks, 1) * stride, dev),
           "ws": _Guarded(3 * max(blocks, 1), dev, F64), "out4": _Guarded(4, dev)}
    o = t["o"]
    vo_p = _p(o["vo"]) if (cev is not None and vo == "given") else None
    rc = _native.lib().pfrl_ppo_head_loss(
        h if h is not None else _p(t["h"]), _p(t["w"][:A]), _p(t["b"][:A]), _p(t["w"][A:]), _p(t["b"][A:]), _p(o["action"]),
        _p(o["adv"]), _p(o["lpo"]), vo_p, _p(o["vt"]), M, K, A, CE, -1.0 if cev is None else cev, VF, ec,
        dh if dh is not None else _p(out["dh"].t), _p(out["part"].t), blocks, _p(out["ws"].t), _p(out["out4"].t), _stream())
    return rc, out


def test_head_case_lists_reach_all_18_instantiations_and_the_gate_contains_the_python_gate():
    """No GPU: every (A, K) of k_ppo_head_loss<1..9, 1|2>, every M of the list, the two big shapes; block
    counts 1 / the rule / M / M + 3 (so workgroups past the last row exist); ``ops.ppo_head_loss_ok`` admits
    nothing the C gate (1 <= A <= 9, K in {256, 512}, M >= 1) refuses."""
    cases = _head_cases()
    assert {(A, K) for _, K, A in cases} == {(A, K) for A in range(1, 10) for K in (256, 512)}
    assert {M for M, _, _ in cases} >= set(HEAD_M) and set(HEAD_BIG) <= set(cases)
    for M, K, A in cases:
        bl = _head_blocks(M, (M, K, A) in HEAD_BIG)
        assert 1 in bl and min(512, (M + 7) // 8) in bl
        if (M, K, A) not in HEAD_BIG:
            assert M in bl and M + 3 in bl
        assert max(bl) * ((A + 1) * K + 12) <= LARGEST and M * K <= LARGEST
    admitted = set()
    for K in (1, 128, 255, 256, 257, 384, 512, 513, 1024):
        for A in range(0, 12):
            if ops.ppo_head_loss_ok(_Shaped((3, K)), _Shaped((A, K))):
                assert 1 <= A <= 9 and K in (256, 512), (A, K)
                admitted.add((A, K))
    assert admitted == {(A, K) for A in range(1, 10) for K in (256, 512)}      # the containment is not vacuous
    assert not ops.ppo_head_loss_ok(_Shaped((3, 256), cuda=False), _Shaped((4, 256)))


class _Shaped:
    """What ``ops.ppo_head_loss_ok`` looks at, without a device."""

    def __init__(self, shape, dtype=torch.float32, cuda=True):
        self.shape, self.dtype, self.is_cuda = shape, dtype, cuda

    def dim(self):
        return len(self.shape)


@gpu
@pytest.mark.parametrize("case", _head_cases(), ids=lambda c: "M%d-K%d-A%d" % c)
def test_ppo_head_loss_matches_float64_per_slab(case):
    dev = _dev()
    M, K, A = case
    NO = A + 1
    c = _HeadCase(M, K, A)
    t = {"h": c.h.to(dev), "w": c.w.to(dev).contiguous(), "b": c.b.to(dev), "o": _dev_o(c.o, dev)}
    H, W = c.h.double(), c.w.double()
    stride = NO * K + (NO + 3) // 4 * 4
    switches = [(None, _f(0.02)), (_f(0.2), 0.0), (0.5, _f(0.02))]
    for si, (cev, ec) in enumerate(switches):
        r = lossfun64(c.z, c.v, c.o, CE, cev, VF, ec)
        b = ppo_bounds(c.z, c.v, c.o, CE, cev, VF, ec, r, c.Ez, c.Ev)
        assert not bool(b["near_r"].any()) and not bool(b["near_v"].any())
        gg = torch.cat([r["dz"], r["dv"][:, None]], 1)                      # [M, NO]
        Egg = torch.cat([b["dz"], b["dv"][:, None]], 1)
        dh, E_dh = gg @ W, (Egg + (A + 2) * U * gg.abs()) @ W.abs()
        blocks_list = _head_blocks(M, case in HEAD_BIG)
        for blocks in (blocks_list if si == 0 else blocks_list[1:2] or blocks_list[:1]):
            tag = "M%d-K%d-A%d-vf%s-ent%g-blocks%d" % (M, K, A, cev, ec, blocks)
            rpb = _cd(M, blocks)
            rc, out = _run_head_loss(dev, t, M, K, A, blocks, cev, ec)
            mt.check(rc, "ppo_head_loss")
            _within("ppo_head_loss out4", tag, out["out4"].done("out4"), r["out4"], 2 * b["out4"])
            _within("ppo_head_loss dh", tag, out["dh"].done("dh"), dh.reshape(-1), 2 * E_dh.reshape(-1))
            # per slab: the reference restricted to the rows [b rpb, min((b + 1) rpb, M))
            idx = torch.arange(M) // rpb

            def slabs(rows):
                return torch.zeros((blocks,) + tuple(rows.shape[1:]), dtype=F64).index_add_(0, idx, rows)
            Erow = Egg + (rpb + 4) * U * gg.abs()
            dW, E_dW = slabs(gg[:, :, None] * H[:, None, :]), slabs(Erow[:, :, None] * H.abs()[:, None, :])
            db, E_db = slabs(gg), slabs(Erow)
            pv = out["part"].guards("slabs").view(blocks, stride).cpu()
            assert bool(torch.isnan(pv[:, NO * K + NO:]).all()), "the padding behind the bias block was written"
            assert not bool(torch.isnan(pv[:, :NO * K + NO]).any())
            _within("ppo_head_loss slab dW", tag, pv[:, :NO * K], dW.view(blocks, NO * K), 2 * E_dW.view(blocks, NO * K))
            _within("ppo_head_loss slab db", tag, pv[:, NO * K:NO * K + NO], db, 2 * E_db)
            ws = out["ws"].done("partials").view(blocks, 3).cpu()
            _within("ppo_head_loss slab partials", tag, ws, slabs(r["rows"]), 2 * slabs(b["rows"]) + 1e-300)
            empty = torch.arange(blocks) * rpb >= M
            if bool(empty.any()):
                assert not bool(pv[empty][:, :NO * K + NO].any()) and not bool(ws[empty].any()), \
                    "%s: a workgroup past the last row wrote something other than zeros" % tag
            # the slab sums, and the fold as ops.ppo_head_loss issues it
            A_dW, A_db = slabs(gg.abs()[:, :, None] * H.abs()[:, None, :]).sum(0), slabs(gg.abs()).sum(0)
            tot_dW, tot_db = dW.sum(0).view(-1), db.sum(0)
            Et_dW, Et_db = E_dW.sum(0).view(-1), E_db.sum(0)
            _within("ppo_head_loss slab sum dW", tag, pv[:, :NO * K].double().sum(0), tot_dW, 2 * Et_dW)
            _within("ppo_head_loss slab sum db", tag, pv[:, NO * K:NO * K + NO].double().sum(0), tot_db, 2 * Et_db)
            part = out["part"].t
            f = {"dwp": _Guarded(A * K, dev), "dbp": _Guarded(A, dev), "dwv": _Guarded(K, dev), "dbv": _Guarded(1, dev)}
            mt._reduce([(part, f["dwp"].t, None, stride, A * K, blocks, 4, 0),
                        (part[A * K:], f["dwv"].t, None, stride, K, blocks, 4, 0),
                        (part[NO * K:], f["dbp"].t, None, stride, A, blocks, 1, 0),
                        (part[NO * K + A:], f["dbv"].t, None, stride, 1, blocks, 1, 0)])
            fold_w = Et_dW + (blocks + 1) * U * A_dW.view(-1)
            fold_b = Et_db + (blocks + 1) * U * A_db
            _within("ppo_head_loss folded dWp", tag, f["dwp"].done("dwp"), tot_dW[:A * K], 2 * fold_w[:A * K])
            _within("ppo_head_loss folded dWv", tag, f["dwv"].done("dwv"), tot_dW[A * K:], 2 * fold_w[A * K:])
            _within("ppo_head_loss folded dbp", tag, f["dbp"].done("dbp"), tot_db[:A], 2 * fold_b[:A])
            _within("ppo_head_loss folded dbv", tag, f["dbv"].done("dbv"), tot_db[A:], 2 * fold_b[A:])


HEAD_GATES = ["A0", "A10", "K128", "K384", "M0", "blocks0", "h+4", "dh+4", "v_old NULL"]


@gpu
@pytest.mark.parametrize("gate", HEAD_GATES)
def test_ppo_head_loss_refuses_what_its_gate_excludes(gate):
    dev = _dev()
    M, K, A = 8, 256, 4
    g = torch.Generator().manual_seed(5)
    t = {"h": torch.randn(M + 1, 512, generator=g).to(dev), "w": torch.randn(11, 512, generator=g).to(dev),
         "b": torch.randn(11, generator=g).to(dev), "o": _dev_o(_draw_ppo(g, M, 2), dev)}
    kw, blocks, cev = {}, 1, None
    if gate == "A0":
        A = 0
    elif gate == "A10":
        A = 10
    elif gate == "K128":
        K = 128
    elif gate == "K384":
        K = 384
    elif gate == "M0":
        M = 0
    elif gate == "blocks0":
        blocks = 0
    elif gate == "h+4":
        kw["h"] = ctypes.c_void_p(t["h"].data_ptr() + 4)
    elif gate == "v_old NULL":
        cev, kw["vo"] = 0.0, "NULL"
    spare = _Guarded(M * K + 8, dev)
    if gate == "dh+4":
        kw["dh"] = ctypes.c_void_p(spare.t.data_ptr() + 4)
    rc, out = _run_head_loss(dev, t, M, K, max(A, 0), blocks, cev, 0.0, **kw)
    assert rc == PFRL_ERR_ARG, (gate, rc)
    torch.cuda.synchronize()
    spare.untouched("dh")
    for k, buf in out.items():
        buf.untouched(k)


# ================================================================== 3. pfrl_ppo_act_head
ACT_NK = [(1, 1), (3, 63), (4, 64), (5, 65), (37, 127), (64, 128), (9, 129), (130, 512)]
ACT_MODES = ["sample", "given", "values"]


def _act_cases():
    return [(N, K, A) for (A, (N, K)) in _spread(list(range(1, 32)), ACT_NK)]


def test_act_head_case_list_reaches_every_width_and_every_k_tail():
    """No GPU: all 31 widths; every (N, K) of the list, with K < 64, K % 128 in {63, 64, 65, 127, 0, 1} and a
    last workgroup of 1, 2 and 3 absent rows; three modes."""
    cases = _act_cases()
    assert {A for _, _, A in cases} == set(range(1, 32))
    assert {(N, K) for N, K, _ in cases} == set(ACT_NK)
    assert {K for _, K in ACT_NK} == {1, 63, 64, 65, 127, 128, 129, 512} and {N % 4 for N, _ in ACT_NK} == {0, 1, 2, 3}
    assert ACT_MODES == ["sample", "given", "values"]


def _act_ref(z, Ez, N, A):
    """float64 entropy / log-probabilities, the bounds of section 3 and a draw per row that is determined."""
    dist = Categorical(logits=z)
    lp = dist.logits
    p = dist.probs
    zero = torch.zeros(N, dtype=F64)
    o = {"action": torch.zeros(N, dtype=torch.int64), "adv": zero.float(), "lpo": zero.float(), "vo": zero.float(), "vt": zero.float()}
    r0 = {"dz": torch.zeros_like(z), "dv": torch.ones(N, dtype=F64), "out4": torch.zeros(4, dtype=F64)}
    b = ppo_bounds(z, zero, o, CE, None, 1.0, 0.0, r0, Ez, zero)
    mx = z.max(1, keepdim=True).values
    lse = torch.logsumexp(z, 1, keepdim=True)
    eps_S = (p * b["eps_e"]).sum(1, keepdim=True) + (A - 1) * U
    E_lp = Ez + eps_S + 2 * U * (lse - mx).abs() + U * lse.abs() + U * lp.abs()
    E_cdf = 2 * (p * b["eps_e"]).sum(1) + 2 * (A + 2) * U
    cdf = torch.cumsum(p, 1)
    target, u = torch.zeros(N, dtype=torch.int64), torch.zeros(N, dtype=F64)
    for i in range(N):
        # among the actions with p > 1e-3, those whose interval is wide enough for the row's bound (the most
        # probable one, p >= 1 / 31, always is; at K = 512 the worst-case E_z leaves out the narrowest)
        live = ((p[i] > 1e-3) & (0.5 * p[i] > 4 * E_cdf[i])).nonzero().view(-1)
        assert len(live) >= 1
        j = int(live[i % len(live)])
        lo = float(cdf[i, j - 1]) if j > 0 else 0.0
        hi = float(cdf[i, j]) if j < A - 1 else 1.0
        target[i], u[i] = j, 0.5 * (lo + hi)
        assert 0.5 * (hi - lo) > 2 * float(E_cdf[i]), "the cdf interval of the target action is too narrow"
    return {"lp": lp, "E_lp": E_lp, "ent": dist.entropy(), "E_H": b["H"], "target": target, "u": u.float()}


def _run_act(dev, h, w, b, N, K, A, u=None, given=None, want_ent=True, want_lp=True, want_action=True, room=None):
    room = N if room is None else room
    out = {"action": _GuardedInt(room, dev), "ent": _Guarded(room, dev), "value": _Guarded(room, dev), "lp": _Guarded(room, dev)}
    rc = _native.lib().pfrl_ppo_act_head(
        _p(h), _p(w[:A]), _p(b[:A]), _p(w[A:]), _p(b[A:]), _p(u), _p(given), _p(out["action"].t) if want_action else None,
        _p(out["ent"].t) if want_ent else None, _p(out["value"].t), _p(out["lp"].t) if want_lp else None, N, K, A, None, _stream())
    return rc, out


@gpu
@pytest.mark.parametrize("case", _act_cases(), ids=lambda c: "N%d-K%d-A%d" % c)
def test_ppo_act_head_matches_float64_in_all_three_modes(case):
    dev = _dev()
    N, K, A = case
    g = torch.Generator().manual_seed(1009 * N + 31 * K + A)
    h = torch.randn(N, K, generator=g)
    w = torch.randn(A + 1, K, generator=g) * (2.0 / math.sqrt(K))
    b = torch.randn(A + 1, generator=g)
    zz = h.double() @ w.double().t() + b.double()
    Ezz = (K + 2) * U * (h.double().abs() @ w.double().abs().t()) + U * b.double().abs()
    z, v, Ez, Ev = zz[:, :A], zz[:, A], Ezz[:, :A], Ezz[:, A]
    r = _act_ref(z, Ez, N, A)
    ar = torch.arange(N)
    hd, wd, bd = h.to(dev), w.to(dev).contiguous(), b.to(dev)
    tag = "N%d-K%d-A%d" % case
    # sampling
    rc, out = _run_act(dev, hd, wd, bd, N, K, A, u=r["u"].to(dev))
    mt.check(rc, "act head")
    _same("ppo_act_head action", tag, out["action"].done("action"), r["target"])
    _within("ppo_act_head value", tag, out["value"].done("value"), v, 2 * Ev)
    _within("ppo_act_head entropy", tag, out["ent"].done("entropy"), r["ent"], 2 * r["E_H"])
    _within("ppo_act_head log_prob", tag, out["lp"].done("log_prob"), r["lp"][ar, r["target"]], 2 * r["E_lp"][ar, r["target"]])
    # given actions: log pi of the recorded action, no draw, nothing else written
    given = torch.randint(0, A, (N,), generator=g)
    given[0], given[-1] = A - 1, 0
    rc, out = _run_act(dev, hd, wd, bd, N, K, A, given=given.to(dev), want_ent=False, want_action=False)
    mt.check(rc, "act head")
    out["action"].untouched("action")
    out["ent"].untouched("entropy")
    _within("ppo_act_head value", tag + "-given", out["value"].done("value"), v, 2 * Ev)
    _within("ppo_act_head log_prob", tag + "-given", out["lp"].done("log_prob"), r["lp"][ar, given], 2 * r["E_lp"][ar, given])
    # values only (ops.ppo_value_head without actions)
    rc, out = _run_act(dev, hd, wd, bd, N, K, A, given=torch.zeros(N, dtype=torch.int64, device=dev),
                       want_ent=False, want_lp=False, want_action=False)
    mt.check(rc, "act head")
    for k in ("action", "ent", "lp"):
        out[k].untouched(k)
    _within("ppo_act_head value", tag + "-values", out["value"].done("value"), v, 2 * Ev)
    # the rows route: action into row 2 of a [3][N] column, (entropy, value) into slot 1 of a [2][2][N] ring
    col, ring = _GuardedInt(3 * N, dev), _Guarded(4 * N, dev)
    lp = _Guarded(N, dev)
    rows = torch.tensor([2, 1], dtype=torch.int32, device=dev)
    ud = r["u"].to(dev)
    mt.check(_native.lib().pfrl_ppo_act_head(
        _p(hd), _p(wd[:A]), _p(bd[:A]), _p(wd[A:]), _p(bd[A:]), _p(ud), None, _p(col.t), _p(ring.t),
        ctypes.c_void_p(ring.t.data_ptr() + 4 * N), _p(lp.t), N, K, A, _p(rows), _stream()), "act head rows")
    cv, rv = col.guards("action column").view(3, N).cpu(), ring.guards("ring").view(2, 2, N).cpu()
    assert bool((cv[:2] == col.MARK).all()) and bool(torch.isnan(rv[0]).all()), "a row / slot other than the addressed one was written"
    _same("ppo_act_head action", tag + "-rows", cv[2], r["target"])
    _within("ppo_act_head entropy", tag + "-rows", rv[1, 0], r["ent"], 2 * r["E_H"])
    _within("ppo_act_head value", tag + "-rows", rv[1, 1], v, 2 * Ev)
    _within("ppo_act_head log_prob", tag + "-rows", lp.done("log_prob"), r["lp"][ar, r["target"]], 2 * r["E_lp"][ar, r["target"]])


def _planted_logits(A):
    """Rows of logits the head reproduces exactly (unit weights, K = 65): (logits, u, wanted action, kind)."""
    g = torch.Generator().manual_seed(A)
    rows = []
    base = torch.randn(4, A, generator=g)
    if A >= 2:
        a = base[0].clone()
        a[0] = -200.0
        rows.append((a, 0.0, 1, "dead first action, u = 0"))
        c = base[1].clone()
        c[A - 1] = -200.0
        rows.append((c, 1.0 - 2.0 ** -24, A - 2, "dead last action, u = 1 - 2^-24"))
        t = base[2].clone().clamp(max=1.0)
        t[0] = t[A - 1] = 2.0
        rows.append((t, None, None, "two equal largest logits"))
    rows.append((base[3], None, None, "plain"))
    return rows


def test_planted_act_rows_are_what_they_claim():
    """No GPU: in float64 the dead action of a planted row has probability below 2^-149 (zero in float32)
    and the wanted action is the first / last live one; the tie row has its two largest logits equal."""
    for A in range(2, 32):
        rows = _planted_logits(A)
        assert [k for *_, k in rows] == ["dead first action, u = 0", "dead last action, u = 1 - 2^-24",
                                         "two equal largest logits", "plain"]
        p0 = torch.softmax(rows[0][0].double(), 0)
        p1 = torch.softmax(rows[1][0].double(), 0)
        assert float(p0[0]) < 2.0 ** -149 < float(p0[1]) and rows[0][2] == 1
        assert float(p1[A - 1]) < 2.0 ** -149 < float(p1[A - 2]) and rows[1][2] == A - 2
        t = rows[2][0]
        assert float(t[0]) == float(t[A - 1]) == float(t.max()) and int((t == t.max()).sum()) == 2
    assert len(_planted_logits(1)) == 1


@gpu
@pytest.mark.parametrize("A", list(range(1, 32)))
def test_ppo_act_head_planted_rows(A):
    dev = _dev()
    K = 65
    rows = _planted_logits(A)
    N = len(rows)
    h = torch.zeros(N, K)
    for i, (lg, *_rest) in enumerate(rows):
        h[i, :A] = lg
    w = torch.zeros(A + 1, K)
    w[torch.arange(A), torch.arange(A)] = 1.0
    b = torch.zeros(A + 1)
    z = h[:, :A].double()
    r = _act_ref(z, torch.zeros_like(z), N, A)
    u, want = r["u"].clone(), r["target"].clone()
    for i, (_lg, ui, ai, _k) in enumerate(rows):
        if ui is not None:
            u[i], want[i] = ui, ai
    assert float(u.max()) < 1.0
    rc, out = _run_act(dev, h.to(dev), w.to(dev), b.to(dev), N, K, A, u=u.to(dev))
    mt.check(rc, "act head")
    act = out["action"].done("action").cpu()
    p = torch.softmax(z, 1)
    assert bool((p[torch.arange(N), act] >= 2.0 ** -149).all()), "a dead action was taken"
    _same("ppo_act_head planted action", "A%d" % A, act, want)
    ar = torch.arange(N)
    _within("ppo_act_head entropy", "A%d-planted" % A, out["ent"].done("entropy"), r["ent"], 2 * r["E_H"])
    _within("ppo_act_head log_prob", "A%d-planted" % A, out["lp"].done("lp"), r["lp"][ar, want], 2 * r["E_lp"][ar, want])
    _same("ppo_act_head planted value", "A%d" % A, out["value"].done("value"), torch.zeros(N))


@gpu
@pytest.mark.parametrize("gate", ["A0", "A32", "K0", "no u01", "no out_action", "N0"])
def test_ppo_act_head_gates(gate):
    dev = _dev()
    N, K, A = 5, 8, 3
    g = torch.Generator().manual_seed(3)
    h, w, b = torch.randn(N, K, generator=g).to(dev), torch.randn(40, K, generator=g).to(dev), torch.randn(40, generator=g).to(dev)
    u = torch.rand(N, generator=g).to(dev)
    kw = {"u": u}
    if gate == "A0":
        A = 0
    elif gate == "A32":
        A = 32
    elif gate == "K0":
        K = 0
    elif gate == "no u01":
        kw = {}
    elif gate == "no out_action":
        kw["want_action"] = False
    elif gate == "N0":
        N = 0
    rc, out = _run_act(dev, h, w, b, N, K, A, room=5, **kw)
    assert rc == (0 if gate == "N0" else PFRL_ERR_ARG), (gate, rc)
    torch.cuda.synchronize()
    for k, buf in out.items():
        buf.untouched(k)


# ================================================================== 4. pfrl_adv_stats, pfrl_ppo_minibatch
STATS_N = [1, 63, 2047, 2048, 2049, 2 * 1024 * 1024 + 1]


def stats_f64(x):
    """The NumPy float64 expression of k_adv_final on exact sums."""
    x = x.astype(np.float64)
    n = x.size
    mean = x.sum() / n
    var = (x * x).sum() / n - mean * mean
    return np.array([mean, math.sqrt(max(var, 0.0))])


def _run_stats(dev, x):
    out, ws = _Guarded(2, dev), _Guarded(2048, dev, F64)
    mt.check(_native.lib().pfrl_adv_stats(_p(x), x.numel(), _p(out.t), _p(ws.t), _stream()), "adv_stats")
    ws.guards("workspace")
    return out.done("mean_std").cpu()


def test_stats_sizes_cross_the_workgroup_cap():
    """No GPU: 2047 / 2048 / 2049 straddle one workgroup's 8 elements per thread; 2 Mi + 1 is the first n whose
    grid (capped at 1024 workgroups of 256 threads x 8) takes a second trip of the grid-stride loop."""
    n = STATS_N[-1]
    assert min((n + 2047) // 2048, 1024) == 1024 and n > 1024 * 256 * 8 and n - 1 == 1024 * 256 * 8
    assert {2047, 2048, 2049} <= set(STATS_N)


@gpu
@pytest.mark.parametrize("n", STATS_N)
def test_adv_stats_exact_on_integers_and_bounded_on_randn(n):
    dev = _dev()
    g = torch.Generator().manual_seed(n)
    xi = torch.randint(-4, 5, (n,), generator=g).float()
    _same("adv_stats integers", "n%d" % n, _run_stats(dev, xi.to(dev)), torch.from_numpy(stats_f64(xi.numpy()).astype(F32)))
    const = torch.full((n,), -3.0)
    _same("adv_stats constant", "n%d" % n, _run_stats(dev, const.to(dev)), torch.tensor([-3.0, 0.0]))
    xr = torch.randn(n, generator=g) * 2 + 0.5
    x64 = xr.double()
    mean, ex2 = x64.mean(), (x64 * x64).mean()
    std = (ex2 - mean * mean).clamp(min=0).sqrt()
    E_var = 64 * 2.0 ** -53 * (ex2 + mean * mean)
    E_std = U * std + torch.min(E_var / (2 * std).clamp(min=1e-300), E_var.sqrt())
    E_mean = U * mean.abs() + 48 * 2.0 ** -53 * x64.abs().mean()
    _within("adv_stats randn", "n%d" % n, _run_stats(dev, xr.to(dev)), torch.stack([mean, std]), 2 * torch.stack([E_mean, E_std]))


def standardise_f32(a, mean_std):
    """(a - mean) / (std + 1e-8f) in float32 operations."""
    a, ms = a.astype(F32), mean_std.astype(F32)
    out = (a - ms[0]) / (ms[1] + F32(1e-8))
    assert out.dtype == np.float32
    return out


def test_standardisation_in_float32_is_what_float64_computes():
    """No GPU: within three roundings of float64, and finite at std = 0."""
    g = torch.Generator().manual_seed(0)
    a = torch.randn(1000, generator=g).numpy()
    for ms in (np.array([0.25, 1.5], F32), np.array([0.25, 0.0], F32)):
        got = standardise_f32(a, ms).astype(np.float64)
        den = np.float64(ms[1]) + np.float64(F32(1e-8))
        want = (a.astype(np.float64) - ms[0]) / den
        assert np.all(np.isfinite(got))
        assert np.all(np.abs(got - want) <= 4 * U * (np.abs(a) + abs(ms[0])) / den)


@gpu
@pytest.mark.parametrize("f32act", [False, True], ids=["int64-actions", "float-actions"])
@pytest.mark.parametrize("k", [1, 4])
@pytest.mark.parametrize("M", [1, 255, 256, 257])
def test_ppo_minibatch_is_the_gather_bit_for_bit(M, k, f32act):
    dev = _dev()
    n, AA = 300, 3
    g = torch.Generator().manual_seed(17 * M + k)
    idx = torch.randint(0, n, (M,), generator=g)
    idx[0] = n - 1
    if M >= 3:
        idx[1] = idx[2] = 7                     # a repeat; unsorted by construction
    col = {key: torch.randn(n, generator=g) for key in ("adv", "lp", "v", "vt")}
    action = torch.randn(n, AA, generator=g) if f32act else torch.randint(0, 18, (n,), generator=g)
    refs = torch.randint(0, 10 ** 6, (n, k), generator=g, dtype=torch.int32)
    L = _native.lib()
    for ms, std in ((torch.tensor([0.25, 1.5]), 1), (torch.tensor([0.25, 0.0]), 1), (torch.tensor([0.25, 1.5]), 0)):
        out = {key: _Guarded(M, dev) for key in ("adv", "lp", "v", "vt")}
        oa = _Guarded(M * AA, dev) if f32act else _GuardedInt(M, dev)
        orf = _GuardedInt(M * k, dev, torch.int32)
        d = {key: t.to(dev) for key, t in col.items()}
        ad, rd, idd, msd = action.to(dev), refs.to(dev), idx.to(dev), ms.to(dev)
        if f32act:
            rc = L.pfrl_ppo_minibatch_f32act(M, _p(idd), _p(d["adv"]), _p(msd), std, _p(d["lp"]), _p(d["v"]), _p(d["vt"]), _p(ad), AA,
                                             _p(rd), k, _p(out["adv"].t), _p(out["lp"].t), _p(out["v"].t), _p(out["vt"].t),
                                             _p(oa.t), _p(orf.t), _stream())
        else:
            rc = L.pfrl_ppo_minibatch(M, _p(idd), _p(d["adv"]), _p(msd), std, _p(d["lp"]), _p(d["v"]), _p(d["vt"]), _p(ad),
                                      _p(rd), k, _p(out["adv"].t), _p(out["lp"].t), _p(out["v"].t), _p(out["vt"].t),
                                      _p(oa.t), _p(orf.t), _stream())
        mt.check(rc, "ppo_minibatch")
        tag = "M%d-k%d-std%d-%g" % (M, k, std, float(ms[1]))
        want_adv = col["adv"][idx]
        if std:
            want_adv = torch.from_numpy(standardise_f32(want_adv.numpy(), ms.numpy()))
        _same("ppo_minibatch adv", tag, out["adv"].done("adv"), want_adv)
        for key in ("lp", "v", "vt"):
            _same("ppo_minibatch " + key, tag, out[key].done(key), col[key][idx])
        _same("ppo_minibatch action", tag, oa.done("action"), action[idx].reshape(-1))
        _same("ppo_minibatch refs", tag, orf.done("refs"), refs[idx].reshape(-1))


# ================================================================== 5. squashed Gaussian
SQ_B = [1, 3, 4, 5, 257]
SQ_A = [1, 6, 63, 64, 65, 128, 130]
LO, HI = -20.0, 2.0
NULL_PATTERNS = [("ga", "gl"), ("ga", None), (None, "gl")]


def _sq_shapes():
    return _spread(SQ_B, SQ_A)


def test_squashed_case_lists():
    """No GPU: a third of the product, every B and A in it; A in {63, 64, 65, 128, 130} round the 64-lane
    stride; three leading dimensions, two ldx, both modes, all NULL patterns; the build contracts nothing."""
    shapes = _sq_shapes()
    assert {B for B, _ in shapes} == set(SQ_B) and {A for _, A in shapes} == set(SQ_A)
    assert len(shapes) * 3 <= len(SQ_B) * len(SQ_A) + 2
    assert NULL_PATTERNS == [("ga", "gl"), ("ga", None), (None, "gl")]
    assert "-ffp-contract=off" in _native.HIPCC_FLAGS and "-fno-fast-math" in _native.HIPCC_FLAGS
    assert not any(f in _native.HIPCC_FLAGS for f in ("-ffast-math", "-Ofast"))


def squashed64(loc, scale, eps):
    """TransformedDistribution(Independent(Normal(loc, scale), 1), [TanhTransform]) on the draw loc + eps scale."""
    x = loc + eps * scale
    tr = TanhTransform(cache_size=1)
    d = TransformedDistribution(Independent(Normal(loc, scale), 1), [tr])
    y = tr(x)
    return x, y, d.log_prob(y)


def head_scale64(ls, lo, hi, mode):
    c = torch.clamp(ls, lo, hi)
    return torch.sqrt(torch.exp(c * 2)) if mode == 0 else torch.exp(c)


def squashed_bounds(loc, scale, eps, eps_s):
    """Section 5's forward bounds (first order, no factor 2) from float64 operands."""
    A = loc.shape[1]
    es = eps * scale
    x = loc + es
    y = torch.tanh(x)
    E_xr = U * es.abs() + U * x.abs()
    E_x = E_xr + es.abs() * eps_s
    E_y = (1 - y * y) * E_x + TANH_ULP * 2 * U * y.abs()
    q = 0.5 * eps * eps
    logs = torch.log(scale)
    nlp = -q - logs - HALF_LOG_2PI
    E_q = eps.abs() * (E_xr + U * es.abs()) / scale + 3 * U * q
    E_nlp = E_q + 2 * U * logs.abs() + eps_s + U * (q + logs).abs() + U * nlp.abs() + U * HALF_LOG_2PI
    z = -2 * x
    sp = torch.nn.functional.softplus(z)
    E_sp = torch.sigmoid(z) * 2 * E_x + SOFTPLUS_ULP * 2 * U * sp + torch.where(z > 20, torch.exp(-z), torch.zeros_like(z))
    t = 2 * (LN2 - x - sp)
    E_t = 2 * (E_x + U * (LN2 + (LN2 - x).abs()) + E_sp + U * (LN2 - x - sp).abs())
    ns = _cd(A, 64) + 6
    lp = nlp.sum(1) - t.sum(1)
    E_lp = (E_t + E_nlp).sum(1) + ns * U * (t.abs() + nlp.abs()).sum(1) + U * lp.abs()
    return {"y": y, "E_y": E_y, "E_lp": E_lp}


def _sq_operands(B, A, seed):
    g = torch.Generator().manual_seed(seed)
    loc = 2 * torch.randn(B, A, generator=g)
    ls = torch.randn(B, A, generator=g) - 1.0
    eps = torch.randn(B, A, generator=g)
    loc.view(-1)[0], eps.view(-1)[0] = 12.0, 0.5          # |x| > 10: the softplus switch, tanhf = 1 exactly
    loc.view(-1)[-1], eps.view(-1)[-1] = -12.0, -0.5
    if B * A > 2:
        loc.view(-1)[1], eps.view(-1)[1] = 9.9, 0.25
    return loc, ls, eps, torch.randn(B, A, generator=g), torch.randn(B, generator=g)


def _padded(dev, t, ld):
    """t [B, n] inside a NaN buffer with row stride ld."""
    buf = torch.full((t.shape[0], ld), float("nan"), device=dev)
    buf[:, :t.shape[1]] = t.to(dev)
    return buf


def squashed_bwd_f32(y, eps, scale, ga, gl):
    """k_squashed_gaussian_bwd in float32 NumPy operations, the kernel's association."""
    y, e, s = y.astype(F32), eps.astype(F32), scale.astype(F32)
    ga = np.zeros_like(y) if ga is None else ga.astype(F32)
    gl = np.zeros((y.shape[0], 1), F32) if gl is None else gl.astype(F32)[:, None]
    t = ga * (F32(1) - y * y)
    y2 = F32(2) * y
    g_loc = t + gl * y2
    g_scale = t * e + gl * (y2 * e - F32(1) / s)
    assert g_loc.dtype == np.float32 and g_scale.dtype == np.float32
    return g_loc, g_scale


def test_float32_backward_restatement_is_what_float64_autograd_computes():
    """No GPU: squashed_bwd_f32 on float32(tanh) against autograd through the float64 distribution, within
    the handful of roundings it holds (pre-activations kept below |x| = 4: from float32(y) alone 1 - y^2
    loses its relative accuracy near |y| = 1, which is the kernel's arithmetic too)."""
    g = torch.Generator().manual_seed(1)
    B, A = 33, 7
    loc, eps = torch.randn(B, A, generator=g).double(), torch.randn(B, A, generator=g).double()
    scale = torch.exp(0.3 * torch.randn(B, A, generator=g)).double()
    ga, gl = torch.randn(B, A, generator=g).double(), torch.randn(B, generator=g).double()
    for pat in NULL_PATTERNS:
        l, s = loc.clone().requires_grad_(True), scale.clone().requires_grad_(True)
        _, y, lp = squashed64(l, s, eps)
        tot = (ga * y).sum() * (pat[0] is not None) + (gl * lp).sum() * (pat[1] is not None)
        gl64, gs64 = torch.autograd.grad(tot, [l, s])
        got_l, got_s = squashed_bwd_f32(_np(y), _np(eps), _np(scale), _np(ga) if pat[0] else None, _np(gl) if pat[1] else None)
        mag_l = ga.abs() + 2 * gl.abs()[:, None]
        mag_s = mag_l * eps.abs() + gl.abs()[:, None] / scale
        assert bool(((torch.from_numpy(got_l).double() - gl64).abs() <= 16 * U * mag_l).all())
        assert bool(((torch.from_numpy(got_s).double() - gs64).abs() <= 16 * U * mag_s).all())


@gpu
@pytest.mark.parametrize("shape", _sq_shapes(), ids=lambda s: "B%d-A%d" % s)
def test_squashed_gaussian_forward_and_backward(shape):
    dev = _dev()
    B, A = shape
    loc, ls, eps, ga, gl = _sq_operands(B, A, 97 * B + A)
    scale = torch.exp(0.5 * ls)
    L = _native.lib()
    x64, y64, lp64 = squashed64(loc.double(), scale.double(), eps.double())
    bd = squashed_bounds(loc.double(), scale.double(), eps.double(), 0.0)
    assert bool((x64.abs() > 10).any())
    epsd, gad, gld = eps.to(dev), ga.to(dev), gl.to(dev)
    for ld_kind in ("A", "A+3", "halves"):
        if ld_kind == "halves":
            both = torch.cat([loc, scale], 1).to(dev)
            lb, sb, ld_l, ld_s = both, both[:, A:], 2 * A, 2 * A
        else:
            ld_l = ld_s = A + (3 if ld_kind == "A+3" else 0)
            lb, sb = _padded(dev, loc, ld_l), _padded(dev, scale, ld_s)
        for want_neg in (False, True):
            tag = "B%d-A%d-ld%s-neg%d" % (B, A, ld_kind, want_neg)
            act, lp, neg = _Guarded(B * A, dev), _Guarded(B, dev), _Guarded(B, dev)
            mt.check(L.pfrl_squashed_gaussian_fwd(_p(lb), ld_l, _p(sb), ld_s, _p(epsd), _p(act.t), _p(lp.t),
                                                  _p(neg.t) if want_neg else None, B, A, _stream()), "sq fwd")
            y = act.done("action")
            _within("squashed_gaussian_fwd action", tag, y, y64, 2 * bd["E_y"])
            _within("squashed_gaussian_fwd logp", tag, lp.done("logp"), lp64, 2 * bd["E_lp"])
            if want_neg:
                _same("squashed_gaussian_fwd neg_logp", tag, neg.done("neg"), -lp.t.cpu())
            else:
                neg.untouched("neg_logp")
            yc = y.cpu().view(B, A)
            assert float(yc.view(-1)[-1]) == -1.0 and (B * A == 1 or float(yc.view(-1)[0]) == 1.0)   # tanhf saturates past |x| = 10
        for pat in NULL_PATTERNS:
            tag = "B%d-A%d-ld%s-%s" % (B, A, ld_kind, pat)
            g_loc, g_scale = _Guarded(B * A, dev), _Guarded(B * A, dev)
            mt.check(L.pfrl_squashed_gaussian_bwd(_p(gad) if pat[0] else None, _p(gld) if pat[1] else None, _p(act.t), _p(epsd),
                                                  _p(sb), ld_s, _p(g_loc.t), _p(g_scale.t), B, A, _stream()), "sq bwd")
            wl, ws = squashed_bwd_f32(yc.numpy(), eps.numpy(), scale.numpy(), ga.numpy() if pat[0] else None, gl.numpy() if pat[1] else None)
            _same("squashed_gaussian_bwd g_loc", tag, g_loc.done("g_loc").view(B, A), torch.from_numpy(wl))
            _same("squashed_gaussian_bwd g_scale", tag, g_scale.done("g_scale").view(B, A), torch.from_numpy(ws))


def _example_head(mode):
    def head(x):
        mean, log_scale = torch.chunk(x, 2, dim=1)
        log_scale = torch.clamp(log_scale, LO, HI)
        scale = torch.sqrt(torch.exp(log_scale * 2)) if mode == 0 else torch.exp(log_scale)
        return TransformedDistribution(Independent(Normal(loc=mean, scale=scale), 1), [TanhTransform(cache_size=1)])
    return head


@functools.lru_cache(maxsize=None)
def _bit_exact(A, mode):
    from pfrl_amd.utils.squashed_gaussian import recognise_head
    spec = recognise_head(_example_head(mode), 2 * A, _dev())
    assert spec is not None and (spec.lo, spec.hi, spec.mode, spec.A) == (LO, HI, mode, A), spec
    return spec.bit_exact


@gpu
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("shape", _sq_shapes(), ids=lambda s: "B%d-A%d" % s)
def test_squashed_head_forward_and_backward(shape, mode):
    dev = _dev()
    B, A = shape
    loc, ls, eps, ga, gl = _sq_operands(B, A, 89 * B + A + mode)
    assert not bool(((ls == LO) | (ls == HI)).any())            # no log-scale on a clamp bound (an input: no error to allow for)
    L = _native.lib()
    xin = torch.cat([loc, ls], 1).double()
    s64 = head_scale64(xin[:, A:], LO, HI, mode)
    _, y64, lp64 = squashed64(xin[:, :A], s64, eps.double())
    bd = squashed_bounds(xin[:, :A], s64, eps.double(), 2 * U)
    epsd, gad, gld = eps.to(dev), ga.to(dev), gl.to(dev)
    exact = _bit_exact(A, mode)
    for ldx in (2 * A, 2 * A + 5):
        xb = _padded(dev, torch.cat([loc, ls], 1), ldx)
        tag = "B%d-A%d-mode%d-ldx%d" % (B, A, mode, ldx)
        act, lp, neg = _Guarded(B * A, dev), _Guarded(B, dev), _Guarded(B, dev)
        mt.check(L.pfrl_squashed_head_fwd(_p(xb), ldx, LO, HI, mode, _p(epsd), _p(act.t), _p(lp.t), _p(neg.t), B, A, _stream()), "head fwd")
        y = act.done("action")
        _within("squashed_head_fwd action", tag, y, y64, 2 * bd["E_y"])
        _within("squashed_head_fwd logp", tag, lp.done("logp"), lp64, 2 * bd["E_lp"])
        _same("squashed_head_fwd neg_logp", tag, neg.done("neg"), -lp.t.cpu())
        # against the plain launch fed the float32 scale torch computes
        s32 = head_scale64(xb[:, A:2 * A], LO, HI, mode).contiguous()
        act2, lp2 = _Guarded(B * A, dev), _Guarded(B, dev)
        mt.check(L.pfrl_squashed_gaussian_fwd(_p(xb), ldx, _p(s32), A, _p(epsd), _p(act2.t), _p(lp2.t), None, B, A, _stream()), "sq fwd")
        if exact:
            _same("squashed_head_fwd == plain action", tag, y, act2.done("a").cpu())
            _same("squashed_head_fwd == plain logp", tag, lp.t, lp2.done("lp").cpu())
        else:
            _within("squashed_head_fwd ~ plain action", tag, y, act2.done("a").cpu().double(), 4 * bd["E_y"].reshape(-1))
            _within("squashed_head_fwd ~ plain logp", tag, lp.t, lp2.done("lp").cpu().double(), 4 * bd["E_lp"])
        for pat in NULL_PATTERNS:
            ptag = "%s-%s" % (tag, pat)
            xr = xin.clone().requires_grad_(True)
            sr = head_scale64(xr[:, A:], LO, HI, mode)
            _, yr, lpr = squashed64(xr[:, :A], sr, eps.double())
            tot = (ga.double() * yr).sum() * (pat[0] is not None) + (gl.double() * lpr).sum() * (pat[1] is not None)
            (gx64,) = torch.autograd.grad(tot, [xr])
            G = ga.double().abs() * (pat[0] is not None)
            Gl = gl.double().abs()[:, None] * (pat[1] is not None)
            yv, e, s = bd["y"], eps.double(), s64
            t = G * (1 - yv * yv)
            E_t = G * (2 * yv.abs() * bd["E_y"] + U) + 2 * U * t
            E_gloc = E_t + Gl * (2 * bd["E_y"] + 2 * U * yv.abs()) + U * gx64[:, :A].abs()
            gs = gx64[:, A:] / s                     # d s / d c = s inside the clamp
            E_gs = (e.abs() * E_t + U * (t * e).abs()
                    + Gl * (2 * e.abs() * bd["E_y"] + 2 * U * (yv * e).abs() + 3 * U / s + U * (2 * yv * e).abs() + U / s) + U * gs.abs())
            E_gc = s * E_gs + 6 * U * gx64[:, A:].abs()
            g_x = _Guarded(B * 2 * A, dev)
            mt.check(L.pfrl_squashed_head_bwd(_p(gad) if pat[0] else None, _p(gld) if pat[1] else None, _p(act.t), _p(epsd), _p(xb), ldx,
                                              LO, HI, mode, _p(g_x.t), B, A, _stream()), "head bwd")
            _within("squashed_head_bwd g_x", ptag, g_x.done("g_x"), gx64, 2 * torch.cat([E_gloc, E_gc], 1))


@gpu
@pytest.mark.parametrize("mode", [0, 1])
def test_squashed_head_clamp_mask_is_exact(mode):
    """Log-scales at lo, hi and the floats next to them: the gradient is exactly 0 strictly outside and what
    float64 autograd gives (non-zero: torch.clamp passes the gradient at its bounds) at and inside."""
    dev = _dev()
    lo, hi = -2.0, 1.0
    edge = np.array([lo, hi], F32)
    ls = np.concatenate([edge, np.nextafter(edge, F32(-np.inf)), np.nextafter(edge, F32(np.inf))]).astype(F32)
    outside = torch.tensor([False, False, True, False, False, True])
    B, A = len(ls), 1
    x = torch.stack([torch.full((B,), 0.3), torch.from_numpy(ls)], 1)
    eps, ga, gl = torch.full((B, 1), 0.7), torch.ones(B, 1), torch.ones(B)
    xr = x.double().requires_grad_(True)
    _, y, lp = squashed64(xr[:, :1], head_scale64(xr[:, 1:], lo, hi, mode), eps.double())
    (g64,) = torch.autograd.grad((ga.double() * y).sum() + (gl.double() * lp).sum(), [xr])
    assert bool((g64[outside, 1] == 0).all()) and bool((g64[~outside, 1] != 0).all())
    L = _native.lib()
    xd, ed, gad, gld = x.to(dev).contiguous(), eps.to(dev), ga.to(dev), gl.to(dev)
    act, lpo, g_x = _Guarded(B, dev), _Guarded(B, dev), _Guarded(2 * B, dev)
    mt.check(L.pfrl_squashed_head_fwd(_p(xd), 2, lo, hi, mode, _p(ed), _p(act.t), _p(lpo.t), None, B, A, _stream()), "head fwd")
    mt.check(L.pfrl_squashed_head_bwd(_p(gad), _p(gld), _p(act.done("a")), _p(ed), _p(xd), 2, lo, hi, mode, _p(g_x.t),
                                      B, A, _stream()), "head bwd")
    got = g_x.done("g_x").view(B, 2).cpu()
    assert bool((got[outside, 1] == 0).all()), got
    assert bool((got[~outside, 1] != 0).all()), got
    _within("squashed_head_bwd clamp edges", "mode%d" % mode, got[:, 1], g64[:, 1], 64 * U * g64[:, 1].abs())


@gpu
@pytest.mark.parametrize("gate", ["A0", "ld<A", "ldx<2A", "mode2", "lo>hi", "B0"])
def test_squashed_gates(gate):
    dev = _dev()
    B, A = 3, 4
    t = torch.ones(B, 2 * A, device=dev)
    e = torch.zeros(B, A, device=dev)
    bufs = [_Guarded(B * 2 * A, dev) for _ in range(4)]
    a, l, n, gx = bufs
    L = _native.lib()
    if gate == "A0":
        rcs = [L.pfrl_squashed_gaussian_fwd(_p(t), A, _p(t), A, _p(e), _p(a.t), _p(l.t), _p(n.t), B, 0, _stream()),
               L.pfrl_squashed_gaussian_bwd(_p(e), _p(e), _p(e), _p(e), _p(t), A, _p(a.t), _p(l.t), B, 0, _stream()),
               L.pfrl_squashed_head_fwd(_p(t), 2 * A, LO, HI, 0, _p(e), _p(a.t), _p(l.t), _p(n.t), B, 0, _stream()),
               L.pfrl_squashed_head_bwd(_p(e), _p(e), _p(e), _p(e), _p(t), 2 * A, LO, HI, 0, _p(gx.t), B, 0, _stream())]
    elif gate == "ld<A":
        rcs = [L.pfrl_squashed_gaussian_fwd(_p(t), A - 1, _p(t), A, _p(e), _p(a.t), _p(l.t), _p(n.t), B, A, _stream()),
               L.pfrl_squashed_gaussian_fwd(_p(t), A, _p(t), A - 1, _p(e), _p(a.t), _p(l.t), _p(n.t), B, A, _stream()),
               L.pfrl_squashed_gaussian_bwd(_p(e), _p(e), _p(e), _p(e), _p(t), A - 1, _p(a.t), _p(l.t), B, A, _stream())]
    elif gate == "ldx<2A":
        rcs = [L.pfrl_squashed_head_fwd(_p(t), 2 * A - 1, LO, HI, 0, _p(e), _p(a.t), _p(l.t), _p(n.t), B, A, _stream()),
               L.pfrl_squashed_head_bwd(_p(e), _p(e), _p(e), _p(e), _p(t), 2 * A - 1, LO, HI, 0, _p(gx.t), B, A, _stream())]
    elif gate == "mode2":
        rcs = [L.pfrl_squashed_head_fwd(_p(t), 2 * A, LO, HI, 2, _p(e), _p(a.t), _p(l.t), _p(n.t), B, A, _stream()),
               L.pfrl_squashed_head_bwd(_p(e), _p(e), _p(e), _p(e), _p(t), 2 * A, LO, HI, 2, _p(gx.t), B, A, _stream())]
    elif gate == "lo>hi":
        rcs = [L.pfrl_squashed_head_fwd(_p(t), 2 * A, 1.0, -1.0, 0, _p(e), _p(a.t), _p(l.t), _p(n.t), B, A, _stream())]
    else:
        rcs = [L.pfrl_squashed_gaussian_fwd(_p(t), A, _p(t), A, _p(e), _p(a.t), _p(l.t), _p(n.t), 0, A, _stream()),
               L.pfrl_squashed_gaussian_bwd(_p(e), _p(e), _p(e), _p(e), _p(t), A, _p(a.t), _p(l.t), 0, A, _stream()),
               L.pfrl_squashed_head_fwd(_p(t), 2 * A, LO, HI, 0, _p(e), _p(a.t), _p(l.t), _p(n.t), 0, A, _stream()),
               L.pfrl_squashed_head_bwd(_p(e), _p(e), _p(e), _p(e), _p(t), 2 * A, LO, HI, 0, _p(gx.t), 0, A, _stream())]
    assert rcs == [0 if gate == "B0" else PFRL_ERR_ARG] * len(rcs), (gate, rcs)
    torch.cuda.synchronize()
    for b in bufs:
        b.untouched(gate)


# ================================================================== 6. the math library on its own
def _f32_step(x, k):
    """x moved k float32 steps (k may be negative)."""
    x = np.asarray(x, F32).copy()
    for _ in range(abs(k)):
        x = np.nextafter(x, F32(np.inf if k > 0 else -np.inf))
    return x


def logp_of_softplus_f32(x, sp):
    """logp of k_squashed_gaussian_fwd at A = 1, eps = 0, scale = 1 as float32 operations round sp."""
    x, sp = x.astype(F32), sp.astype(F32)
    xx = x + F32(0) * F32(1)
    d = xx - x
    nlp = -(d * d) / (F32(2) * (F32(1) * F32(1))) - F32(0) - F32(HALF_LOG_2PI)
    ladj = F32(0) + F32(2) * (F32(LN2) - xx - sp)
    return (F32(0) - ladj) + (F32(0) + nlp)


def _sweep():
    a = np.concatenate([np.linspace(-12, 12, 1537), np.linspace(-10.5, -9.5, 513), [-10.0, 10.0, 0.0, -0.0, 1e-3, -1e-3, 1e-6, 20.0, -20.0]])
    return torch.from_numpy(a.astype(F32))


def test_softplus_restatement_matches_float64_at_the_correctly_rounded_softplus():
    """No GPU: fed float32(softplus64), the float32 chain is within a few roundings of the float64 log-density."""
    x = _sweep()
    z = -2 * x.double()
    sp = torch.nn.functional.softplus(z)
    got = logp_of_softplus_f32(x.numpy(), sp.float().numpy()).astype(np.float64)
    _, _, lp = squashed64(x.double()[:, None], torch.ones(len(x), 1, dtype=F64), torch.zeros(len(x), 1, dtype=F64))
    mag = 2 * (LN2 + x.double().abs() + sp) + HALF_LOG_2PI
    assert bool(((torch.from_numpy(got) - lp).abs() <= 8 * U * mag).all())


@gpu
def test_device_tanhf_and_softplus_accuracy_in_ulp():
    """The single-function cases: what they observe is the math library's figure, not the kernel's."""
    dev = _dev()
    x = _sweep()
    n = len(x)
    L = _native.lib()
    xd = x.to(dev).view(n, 1).contiguous()
    one, zero = torch.ones(n, 1, device=dev), torch.zeros(n, 1, device=dev)
    act, lp = _Guarded(n, dev), _Guarded(n, dev)
    mt.check(L.pfrl_squashed_gaussian_fwd(_p(xd), 1, _p(one), 1, _p(zero), _p(act.t), _p(lp.t), None, n, 1, _stream()), "sq fwd")
    y = act.done("action").cpu().double()
    y64 = torch.tanh(x.double())
    ulps = float(((y - y64).abs() / _ulp32(y64)).max())
    _note("mathlib tanhf [ulp]", "sweep", ulps)
    assert ulps <= TANH_ULP, "tanhf is off by %.2f ulp: raise TANH_ULP to the next integer" % ulps
    assert bool((y[x.abs() >= 10] .abs() == 1).all())
    # log1pf(expf(z)), z = -2 x, read out of logp: the smallest |k| with chain(float32(sp64) + k ulp) == logp
    z = -2 * x.double()
    sp32 = torch.nn.functional.softplus(z).float().numpy()
    got = lp.done("logp").cpu().numpy()
    K = 8
    best = np.full(n, np.inf)
    for k in range(-K, K + 1):
        hit = logp_of_softplus_f32(x.numpy(), _f32_step(sp32, k)) == got
        best = np.where(hit & (abs(k) < best), abs(k), best)
    assert np.all(np.isfinite(best)), "logp is not the float32 chain round any softplus within %d ulp at x = %r" % (K, x.numpy()[~np.isfinite(best)][:5])
    past = (z > 20).numpy()
    assert np.all(best[past] <= 1), "past the switch sp is -2 x itself"
    _note("mathlib log1pf(expf) [ulp]", "sweep", float(best.max()))
    assert best.max() <= SOFTPLUS_ULP, "log1pf(expf(.)) is off by %d ulp: raise the assumption" % best.max()


# ================================================================== 7. SAC losses
SAC_B = [1, 63, 64, 255, 256, 257, 1000, 4099]
TEMPS = [("value", 0.5), ("value", _f(0.2)), ("log", 0.0), ("log", _f(-0.7))]


def _temp(dev, kind, val):
    """-> (log_temperature device pointer or None, numeric temperature, T as float64, relative error of T)."""
    if kind == "value":
        return None, val, float(val), 0.0
    lt = torch.tensor([val], dtype=torch.float32, device=dev)
    return lt, 123.0, math.exp(val), (0.0 if val == 0.0 else 2 * U)


def target_q_f32(r, d, t, q1, q2, nlp, T):
    soft = np.minimum(q1, q2) - F32(T) * nlp
    out = r + (d * (F32(1) - t)) * soft
    assert out.dtype == np.float32
    return out


def test_float32_target_is_what_float64_computes():
    """No GPU: r + (d (1 - t)) (min(q1, q2) - T lp) in float32 within five roundings of float64."""
    g = torch.Generator().manual_seed(2)
    r, q1, q2, lp = (torch.randn(500, generator=g) for _ in range(4))
    d, t = torch.full((500,), _f(0.99)), (torch.rand(500, generator=g) < 0.2).float()
    got = torch.from_numpy(target_q_f32(*(x.numpy() for x in (r, d, t, q1, q2, lp)), _f(0.2))).double()
    soft = torch.min(q1, q2).double() - _f(0.2) * lp.double()
    want = r.double() + d.double() * (1 - t.double()) * soft
    mag = r.abs().double() + torch.min(q1, q2).abs().double() + 0.2 * lp.abs().double()
    assert bool(((got - want).abs() <= 6 * U * mag).all())


def _red_bound(B, per_term, mag):
    return (_cd(B, 256) + 9 + per_term) * U * mag


def _sixteenths(g, n, lo=-32, hi=32, step=0.25):
    return torch.randint(lo, hi + 1, (n,), generator=g).float() * step


@gpu
@pytest.mark.parametrize("B", SAC_B)
def test_sac_target_q(B):
    dev = _dev()
    g = torch.Generator().manual_seed(B)
    r, q1, q2, lp = (torch.randn(B, generator=g) for _ in range(4))
    d, t = torch.full((B,), _f(0.99)), (torch.rand(B, generator=g) < 0.2).float()
    q2[::5] = q1[::5]
    L = _native.lib()
    dv = [x.to(dev) for x in (r, d, t, q1, q2, lp)]
    for kind, val in TEMPS:
        lt, tnum, T, relT = _temp(dev, kind, val)
        out = _Guarded(B, dev)
        mt.check(L.pfrl_sac_target_q(*[_p(x) for x in dv], _p(lt), tnum, _p(out.t), B, _stream()), "target_q")
        got = out.done("target_q")
        tag = "B%d-%s%g" % (B, kind, val)
        if relT == 0.0:
            _same("sac_target_q", tag, got, torch.from_numpy(target_q_f32(*(x.numpy() for x in (r, d, t, q1, q2, lp)), T)))
        else:
            coef = d.double() * (1 - t.double())
            mn, tl = torch.min(q1, q2).double(), T * lp.double()
            soft = mn - tl
            want = r.double() + coef * soft
            E = coef * ((relT + U) * tl.abs() + U * soft.abs()) + 2 * U * (coef * soft).abs() + U * want.abs()
            _within("sac_target_q expf", tag, got, want, 2 * E)
    out = _Guarded(4, dev)
    assert L.pfrl_sac_target_q(*[_p(x) for x in dv], None, 1.0, _p(out.t), 0, _stream()) == 0
    torch.cuda.synchronize()
    out.untouched("B = 0")


def _ptrs(*ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() if t is not None else 0 for t in ts])


@gpu
@pytest.mark.parametrize("B", SAC_B)
def test_half_mse_single_and_twin(B):
    dev = _dev()
    g = torch.Generator().manual_seed(3 * B)
    L = _native.lib()
    for kind in ("exact", "randn"):
        if kind == "exact":
            tg, p1, p2 = (_sixteenths(g, B, -16, 16) for _ in range(3))
        else:
            tg, p1, p2 = (torch.randn(B, generator=g) for _ in range(3))
        tag = "B%d-%s" % (B, kind)
        tgd, p1d, p2d = tg.to(dev), p1.to(dev), p2.to(dev)
        gl = torch.tensor([_f(0.75), _f(-1.3)])
        gld = gl.to(dev)
        single = []
        for i, (p, pd) in enumerate(((p1, p1d), (p2, p2d))):
            loss, gp = _Guarded(1, dev), _Guarded(B, dev)
            mt.check(L.pfrl_half_mse_fwd(_p(tgd), _p(pd), _p(loss.t), B, _stream()), "half_mse_fwd")
            mt.check(L.pfrl_half_mse_bwd(_p(gld[i:]), _p(tgd), _p(pd), _p(gp.t), B, _stream()), "half_mse_bwd")
            d64 = tg.double() - p.double()
            terms = d64 * d64
            if kind == "exact":
                assert bool((terms * 16 == (terms * 16).round()).all()) and float(terms.sum()) < 2 ** 20
                want = F32(0.5) * (F32(float(terms.sum())) / F32(B))
                _same("half_mse_fwd exact", tag, loss.done("loss"), torch.tensor([want]))
            else:
                _within("half_mse_fwd", tag, loss.done("loss"), (0.5 * terms.mean()).reshape(1), (2 * 0.5 * _red_bound(B, 3, terms.sum()) / B).reshape(1))
            d32 = tg.numpy() - p.numpy()
            want_g = -((F32(2) * d32) * ((F32(0.5) * gl.numpy()[i]) / F32(B)))
            _same("half_mse_bwd", tag, gp.done("g_pred"), torch.from_numpy(want_g))
            single.append((loss.t.cpu(), gp.t.cpu(), d32))
        # twins: bit for bit the two single launches; unit gradients; NULL patterns
        l2, u2, g2 = _Guarded(2, dev), _Guarded(2 * B, dev), _Guarded(2 * B, dev)
        mt.check(L.pfrl_half_mse_twin_fwd(_p(tgd), _ptrs(p1d, p2d), _ptrs(l2.t, l2.t[1:]), _ptrs(u2.t, u2.t[B:]), B, _stream()), "twin fwd")
        mt.check(L.pfrl_half_mse_twin_bwd(_ptrs(gld, gld[1:]), _p(tgd), _ptrs(p1d, p2d), _ptrs(g2.t, g2.t[B:]), B, _stream()), "twin bwd")
        lv, uv, gv = l2.done("losses").cpu(), u2.done("unit").view(2, B).cpu(), g2.done("g").view(2, B).cpu()
        for i in range(2):
            _same("half_mse_twin_fwd == single", tag, lv[i:i + 1], single[i][0])
            _same("half_mse_twin_bwd == single", tag, gv[i], single[i][1])
            _same("half_mse_twin_fwd unit gradient", tag, uv[i], torch.from_numpy(-((F32(2) * single[i][2]) * (F32(0.5) / F32(B)))))
        l3, u3, g3 = _Guarded(2, dev), _Guarded(2 * B, dev), _Guarded(2 * B, dev)
        mt.check(L.pfrl_half_mse_twin_fwd(_p(tgd), _ptrs(p1d, p2d), _ptrs(l3.t, l3.t[1:]), None, B, _stream()), "twin fwd")
        _same("half_mse_twin_fwd losses only", tag, l3.done("losses"), lv)
        u3.untouched("unit gradients")
        mt.check(L.pfrl_half_mse_twin_bwd(_ptrs(None, gld[1:]), _p(tgd), _ptrs(p1d, p2d), _ptrs(g3.t, g3.t[B:]), B, _stream()), "twin bwd")
        gz = g3.done("g").view(2, B).cpu()
        _same("half_mse_twin_bwd NULL g_loss", tag, gz[0], torch.zeros(B))
        _same("half_mse_twin_bwd NULL g_loss", tag, gz[1], single[1][1])


@gpu
@pytest.mark.parametrize("B", SAC_B)
def test_sac_policy_loss(B):
    dev = _dev()
    g = torch.Generator().manual_seed(5 * B)
    L = _native.lib()
    for kind in ("exact", "randn"):
        if kind == "exact":
            lp, q1, q2 = _sixteenths(g, B, -16, 16, 0.125), _sixteenths(g, B, -32, 32, 0.0625), _sixteenths(g, B, -32, 32, 0.0625)
        else:
            lp, q1, q2 = (torch.randn(B, generator=g) for _ in range(3))
        q2[::3] = q1[::3]                               # ties: half each
        if B >= 3:
            q1[1], q2[1], q1[2], q2[2] = -1.0, 1.0, 1.0, -1.0
            assert bool((q1 < q2).any()) and bool((q1 > q2).any())
        assert bool((q1 == q2).any())
        lpd, q1d, q2d = lp.to(dev), q1.to(dev), q2.to(dev)
        for tk, val in (TEMPS if kind == "randn" else [("value", 0.5), ("log", 0.0)]):
            lt, tnum, T, relT = _temp(dev, tk, val)
            tag = "B%d-%s-%s%g" % (B, kind, tk, val)
            loss = _Guarded(1, dev)
            u = [_Guarded(B, dev) for _ in range(3)]
            mt.check(L.pfrl_sac_policy_loss_fwd(_p(lpd), _p(q1d), _p(q2d), _p(lt), tnum, _p(loss.t), _p(u[0].t), _p(u[1].t), _p(u[2].t),
                                                B, _stream()), "policy fwd")
            mn = torch.min(q1, q2).double()
            terms = T * lp.double() - mn
            mag = (T * lp.double()).abs().sum() + mn.abs().sum()
            if kind == "exact":
                assert bool((terms * 16 == (terms * 16).round()).all()) and float(mag) < 2 ** 20
                _same("sac_policy_loss_fwd exact", tag, loss.done("loss"), torch.tensor([F32(float(terms.sum())) / F32(B)]))
            else:
                E = _red_bound(B, 2, mag) / B + relT * (T * lp.double()).abs().sum() / B
                _within("sac_policy_loss_fwd", tag, loss.done("loss"), terms.mean().reshape(1), (2 * E).reshape(1))
            a, b = q1.numpy(), q2.numpy()
            w1 = np.where(a < b, F32(1), np.where(a == b, F32(0.5), F32(0)))
            w2 = np.where(b < a, F32(1), np.where(a == b, F32(0.5), F32(0)))
            glv = torch.tensor([_f(-0.6)])
            glvd = glv.to(dev)
            gb = [_Guarded(B, dev) for _ in range(3)]
            mt.check(L.pfrl_sac_policy_loss_bwd(_p(glvd), _p(q1d), _p(q2d), _p(lt), tnum, _p(gb[0].t), _p(gb[1].t), _p(gb[2].t),
                                                B, _stream()), "policy bwd")
            for name, bufs, gg in (("fwd unit", u, F32(1) / F32(B)), ("bwd", gb, glv.numpy()[0] / F32(B))):
                got = [x.done(name).cpu() for x in bufs]
                _same("sac_policy_loss %s g_q1" % name, tag, got[1], torch.from_numpy(-(gg * w1)))
                _same("sac_policy_loss %s g_q2" % name, tag, got[2], torch.from_numpy(-(gg * w2)))
                if relT == 0.0:
                    _same("sac_policy_loss %s g_logp" % name, tag, got[0], torch.full((B,), float(gg * F32(T))))
                else:
                    want = torch.full((B,), float(gg) * T, dtype=F64)
                    _within("sac_policy_loss %s g_logp expf" % name, tag, got[0], want, 2 * (relT + U) * want.abs())
            l2 = _Guarded(1, dev)
            mt.check(L.pfrl_sac_policy_loss_fwd(_p(lpd), _p(q1d), _p(q2d), _p(lt), tnum, _p(l2.t), None, None, None, B, _stream()), "policy fwd")
            _same("sac_policy_loss_fwd without unit gradients", tag, l2.done("loss"), loss.t.cpu())


@gpu
def test_sac_loss_gates():
    dev = _dev()
    L = _native.lib()
    x = torch.zeros(8, device=dev)
    lt = torch.zeros(1, device=dev)
    o = [_Guarded(8, dev) for _ in range(4)]
    rcs = [L.pfrl_half_mse_fwd(_p(x), _p(x), _p(o[0].t), 0, _stream()),
           L.pfrl_half_mse_bwd(_p(x), _p(x), _p(x), _p(o[0].t), 0, _stream()),
           L.pfrl_half_mse_twin_fwd(_p(x), _ptrs(x, x), _ptrs(o[0].t, o[1].t), None, 0, _stream()),
           L.pfrl_half_mse_twin_bwd(_ptrs(x, x), _p(x), _ptrs(x, x), _ptrs(o[0].t, o[1].t), 0, _stream()),
           L.pfrl_sac_policy_loss_fwd(_p(x), _p(x), _p(x), None, 1.0, _p(o[0].t), None, None, None, 0, _stream()),
           L.pfrl_sac_policy_loss_bwd(_p(x), _p(x), _p(x), None, 1.0, _p(o[0].t), _p(o[1].t), _p(o[2].t), 0, _stream()),
           L.pfrl_sac_temperature_loss(_p(lt), _p(x), 1.0, _p(o[0].t), 0, _stream()),
           L.pfrl_sac_temperature_loss(None, _p(x), 1.0, _p(o[0].t), 8, _stream()),
           # one or two (not three) unit-gradient pointers
           L.pfrl_sac_policy_loss_fwd(_p(x), _p(x), _p(x), None, 1.0, _p(o[0].t), _p(o[1].t), None, None, 8, _stream()),
           L.pfrl_sac_policy_loss_fwd(_p(x), _p(x), _p(x), None, 1.0, _p(o[0].t), _p(o[1].t), _p(o[2].t), None, 8, _stream()),
           L.pfrl_sac_policy_loss_fwd(_p(x), _p(x), _p(x), None, 1.0, _p(o[0].t), None, _p(o[2].t), _p(o[3].t), 8, _stream())]
    assert rcs == [PFRL_ERR_ARG] * len(rcs), rcs
    torch.cuda.synchronize()
    for b in o:
        b.untouched("gate")


def adam_element(p0, g, m0, v0, step, lr, b1, b2, eps, wd):
    """k_sac_temperature_step's update of one element: double scalars, float32 element operations.
    -> (p, m, v, step) as float32."""
    p0, g, m0, v0 = F32(p0), F32(g), F32(m0), F32(v0)
    t = float(F32(step)) + 1.0
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    step_size, bc2_sqrt = F32(-(lr / bc1)), F32(math.sqrt(bc2))
    w1, fb2, omb2 = F32(1.0 - b1), F32(b2), F32(1.0 - b2)
    feps, fwd = F32(eps), F32(wd)
    gi = g
    if fwd != 0:
        gi = gi + fwd * p0
    dm = gi - m0
    mi = (m0 + w1 * dm) if w1 < F32(0.5) else (gi - dm * (F32(1) - w1))
    vi = v0 * fb2 + (omb2 * gi) * gi
    denom = np.sqrt(vi) / bc2_sqrt + feps
    p = p0 + (step_size * mi) / denom
    out = (p, mi, vi, F32(step) + F32(1))
    assert all(type(x) is np.float32 for x in out)
    return out


ADAM_CASES = [(step, b1, wd) for step in (0, 1, 9) for b1 in (0.9, 0.4) for wd in (0.0, 0.01)]


@pytest.mark.parametrize("case", ADAM_CASES, ids=lambda c: "step%d-b1_%g-wd%g" % c)
def test_adam_element_is_torch_adam_on_the_cpu(case):
    """No GPU: the restatement against torch.optim.Adam on a one-element float32 CPU parameter -- the step
    counter equal, the rest within the difference between a fused and a rounded product (torch's CPU lerp
    is a fused multiply-add, so bit equality with the kernel's rounded operations cannot hold: on 3 000
    random elements exp_avg differed in the last bit on a fifth of them, exp_avg_sq on 6, the parameter
    never) -- both lerp branches (w1 = 0.1 < 0.5, w1 = 0.6 >= 0.5), with and without weight decay, and
    against float64."""
    step, b1, wd = case
    lr, b2, eps = 3e-4, 0.999, 1e-8
    for p0, g, m0, v0 in ((0.3, -1.7, 0.02, 0.4), (-0.7, 0.33, -0.5, 1e-3), (0.0, 2.5, 0.0, 0.0)):
        if step == 0:
            m0 = v0 = 0.0
        p = torch.nn.Parameter(torch.tensor([p0], dtype=torch.float32))
        opt = torch.optim.Adam([p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, foreach=False)
        opt.state[p] = {"step": torch.tensor(float(step)), "exp_avg": torch.tensor([m0], dtype=torch.float32),
                        "exp_avg_sq": torch.tensor([v0], dtype=torch.float32)}
        p.grad = torch.tensor([g], dtype=torch.float32)
        opt.step()
        st = opt.state[p]
        got = adam_element(p0, g, m0, v0, step, lr, b1, b2, eps, wd)
        want = (p.detach()[0], st["exp_avg"][0], st["exp_avg_sq"][0], st["step"])
        # torch's CPU kernels fuse a product into the addition that follows it (lerp is one fmadd, the
        # compiler may contract add(alpha) and addcmul), the kernel rounds both: x = fl(a + fl(b c)) and
        # x' = fl(a + b c) differ by at most u |b c| + 2 u |x|.  Carried through the update (factor 2):
        f = [float(F32(t)) for t in (p0, g, m0, v0)]
        gi = f[1] + wd * f[0]
        E_gi = (U * abs(wd * f[0]) + 2 * U * abs(gi)) if wd else 0.0
        w1 = 1 - b1
        prod_m = (w1 if w1 < 0.5 else 1 - w1) * abs(gi - f[2])
        E_m = w1 * E_gi + U * prod_m + 2 * U * abs(float(got[1]))
        E_v = 2 * (1 - b2) * abs(gi) * E_gi + U * (1 - b2) * gi * gi + 2 * U * float(got[2])
        denom = math.sqrt(float(got[2])) / math.sqrt(1 - b2 ** (step + 1)) + eps
        ss = lr / (1 - b1 ** (step + 1))
        upd = ss * abs(float(got[1])) / denom
        E_p = ss * E_m / denom + upd * E_v / (2 * max(float(got[2]), 1e-30)) + 4 * U * upd + 2 * U * abs(float(got[0]))
        for name, a, b, E in zip(("p", "exp_avg", "exp_avg_sq", "step"), got, want, (E_p, E_m, E_v, 0.0)):
            assert abs(float(a) - float(b)) <= 2 * E, (name, float(a), float(b), E)
        # float64: the same update without element rounding
        gi = float(F32(g)) + wd * float(F32(p0))
        m64 = b1 * float(F32(m0)) + (1 - b1) * gi
        v64 = b2 * float(F32(v0)) + (1 - b2) * gi * gi
        p64 = float(F32(p0)) - lr / (1 - b1 ** (step + 1)) * m64 / (math.sqrt(v64) / math.sqrt(1 - b2 ** (step + 1)) + eps)
        assert abs(float(got[0]) - p64) <= 4 * U * abs(p64) + 16 * U * lr / (1 - b1 ** (step + 1))


def test_adam_cases_take_both_lerp_branches():
    assert {F32(1.0 - b1) < F32(0.5) for _, b1, _ in ADAM_CASES} == {True, False}
    assert {s for s, _, _ in ADAM_CASES} == {0, 1, 9} and {w for _, _, w in ADAM_CASES} == {0.0, 0.01}


@gpu
@pytest.mark.parametrize("B", SAC_B)
def test_sac_temperature_loss(B):
    dev = _dev()
    g = torch.Generator().manual_seed(7 * B)
    L = _native.lib()
    target = -3.0
    for kind, ltv in (("exact", 0.0), ("randn", 0.0), ("randn", _f(-0.7))):
        lp = _sixteenths(g, B, -64, 64, 0.0625) if kind == "exact" else torch.randn(B, generator=g) * 2
        lt = torch.tensor([ltv], dtype=torch.float32, device=dev)
        loss, lpd = _Guarded(1, dev), lp.to(dev)
        mt.check(L.pfrl_sac_temperature_loss(_p(lt), _p(lpd), target, _p(loss.t), B, _stream()), "temperature loss")
        T = math.exp(ltv)
        terms = T * (lp.double() + target)
        tag = "B%d-%s-logT%g" % (B, kind, ltv)
        if kind == "exact":
            assert bool((terms * 16 == (terms * 16).round()).all()) and float(terms.abs().sum()) < 2 ** 20
            _same("sac_temperature_loss exact", tag, loss.done("loss"), torch.tensor([-(F32(float(terms.sum())) / F32(B))]))
        else:
            relT = 0.0 if ltv == 0.0 else 2 * U
            E = _red_bound(B, 2, terms.abs().sum()) / B + relT * terms.abs().sum() / B
            _within("sac_temperature_loss", tag, loss.done("loss"), (-terms.mean()).reshape(1), (2 * E).reshape(1))


@gpu
@pytest.mark.parametrize("B", [1, 257])
@pytest.mark.parametrize("case", ADAM_CASES, ids=lambda c: "step%d-b1_%g-wd%g" % c)
def test_sac_temperature_step(case, B):
    dev = _dev()
    step, b1, wd = case
    lr, b2, eps, target = 3e-4, 0.999, 1e-8, -3.0
    g = torch.Generator().manual_seed(11 * B + step)
    lp = torch.randn(B, generator=g) * 2
    L = _native.lib()
    p0, m0, v0 = _f(-0.7), (0.0 if step == 0 else _f(0.02)), (0.0 if step == 0 else _f(0.4))
    lpd = lp.to(dev)
    ref_loss = _Guarded(1, dev)
    lt0 = torch.tensor([p0], dtype=torch.float32, device=dev)
    mt.check(L.pfrl_sac_temperature_loss(_p(lt0), _p(lpd), target, _p(ref_loss.t), B, _stream()), "temperature loss")
    st = {k: _Guarded(1, dev) for k in ("log_t", "loss", "m", "v", "step")}
    for k, val in (("log_t", p0), ("m", m0), ("v", v0), ("step", float(step))):
        st[k].t.fill_(val)
    mt.check(L.pfrl_sac_temperature_step(_p(st["log_t"].t), _p(lpd), target, _p(st["loss"].t), _p(st["m"].t), _p(st["v"].t), _p(st["step"].t),
                                         lr, b1, b2, eps, wd, B, _stream()), "temperature step")
    got = {k: t.done(k).cpu() for k, t in st.items()}
    tag = "B%d-step%d-b1_%g-wd%g" % (B, step, b1, wd)
    loss = ref_loss.done("loss").cpu()
    _same("sac_temperature_step loss", tag, got["loss"], loss)
    p, m, v, s = adam_element(p0, float(loss[0]), m0, v0, step, lr, b1, b2, eps, wd)
    _same("sac_temperature_step exp_avg", tag, got["m"], torch.tensor([m]))
    _same("sac_temperature_step exp_avg_sq", tag, got["v"], torch.tensor([v]))
    _same("sac_temperature_step log_temperature", tag, got["log_t"], torch.tensor([p]))
    _same("sac_temperature_step step", tag, got["step"], torch.tensor([s]))
    assert float(got["log_t"][0]) != p0
