"""A2C's fused loss launch: ``pfrl_a2c_loss`` / ``pfrl_a2c_gaussian_loss`` through the C ABI against
float64 torch with autograd on the reference's own expression (pfrl/agents/a2c.py:175-187:
``advantages = returns[:-1] - values``, ``value_loss = (advantages * advantages).mean()``,
``action_loss = -(advantages.detach() * action_log_probs).mean()``, backward of ``value_loss * v_coef +
action_loss * pi_coef - dist_entropy * ent_coef``) on ``Categorical(logits=...)`` /
``Independent(Normal(mean, scale), 1)``, evaluated on the CPU on the same float32 operands.  Method,
helpers and guard zones of tests/test_reinforce.py and tests/test_actor_critic_envelope.py:
``torch.equal`` where the arithmetic is fixed, a derived bound elsewhere, every output and workspace
buffer between NaN guard zones.

u = 2^-24.  Every rounded bound below is first order and is asserted with a factor 2; the assumptions
on the device math library are those of tests/test_actor_critic_envelope.py (``expf`` / ``logf`` 1 ulp
= 2 u relative, division correctly rounded, ``expf(0) == 1``).  The three coefficients reach the kernel
as float32 values the reference uses too; R (``returns[:-1]``) and v (the value column) are float32.

0. What both kernels share.  adv = fl(R - v): u |adv|.  The scale factors inv_m = fl(1 / M) (u),
   c_pi = fl(pi_coef inv_m), c_e = fl(ent_coef inv_m), c_v = fl(fl(2 v_coef) inv_m) (the doubling is
   exact): 2 u relative each.
       dvalue = fl(c_v (-adv)): 2 u + u + u:                          E_dv = 4 u |dvalue|;
       gl = fl(c_pi (-adv)) (= d total / d log pi(a|s)): likewise      4 u |gl|.
   The row terms: sq = fl(adv adv): 2 u from adv, u from the product: 3 u adv^2;
   pol = fl(adv lp_a): |adv| E_lp + u |adv lp_a| (adv) + u |adv lp_a| (the product).
   The sums are float64 per workgroup and per launch (n 2^-53 relative, nothing measurable), divided
   by M in float64, cast once:
       E_value_loss = mean_m 3 u adv_m^2 + u |value_loss|,
       E_action_loss = mean_m (|adv_m| E_lp,m + 2 u |adv_m lp_m|) + u |action_loss|,
       E_entropy = mean_m E_H,m + u |entropy|.

1. ``pfrl_a2c_loss``.  lp, p and H are k_reinforce_loss's: section 1 of tests/test_reinforce.py gives
   eps_e,j, eps_S, E_lse, E_lp,j, eps_p,j and E_H unchanged.  The gradient
   g_j = gl (1[j = a] - p_j) + c_e p_j (lp_j + H): the difference carries p_j eps_p,j + u |.|, gl 4 u, the
   product u; c_e p_j carries eps_p,j + 2 u + u, lp_j + H carries E_lp,j + E_H + u |.|, their product u, the
   sum u:
       E_g,j = |gl| (p_j eps_p,j + 6 u |1[j = a] - p_j|)
             + (ent_coef / M) p_j ((eps_p,j + 5 u) |lp_j + H| + E_lp,j + E_H) + u |g_j|.

2. ``pfrl_a2c_gaussian_loss``.  log pi and H are k_reinforce_gaussian_loss's: section 2 of
   tests/test_reinforce.py gives E_t, E_lp and E_H unchanged.  With g = gl:
       dmean_j = fl(g fl(d / fl(s s))): d, s s, the division and the product u each, g 4 u: 8 u |dmean_j|;
       dscale_j = float32(sum_m g ((double) fl(d d) / s^3 - 1 / s) - ent_coef / s_j), float64 throughout:
       E_dscale,j = sum_m |g_m| (4 u |d^2 / s^3 - 1 / s| + 3 u d^2 / s^3) + u |dscale_j|.

``test_bounds_hold_for_a_float32_emulation_*`` (no GPU) evaluate the same row arithmetic in float32 with
torch on the CPU -- sequential sums over the action dimension as the kernel's loops run them, the tree
sum of gaussian_rows.h for log pi -- and assert these bounds on these very operands before the GPU tests
rely on them.

3. Exact cases.  R == v: adv = +0, every row term and dvalue are zeros, and with ent_coef = 0 so is the
   policy gradient.  Uniform zero logits: A = 1 has lp = H = 0, p = 1; A = 2 has p = 1/2 exactly
   (``expf(0) == 1``), lp_0 = lp_1 = -L with L = logf(2) and H = L/2 + L/2 = L exactly, so lp_j + H = 0 and
   the entropy term of the gradient vanishes for any ent_coef.  With dyadic R and v, M a power of two and
   pi_coef = 1, v_coef = 1/2, every gradient entry and value_loss are exact in float32 and equal the
   float64 closed form (``ops.a2c_loss_closed_form``).  entropy = L and action_loss = -mean fl(adv (-L))
   depend on the device's logf(2): L is asserted within 2 u ln 2 (factor 2) of ln 2, and action_loss
   must equal, bit for bit, the closed form evaluated with that L (float32 products, an exact float64
   sum of M <= 512 products of a few bits each, an exact division by M, one cast).
   The statistics: ``avg + (1 - decay) * (x - avg)`` in float32 torch on the launch's own out3.
"""
import functools

import pytest
import torch
from torch.distributions import Categorical, Independent, Normal

from pfrl_amd import _native, ops
from test_actor_critic_envelope import (F64, PFRL_ERR_ARG, U, _cd, _dev, _f, _Guarded, _p, _same,
                                        _stream, _within)
from test_reinforce import C_ENT, C_LP, GAUSSIAN_A, M_LIST, SOFTMAX_A, _tree_sum
from pfrl_amd.nn import mfma_trunk as mt

gpu = pytest.mark.gpu

COEFS = [(1.0, 0.5, _f(0.01)), (1.0, 0.5, 0.0), (_f(0.7), 0.25, _f(0.02))]      # (pi, v, ent)
DECAY = (_f(0.999), _f(0.99), _f(0.9))
AVG0 = torch.tensor([0.3, -1.7, 2.2], dtype=torch.float32)
LN2 = 0.6931471805599453


def test_case_lists_are_the_ones_the_kernels_were_specified_for():
    """The census: every listed M and A is reached by the parametrised GPU tests and by the CPU
    emulation (both run over exactly these lists), three coefficient triples, dscale and avg each
    present and NULL."""
    assert M_LIST == [1, 63, 64, 65, 257, 2053]
    assert SOFTMAX_A == [1, 2, 9, 31] and GAUSSIAN_A == [1, 3, 32]
    assert COEFS == [(1.0, 0.5, _f(0.01)), (1.0, 0.5, 0.0), (_f(0.7), 0.25, _f(0.02))]
    assert {_cd(M, 256) for M in M_LIST} == {1, 2, 9}          # one block, two, many
    reached = {(M, A) for M in M_LIST for A in SOFTMAX_A}
    assert len(reached) == 24 and len({(M, A) for M in M_LIST for A in GAUSSIAN_A}) == 18
    assert sorted(_variants()) == [(False, False), (False, True), (True, False), (True, True)]


def _variants():
    """(dscale present, avg present)"""
    return [(d, a) for d in (True, False) for a in (True, False)]


# ================================================================== 1. pfrl_a2c_loss
@functools.lru_cache(maxsize=None)
def _softmax_operands(M, A):
    g = torch.Generator().manual_seed(104729 * M + A)
    v = torch.randn(M, generator=g)
    return {"z": 2 * torch.randn(M, A, generator=g), "value": v,
            "action": torch.randint(0, A, (M,), generator=g).float(),
            "ret": v + 2 * torch.randn(M, generator=g)}


def _shared_bounds(adv, lpa, E_lp, E_H, out3):
    """section 0: the bounds of out3 (no factor 2)"""
    E_vl = (3 * U * adv * adv).mean() + U * out3[0].abs()
    E_al = (adv.abs() * E_lp + 2 * U * (adv * lpa).abs()).mean() + U * out3[1].abs()
    E_ent = E_H.mean() + U * out3[2].abs()
    return torch.stack([E_vl, E_al, E_ent])


@functools.lru_cache(maxsize=None)
def _softmax_reference(M, A, coefs):
    """float64 + autograd on the reference expression, and the bounds of sections 0 and 1."""
    pi_c, v_c, e_c = coefs
    o = _softmax_operands(M, A)
    z = o["z"].double().requires_grad_(True)
    v = o["value"].double().requires_grad_(True)
    a, R = o["action"].long(), o["ret"].double()
    dist = Categorical(logits=z)
    lpa, H = dist.log_prob(a), dist.entropy()
    adv = R - v
    value_loss = (adv * adv).mean()
    action_loss = -(adv.detach() * lpa).mean()
    ent = H.mean()
    dz, dv = torch.autograd.grad(value_loss * v_c + action_loss * pi_c - ent * e_c, [z, v])
    z, adv, lpa, H = z.detach(), adv.detach(), lpa.detach(), H.detach()
    ar = torch.arange(M)
    mx = z.max(1, keepdim=True).values
    lse = torch.logsumexp(z, 1, keepdim=True)
    lp = z - lse
    p = lp.exp()
    eps_e = (2 + (z - mx).abs()) * U
    eps_S = (p * eps_e).sum(1, keepdim=True) + (A - 1) * U
    E_lse = eps_S + 2 * U * (lse - mx).abs() + U * lse.abs()
    E_lp = E_lse + U * lp.abs()
    eps_p = eps_e + eps_S + U
    Hc = H[:, None]
    E_H = (p * ((eps_p + U) * lp.abs() + E_lp)).sum(1, keepdim=True) + (A - 1) * U * (p * lp.abs()).sum(1, keepdim=True)
    oh = torch.zeros_like(z)
    oh[ar, a] = 1.0
    gl, ge = (pi_c * adv / M).abs()[:, None], e_c / M
    E_g = (gl * (p * eps_p + 6 * U * (oh - p).abs())
           + ge * p * ((eps_p + 5 * U) * (lp + Hc).abs() + E_lp + E_H) + U * dz.abs())
    out3 = torch.stack([value_loss.detach(), action_loss.detach(), ent.detach()])
    return {"out3": out3, "dz": dz, "dv": dv, "E_dz": E_g, "E_dv": 4 * U * dv.abs(),
            "E_out3": _shared_bounds(adv, lpa, E_lp[ar, a], E_H[:, 0], out3)}


def _coefs32(M, coefs):
    f = torch.float32
    pi_c, v_c, e_c = (torch.tensor(c, dtype=f) for c in coefs)
    inv_m = torch.tensor(1.0, dtype=f) / torch.tensor(float(M), dtype=f)
    return pi_c * inv_m, (2 * v_c) * inv_m, e_c * inv_m


def _out3_of(sq, pol, H, M):
    return torch.stack([(sq.double().sum() / M).float(), (-(pol.double().sum()) / M).float(),
                        (H.double().sum() / M).float()])


def _emulate_softmax(o, coefs):
    """The row arithmetic of k_a2c_loss in float32 torch on the CPU, loops over the action dimension in
    the kernel's order; the batch sums in float64."""
    z, v, a, R = o["z"], o["value"], o["action"].long(), o["ret"]
    M, A = z.shape
    f = torch.float32
    c_pi, c_v, c_e = _coefs32(M, coefs)
    mx = z.max(1).values
    e = torch.exp(z - mx[:, None])
    s = torch.zeros(M, dtype=f)
    for j in range(A):
        s = s + e[:, j]
    lse = mx + torch.log(s)
    lp = z - lse[:, None]
    p = e / s[:, None]
    H = torch.zeros(M, dtype=f)
    for j in range(A):
        H = H - torch.where(p[:, j] > 0, p[:, j] * lp[:, j], torch.zeros(M, dtype=f))
    lpa = lp[torch.arange(M), a]
    adv = R - v
    gl = c_pi * (-adv)
    oh = torch.zeros_like(z)
    oh[torch.arange(M), a] = 1.0
    g = gl[:, None] * (oh - p) + torch.where(p > 0, c_e * p * (lp + H[:, None]), torch.zeros_like(p))
    dv = c_v * (-adv)
    assert g.dtype == f and dv.dtype == f
    return {"out3": _out3_of(adv * adv, adv * lpa, H, M), "dz": g, "dv": dv}


def _stats_args(dev, with_avg):
    avg = _Guarded(3, dev)
    if with_avg:
        avg.t.copy_(AVG0)
    return avg, (_p(avg.t) if with_avg else None)


def _check_stats(name, tag, out, with_avg):
    """the float32 sequence of A2C.update on the launch's own out3, bit for bit; NULL: nothing written"""
    avg = out.pop("avg")
    if not with_avg:
        avg.untouched(name + " avg")
        return
    x = out["out3"].cpu()[[1, 0, 2]]
    want = AVG0 + (1 - torch.tensor(DECAY, dtype=torch.float32)) * (x - AVG0)
    assert want.dtype == torch.float32
    _same(name + " avg", tag, avg.done(name + " avg"), want)


def _run_softmax(dev, o, M, A, coefs, with_avg=False):
    nb = _cd(M, 256)
    out = {"dz": _Guarded(M * A, dev), "dv": _Guarded(M, dev), "ws": _Guarded(3 * nb, dev, F64),
           "out3": _Guarded(3, dev)}
    avg, avg_p = _stats_args(dev, with_avg)
    mt.check(_native.lib().pfrl_a2c_loss(
        _p(o["z"]), _p(o["value"]), _p(o["action"]), _p(o["ret"]), M, A, coefs[0], coefs[1], coefs[2],
        _p(out["dz"].t), _p(out["dv"].t), _p(out["ws"].t), _p(out["out3"].t), avg_p, DECAY[0], DECAY[1],
        DECAY[2], _stream()), "a2c_loss")
    torch.cuda.synchronize()
    got = {k: t.guards(k) for k, t in out.items()}
    got["avg"] = avg
    return got


def _check_softmax(name, tag, got, r):
    _within(name + " dlogits", tag, got["dz"], r["dz"], 2 * r["E_dz"] + 1e-300)
    _within(name + " dvalue", tag, got["dv"], r["dv"], 2 * r["E_dv"] + 1e-300)
    _within(name + " out3", tag, got["out3"], r["out3"], 2 * r["E_out3"] + 1e-300)


# ================================================================== 2. pfrl_a2c_gaussian_loss
@functools.lru_cache(maxsize=None)
def _gaussian_operands(M, A):
    g = torch.Generator().manual_seed(15485863 * M + A)
    mean = torch.randn(M, A, generator=g)
    scale = torch.exp(0.3 * torch.randn(A, generator=g))
    v = torch.randn(M, generator=g)
    return {"mean": mean, "scale": scale, "value": v,
            "action": mean + scale * torch.randn(M, A, generator=g),
            "ret": v + 2 * torch.randn(M, generator=g)}


@functools.lru_cache(maxsize=None)
def _gaussian_reference(M, A, coefs):
    pi_c, v_c, e_c = coefs
    o = _gaussian_operands(M, A)
    mean = o["mean"].double().requires_grad_(True)
    scale = o["scale"].double().requires_grad_(True)
    v = o["value"].double().requires_grad_(True)
    a, R = o["action"].double(), o["ret"].double()
    dist = Independent(Normal(mean, scale.expand_as(mean)), 1)
    lpa, H = dist.log_prob(a), dist.entropy()
    adv = R - v
    value_loss = (adv * adv).mean()
    action_loss = -(adv.detach() * lpa).mean()
    ent = H.mean()
    dmean, dscale, dv = torch.autograd.grad(value_loss * v_c + action_loss * pi_c - ent * e_c,
                                            [mean, scale, v])
    mean, s, adv, lpa, Hd = mean.detach(), scale.detach(), adv.detach(), lpa.detach(), H.detach()
    d = a - mean
    q = d * d / (2 * s * s)
    log_s = s.log()
    t = -q - log_s - C_LP
    E_t = 5 * U * q + 2 * U * log_s.abs() + U * (q + log_s).abs() + U * C_LP + U * t.abs()
    E_lp = E_t.sum(1) + 6 * U * t.abs().sum(1)
    E_H = (2 * U * log_s.abs() + U * C_ENT + U * (C_ENT + log_s).abs()).sum() + U * Hd.abs()
    g = (pi_c * adv / M).abs()[:, None]
    E_dscale = (g * (4 * U * (d * d / s ** 3 - 1 / s).abs() + 3 * U * d * d / s ** 3)).sum(0) + U * dscale.abs()
    out3 = torch.stack([value_loss.detach(), action_loss.detach(), ent.detach()])
    return {"out3": out3, "dmean": dmean, "dscale": dscale, "dv": dv,
            "E_out3": _shared_bounds(adv, lpa, E_lp, E_H, out3),
            "E_dmean": 8 * U * dmean.abs(), "E_dscale": E_dscale, "E_dv": 4 * U * dv.abs()}


def _emulate_gaussian(o, coefs):
    mean, s, v, a, R = o["mean"], o["scale"], o["value"], o["action"], o["ret"]
    M, A = mean.shape
    f = torch.float32
    c_pi, c_v, c_e = _coefs32(M, coefs)
    c_lp, c_ent = torch.tensor(C_LP, dtype=f), torch.tensor(C_ENT, dtype=f)
    d = a - mean
    log_s = torch.log(s)
    t = (-(d * d) / (2 * (s * s)) - log_s) - c_lp
    lpa = _tree_sum(t)
    H = (c_ent + log_s).double().sum().float()
    adv = R - v
    g = c_pi * (-adv)
    dmean = g[:, None] * (d / (s * s))
    dv = c_v * (-adv)
    sd = s.double()
    terms = g.double()[:, None] * ((d * d).double() / (sd * sd * sd) - 1.0 / sd)
    dscale = (terms.sum(0) - float(coefs[2]) / sd).float()
    assert dmean.dtype == f and dv.dtype == f
    return {"out3": _out3_of(adv * adv, adv * lpa, H.expand(M), M), "dmean": dmean, "dv": dv,
            "dscale": dscale}


def _run_gaussian(dev, o, M, A, coefs, want_dscale=True, with_avg=False):
    nb = _cd(M, 256)
    out = {"dmean": _Guarded(M * A, dev), "dv": _Guarded(M, dev), "dscale": _Guarded(A, dev),
           "ws": _Guarded((3 + A) * nb, dev, F64), "out3": _Guarded(3, dev)}
    avg, avg_p = _stats_args(dev, with_avg)
    mt.check(_native.lib().pfrl_a2c_gaussian_loss(
        _p(o["mean"]), _p(o["scale"]), _p(o["value"]), _p(o["action"]), _p(o["ret"]), M, A, coefs[0],
        coefs[1], coefs[2], _p(out["dmean"].t), _p(out["dv"].t),
        _p(out["dscale"].t) if want_dscale else None, _p(out["ws"].t), _p(out["out3"].t), avg_p,
        DECAY[0], DECAY[1], DECAY[2], _stream()), "a2c_gaussian_loss")
    torch.cuda.synchronize()
    if not want_dscale:
        out.pop("dscale").untouched("dscale")
    got = {k: t.guards(k) for k, t in out.items()}
    got["avg"] = avg
    return got


def _check_gaussian(name, tag, got, r):
    _within(name + " dmean", tag, got["dmean"], r["dmean"], 2 * r["E_dmean"] + 1e-300)
    _within(name + " dvalue", tag, got["dv"], r["dv"], 2 * r["E_dv"] + 1e-300)
    _within(name + " out3", tag, got["out3"], r["out3"], 2 * r["E_out3"] + 1e-300)
    if "dscale" in got:
        _within(name + " dscale", tag, got["dscale"], r["dscale"], 2 * r["E_dscale"] + 1e-300)


# ------------------------------------------------------------------ no GPU: bounds, closed forms
@pytest.mark.parametrize("A", SOFTMAX_A)
def test_bounds_hold_for_a_float32_emulation_of_the_softmax_rows(A):
    for M in M_LIST:
        for coefs in COEFS:
            got = _emulate_softmax(_softmax_operands(M, A), coefs)
            _check_softmax("emulated a2c_loss", "M%d-A%d-%s" % (M, A, coefs), got,
                           _softmax_reference(M, A, coefs))


@pytest.mark.parametrize("A", GAUSSIAN_A)
def test_bounds_hold_for_a_float32_emulation_of_the_gaussian_rows(A):
    for M in M_LIST:
        for coefs in COEFS:
            got = _emulate_gaussian(_gaussian_operands(M, A), coefs)
            _check_gaussian("emulated a2c_gaussian_loss", "M%d-A%d-%s" % (M, A, coefs), got,
                            _gaussian_reference(M, A, coefs))


def _close64(name, got, want):
    assert got.dtype == F64 and got.shape == want.shape, name
    assert bool(((got - want).abs() <= 1e-12 * (1 + want.abs())).all()), name


@pytest.mark.parametrize("coefs", COEFS)
def test_closed_forms_are_what_float64_autograd_computes(coefs):
    for M, A in ((1, 1), (65, 9), (257, 31)):
        o, r = _softmax_operands(M, A), _softmax_reference(M, A, coefs)
        out3, dz, dv = ops.a2c_loss_closed_form(o["z"].double(), o["value"].double(), o["action"],
                                                o["ret"].double(), *coefs)
        for name, got, want in (("out3", out3, r["out3"]), ("dlogits", dz, r["dz"]), ("dvalue", dv, r["dv"])):
            _close64("a2c_loss_closed_form %s M%d A%d" % (name, M, A), got, want)
    for M, A in ((1, 1), (65, 3), (257, 32)):
        o, r = _gaussian_operands(M, A), _gaussian_reference(M, A, coefs)
        out3, dmean, dv, dscale = ops.a2c_gaussian_loss_closed_form(
            o["mean"].double(), o["scale"].double(), o["value"].double(), o["action"].double(),
            o["ret"].double(), *coefs)
        for name, got, want in (("out3", out3, r["out3"]), ("dmean", dmean, r["dmean"]),
                                ("dvalue", dv, r["dv"]), ("dscale", dscale, r["dscale"])):
            _close64("a2c_gaussian_loss_closed_form %s M%d A%d" % (name, M, A), got, want)


def test_the_python_gate_needs_no_gpu_to_refuse():
    z, v = torch.zeros(4, 3), torch.zeros(4)
    assert not ops.a2c_loss_supported("softmax", z, v, v, v)            # (not on a GPU)
    assert not ops.a2c_loss_supported("beta", z, v, v, v)


# ------------------------------------------------------------------ kernels against float64
def _on(dev, o):
    return {k: t.to(dev).contiguous() for k, t in o.items()}


@gpu
@pytest.mark.parametrize("A", SOFTMAX_A)
@pytest.mark.parametrize("M", M_LIST)
def test_a2c_loss_matches_float64(M, A):
    dev = _dev()
    o = _on(dev, _softmax_operands(M, A))
    for i, coefs in enumerate(COEFS):
        r = _softmax_reference(M, A, coefs)
        for with_avg in (True, False) if i == 0 else (i == 1,):
            tag = "M%d-A%d-%s-avg%d" % (M, A, coefs, with_avg)
            got = _run_softmax(dev, o, M, A, coefs, with_avg)
            _check_stats("a2c_loss", tag, got, with_avg)
            assert not any(bool(torch.isnan(got[k]).any()) for k in ("dz", "dv", "out3", "ws"))
            _check_softmax("a2c_loss", tag, got, r)


@gpu
@pytest.mark.parametrize("A", GAUSSIAN_A)
@pytest.mark.parametrize("M", M_LIST)
def test_a2c_gaussian_loss_matches_float64(M, A):
    dev = _dev()
    o = _on(dev, _gaussian_operands(M, A))
    for i, coefs in enumerate(COEFS):
        r = _gaussian_reference(M, A, coefs)
        for want_dscale, with_avg in _variants() if i == 0 else [(i == 1, i == 2)]:
            tag = "M%d-A%d-%s-dscale%d-avg%d" % (M, A, coefs, want_dscale, with_avg)
            got = _run_gaussian(dev, o, M, A, coefs, want_dscale, with_avg)
            _check_stats("a2c_gaussian_loss", tag, got, with_avg)
            assert not any(bool(torch.isnan(t).any()) for t in got.values())
            _check_gaussian("a2c_gaussian_loss", tag, got, r)


@gpu
def test_ops_wrappers_return_what_the_entry_points_write():
    dev = _dev()
    M, A, coefs = 257, 9, COEFS[0]
    o = _on(dev, _softmax_operands(M, A))
    avg = AVG0.to(dev)
    out3, dz, dv = ops.a2c_loss(o["z"], o["value"].view(M, 1), o["action"], o["ret"], *coefs, avg=avg,
                                decay=DECAY)
    raw = _run_softmax(dev, o, M, A, coefs, True)
    assert torch.equal(out3, raw["out3"]) and torch.equal(dz.view(-1), raw["dz"]) and dz.shape == (M, A)
    assert torch.equal(dv.view(-1), raw["dv"]) and dv.shape == (M, 1) and torch.equal(avg, raw["avg"].t)
    assert ops.a2c_loss_supported("softmax", o["z"], o["value"], o["action"], o["ret"])
    M, A = 257, 3
    o = _on(dev, _gaussian_operands(M, A))
    avg = AVG0.to(dev)
    out3, dmean, dv, dscale = ops.a2c_gaussian_loss(o["mean"], o["scale"], o["value"], o["action"],
                                                    o["ret"], *coefs, avg=avg, decay=DECAY)
    raw = _run_gaussian(dev, o, M, A, coefs, True, True)
    assert torch.equal(out3, raw["out3"]) and torch.equal(dmean.view(-1), raw["dmean"])
    assert torch.equal(dv, raw["dv"]) and torch.equal(dscale, raw["dscale"])
    assert torch.equal(avg, raw["avg"].t)
    assert ops.a2c_gaussian_loss(o["mean"], o["scale"], o["value"], o["action"], o["ret"], *coefs,
                                 want_dscale=False)[3] is None
    assert ops.a2c_loss_supported("gaussian", o["mean"], o["value"], o["action"], o["ret"])


# ------------------------------------------------------------------ exact cases
def _all_zero(t):
    return bool((t == 0).all())


@gpu
def test_returns_equal_to_the_values_give_exact_zeros():
    dev = _dev()
    for M, A in ((65, 9), (257, 31)):
        o = _on(dev, _softmax_operands(M, A))
        o["ret"] = o["value"].clone()
        for coefs in COEFS:
            got = _run_softmax(dev, o, M, A, coefs)
            vl = got["out3"][0:1].cpu()
            assert torch.equal(vl, torch.zeros(1)) and not bool(torch.signbit(vl).any())
            assert _all_zero(got["dv"]) and _all_zero(got["out3"][1])
            if coefs[2] == 0.0:
                assert _all_zero(got["dz"])
    for M, A in ((65, 3), (257, 32)):
        o = _on(dev, _gaussian_operands(M, A))
        o["ret"] = o["value"].clone()
        for coefs in COEFS:
            got = _run_gaussian(dev, o, M, A, coefs)
            vl = got["out3"][0:1].cpu()
            assert torch.equal(vl, torch.zeros(1)) and not bool(torch.signbit(vl).any())
            assert _all_zero(got["dv"]) and _all_zero(got["out3"][1])
            if coefs[2] == 0.0:
                assert _all_zero(got["dmean"]) and _all_zero(got["dscale"])


@gpu
@pytest.mark.parametrize("M", [64, 512])
@pytest.mark.parametrize("A", [1, 2])
def test_uniform_zero_logits_and_dyadic_columns_give_the_closed_form(M, A):
    """Section 3 of the module docstring."""
    dev = _dev()
    g = torch.Generator().manual_seed(M + A)
    o = {"z": torch.zeros(M, A), "value": torch.randint(-16, 17, (M,), generator=g).float() / 8,
         "action": torch.randint(0, A, (M,), generator=g).float(),
         "ret": torch.randint(-16, 17, (M,), generator=g).float() / 4}
    adv64 = o["ret"].double() - o["value"].double()
    oh = torch.nn.functional.one_hot(o["action"].long(), A).double()
    for coefs in COEFS[:2]:
        tag = "M%d-A%d-%s" % (M, A, coefs)
        # the closed form at p_j = 1 / A, lp_j + H = 0
        dz = -coefs[0] * adv64[:, None] * (oh - 1.0 / A) / M
        dv = coefs[1] * 2 * -adv64 / M
        out3 = torch.stack([(adv64 * adv64).mean()])
        general = ops.a2c_loss_closed_form(o["z"].double(), o["value"].double(), o["action"],
                                           o["ret"].double(), *coefs)
        _close64("closed form dlogits", general[1], dz)
        _close64("closed form dvalue", general[2], dv)
        _close64("closed form value_loss", general[0][:1], out3)
        assert torch.equal(dz.float().double(), dz) and torch.equal(dv.float().double(), dv)
        assert torch.equal(out3[0].float().double(), out3[0])
        got = _run_softmax(dev, _on(dev, o), M, A, coefs)
        _same("a2c_loss dyadic dlogits", tag, got["dz"].view(M, A), dz.float())
        _same("a2c_loss dyadic dvalue", tag, got["dv"], dv.float())
        _same("a2c_loss dyadic value_loss", tag, got["out3"][0], out3[0].float())
        L = got["out3"][2].cpu()
        adv = o["ret"] - o["value"]
        if A == 1:
            assert float(L) == 0.0 and float(got["out3"][1]) == 0.0
        else:
            assert abs(float(L) - LN2) <= 2 * (2 * U * LN2)
            want = (-((adv * (-L)).double().sum()) / M).float()
            _same("a2c_loss dyadic action_loss", tag, got["out3"][1], want)


@gpu
def test_two_calls_on_the_same_operands_give_the_same_bits():
    dev = _dev()
    M = 2053
    o = _on(dev, _softmax_operands(M, 31))
    a, b = _run_softmax(dev, o, M, 31, COEFS[0], True), _run_softmax(dev, o, M, 31, COEFS[0], True)
    assert torch.equal(a.pop("avg").t, b.pop("avg").t)
    assert all(torch.equal(a[k], b[k]) for k in a)
    o = _on(dev, _gaussian_operands(M, 32))
    a, b = _run_gaussian(dev, o, M, 32, COEFS[0], True, True), _run_gaussian(dev, o, M, 32, COEFS[0], True, True)
    assert torch.equal(a.pop("avg").t, b.pop("avg").t)
    assert all(torch.equal(a[k], b[k]) for k in a)


@gpu
def test_nan_logit_stays_in_its_own_row_of_the_gradients():
    dev = _dev()
    M, bad = 257, 70
    keep = torch.arange(M, device=dev) != bad
    for A in (1, 9):
        o = _on(dev, _softmax_operands(M, A))
        clean = _run_softmax(dev, o, M, A, COEFS[0])
        o["z"] = o["z"].clone()
        o["z"][bad, A - 1] = float("nan")
        got = _run_softmax(dev, o, M, A, COEFS[0])
        dz, dz0 = got["dz"].view(M, A), clean["dz"].view(M, A)
        assert torch.equal(dz[keep], dz0[keep]) and torch.equal(got["dv"], clean["dv"])
        assert bool(torch.isnan(dz[bad]).all())
        assert torch.equal(got["out3"][0], clean["out3"][0])        # (the value loss reads no logit)
    A = 3
    o = _on(dev, _gaussian_operands(M, A))
    clean = _run_gaussian(dev, o, M, A, COEFS[0])
    o["mean"] = o["mean"].clone()
    o["mean"][bad, 1] = float("nan")
    got = _run_gaussian(dev, o, M, A, COEFS[0])
    dm, dm0 = got["dmean"].view(M, A), clean["dmean"].view(M, A)
    assert torch.equal(dm[keep], dm0[keep]) and torch.equal(got["dv"], clean["dv"])
    assert bool(torch.isnan(dm[bad, 1])) and torch.equal(got["out3"][0], clean["out3"][0])


@gpu
def test_an_action_outside_the_range_matches_no_logit_and_indexes_nothing():
    """1[j = a] is zero for every j: the row's gradient is that of lp_a = 0, nothing outside the
    guarded buffers is touched, every other row is unchanged."""
    dev = _dev()
    M, A, bad = 65, 9, 7
    o = _on(dev, _softmax_operands(M, A))
    clean = _run_softmax(dev, o, M, A, COEFS[0])
    keep = torch.arange(M, device=dev) != bad
    for value in (-1.0, float(A), 1e30, float("nan"), float("-inf")):
        o["action"] = o["action"].clone()
        o["action"][bad] = value
        got = _run_softmax(dev, o, M, A, COEFS[0])
        dz, dz0 = got["dz"].view(M, A), clean["dz"].view(M, A)
        assert torch.equal(dz[keep], dz0[keep]) and not bool(torch.isnan(dz).any())


# ------------------------------------------------------------------ gates
@gpu
def test_out_of_range_arguments_are_rejected_before_any_launch():
    dev = _dev()
    L = _native.lib()
    M, A = 8, 4
    o = _on(dev, _softmax_operands(M, A))
    dz, dv, ws, out3, avg = (_Guarded(M * 33, dev), _Guarded(M, dev), _Guarded(64, dev, F64),
                             _Guarded(3, dev), _Guarded(3, dev))
    a = [_p(o["z"]), _p(o["value"]), _p(o["action"]), _p(o["ret"]), M, A, 1.0, 0.5, 0.0, _p(dz.t),
         _p(dv.t), _p(ws.t), _p(out3.t), _p(avg.t), DECAY[0], DECAY[1], DECAY[2], _stream()]
    for M_, A_ in ((M, 0), (M, 32), (0, A), (-1, A)):
        b = list(a)
        b[4], b[5] = M_, A_
        assert L.pfrl_a2c_loss(*b) == PFRL_ERR_ARG
    for i in (0, 1, 2, 3, 9, 10, 11, 12):
        b = list(a)
        b[i] = None
        assert L.pfrl_a2c_loss(*b) == PFRL_ERR_ARG
    g = _on(dev, _gaussian_operands(M, 3))
    ga = [_p(g["mean"]), _p(g["scale"]), _p(g["value"]), _p(g["action"]), _p(g["ret"]), M, 3, 1.0, 0.5,
          0.0, _p(dz.t), _p(dv.t), None, _p(ws.t), _p(out3.t), _p(avg.t), DECAY[0], DECAY[1], DECAY[2],
          _stream()]
    for M_, A_ in ((M, 0), (M, 33), (0, 3), (-1, 3)):
        b = list(ga)
        b[5], b[6] = M_, A_
        assert L.pfrl_a2c_gaussian_loss(*b) == PFRL_ERR_ARG
    for i in (0, 1, 2, 3, 4, 10, 11, 13, 14):
        b = list(ga)
        b[i] = None
        assert L.pfrl_a2c_gaussian_loss(*b) == PFRL_ERR_ARG
    torch.cuda.synchronize()
    for t in (dz, dv, ws, out3, avg):
        t.untouched("an output of a rejected call")


@gpu
def test_the_python_gate_is_inside_the_c_gate():
    """Whatever ``ops.a2c_loss_supported`` admits the entry point accepts (A = 0 .. 34, both kinds);
    other dtypes, strides and row counts are refused in Python."""
    dev = _dev()
    L = _native.lib()
    M = 5
    v = torch.zeros(M, device=dev)
    admitted = {"softmax": [], "gaussian": []}
    for kind in admitted:
        for A in range(0, 35):
            z = torch.zeros(M, A, device=dev)
            act = torch.zeros((M,) if kind == "softmax" else (M, A), device=dev)
            if not ops.a2c_loss_supported(kind, z, v, act, v):
                continue
            admitted[kind].append(A)
            dz, dv, out3 = _Guarded(M * A, dev), _Guarded(M, dev), _Guarded(3, dev)
            ws = _Guarded(3 if kind == "softmax" else 3 + A, dev, F64)
            if kind == "softmax":
                rc = L.pfrl_a2c_loss(_p(z), _p(v), _p(act), _p(v), M, A, 1.0, 0.5, 0.0, _p(dz.t), _p(dv.t),
                                     _p(ws.t), _p(out3.t), None, 0.0, 0.0, 0.0, _stream())
            else:
                s = torch.ones(A, device=dev)
                rc = L.pfrl_a2c_gaussian_loss(_p(z), _p(s), _p(v), _p(act), _p(v), M, A, 1.0, 0.5, 0.0,
                                              _p(dz.t), _p(dv.t), None, _p(ws.t), _p(out3.t), None, 0.0,
                                              0.0, 0.0, _stream())
            assert rc == 0, (kind, A)
            torch.cuda.synchronize()
            for name, t in (("dz", dz), ("dv", dv), ("ws", ws), ("out3", out3)):
                t.done(name)
    assert admitted == {"softmax": list(range(1, 32)), "gaussian": list(range(1, 33))}
    z, act = torch.zeros(M, 4, device=dev), torch.zeros(M, device=dev)
    assert ops.a2c_loss_supported("softmax", z, v, act, v)
    assert not ops.a2c_loss_supported("softmax", z.double(), v, act, v)
    assert not ops.a2c_loss_supported("softmax", z, v, act.long(), v)
    assert not ops.a2c_loss_supported("softmax", torch.zeros(M, 8, device=dev)[:, ::2], v, act, v)
    assert not ops.a2c_loss_supported("softmax", z, v[:-1], act, v)
    assert not ops.a2c_loss_supported("softmax", z, v, act, v.cpu())
    assert not ops.a2c_loss_supported("gaussian", z, v, act, v)         # (one action per dimension)
