"""REINFORCE on the device: ``pfrl_reinforce_loss`` / ``pfrl_reinforce_gaussian_loss`` through the C ABI
against float64 torch with autograd on the reference's own expression
(``(-R log pi(a|s) - beta H).sum() / batchsize`` on ``Categorical(logits=...)`` /
``Independent(Normal(mean, scale), 1)``) evaluated on the same float32 operands, and the agent's device
route against the trace of the reference (tests/golden/make_reinforce_fixtures.py).  Method and helpers
of tests/test_actor_critic_envelope.py: ``torch.equal`` where the arithmetic is fixed, a derived bound
elsewhere, every output and workspace buffer between NaN guard zones.

u = 2^-24.  Every rounded bound below is first order and is asserted with a factor 2; the assumptions
on the device math library are those of tests/test_actor_critic_envelope.py (``expf`` / ``logf`` 1 ulp
= 2 u relative, division correctly rounded, ``expf(0) == 1``).  inv_b (= 1 / batchsize) and beta reach
the kernel as float32 values the reference uses too, R is the float32 return column.

1. ``pfrl_reinforce_loss``.  With d_j = z_j - max, p = softmax(z), lp = log_softmax(z), section 1 of
   tests/test_actor_critic_envelope.py applies unchanged (E_z = 0):
       eps_e,j = (2 + |d_j|) u,   eps_S = sum_j p_j eps_e,j + (A - 1) u,
       E_lse = eps_S + 2 u |log sum| + u |lse|,   E_lp,j = E_lse + u |lp_j|,   eps_p,j = eps_e,j + eps_S + u,
       E_H = sum_j p_j ((eps_p,j + u) |lp_j| + E_lp,j) + (A - 1) u sum_j p_j |lp_j|.
   The row: t1 = fl(fl(-R) lp_a) (-R is exact), t2 = fl(beta H), row = fl(t1 - t2):
       E_row = |R| E_lp,a + u |R lp_a| + beta E_H + u beta |H| + u |row|.
   The sums are float64 per workgroup and per launch (n 2^-53 relative, nothing measurable), the loss
   is their product with inv_b in float64, cast once, the mean entropy likewise:
       E_loss = inv_b sum_m E_row,m + u |loss|,   E_ent = mean_m E_H,m + u |ent|.
   The gradient g_j = gl (1[j = a] - p_j) + ge p_j (lp_j + H) with gl = fl(inv_b (-R)), ge = fl(beta inv_b)
   (u each): the difference 1[j = a] - p_j carries p_j eps_p,j + u |.|, the first product u more; ge p_j
   carries eps_p,j + 2 u, lp_j + H carries E_lp,j + E_H + u |.|, their product u, the sum u:
       E_g,j = |gl| (p_j eps_p,j + 3 u |1[j = a] - p_j|)
             + ge p_j ((eps_p,j + 4 u) |lp_j + H| + E_lp,j + E_H) + u |g_j|.

2. ``pfrl_reinforce_gaussian_loss``.  Per element d = fl(a - mu) (u), q = fl(fl(d d) / fl(2 fl(s s)))
   (5 u), log s (2 u |log s|), t = fl(fl(-q - log s) - c) with c = fl(log sqrt(2 pi)):
       E_t = 5 u q + 2 u |log s| + u |q + log s| + u c + u |t|;
   log pi is the tree sum of csrc/gaussian_rows.h, at most 6 additions on any path:
       E_lp = sum_j E_t,j + 6 u sum_j |t_j|.
   The entropy sums fl(C + logf(s_j)) in float64 and casts once:
       E_H = sum_j (2 u |log s_j| + u C + u |C + log s_j|) + u |H|.
   E_row, E_loss, E_ent as in 1. with these.  With g = fl(inv_b (-R)):
       dmean_j = fl(g fl(d / fl(s s))): d, s s, the division, g and the product round once each: 5 u |dmean_j|;
       dscale_j = float32(sum_m g ((double) fl(d d) / s^3 - 1 / s) - beta M inv_b / s_j), float64 throughout:
       E_dscale,j = sum_m |g_m| (u |d^2 / s^3 - 1 / s| + 3 u d^2 / s^3) + u |dscale_j|.

``test_bounds_hold_for_a_float32_emulation`` (no GPU) evaluates the same row arithmetic in float32 with
torch on the CPU -- sequential sums over the action dimension as the kernel's loops run them, the tree
sum of gaussian_rows.h for log pi -- and asserts these bounds on these very operands before the GPU
tests rely on them.

3. The agent.  The device route is teacher-forced on the reference's trace: the loss of every
   ``accumulate_grad`` call within 1e-5 (the teacher-forced standard of tests/test_teacher_forced_loss.py),
   the gradient before clipping and the parameters after the step within the fixture's measured
   ``*_grad_tol`` / ``*_param_tol`` (ten times the reference's own float32 - float64 difference).
"""
import functools
import os

import numpy as np
import pytest
import torch
from torch.distributions import Categorical, Independent, Normal

from pfrl_amd import _native, ops
from test_actor_critic_envelope import (F64, PFRL_ERR_ARG, U, _cd, _dev, _f, _Guarded, _p, _same,
                                        _stream, _within)
from test_reinforce_cpu import (CONFIGS, OBS, UPDATES, _flat, _flat_grads, _load_flat,
                                _trace, fixture_agent, run_loop, update_of)
from pfrl_amd.nn import mfma_trunk as mt

gpu = pytest.mark.gpu

TOL = 1e-5
M_LIST = [1, 63, 64, 65, 257, 2053]
SOFTMAX_A = [1, 2, 9, 31]
GAUSSIAN_A = [1, 3, 32]
BETAS = [0.0, _f(0.01)]
INV_B = _f(1.0 / 3)
C_ENT, C_LP = float(np.float32(1.4189385332046727)), float(np.float32(0.9189385332046727))


# ================================================================== 1. pfrl_reinforce_loss
@functools.lru_cache(maxsize=None)
def _softmax_operands(M, A):
    g = torch.Generator().manual_seed(7919 * M + A)
    return {"z": 2 * torch.randn(M, A, generator=g), "action": torch.randint(0, A, (M,), generator=g),
            "ret": 3 * torch.randn(M, generator=g)}


@functools.lru_cache(maxsize=None)
def _softmax_reference(M, A, beta):
    """float64 + autograd on the reference expression, and the bounds of section 1 (no factor 2)."""
    o = _softmax_operands(M, A)
    z = o["z"].double().requires_grad_(True)
    a, R = o["action"], o["ret"].double()
    dist = Categorical(logits=z)
    lpa, H = dist.log_prob(a), dist.entropy()
    rows = -R * lpa - beta * H
    loss = rows.sum() * INV_B
    (dz,) = torch.autograd.grad(loss, [z])
    z = z.detach()
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
    Hc = H.detach()[:, None]
    E_H = (p * ((eps_p + U) * lp.abs() + E_lp)).sum(1, keepdim=True) + (A - 1) * U * (p * lp.abs()).sum(1, keepdim=True)
    rows = rows.detach()
    E_row = (R.abs() * E_lp[ar, a] + U * (R * lpa.detach()).abs() + beta * E_H[:, 0]
             + U * beta * Hc[:, 0].abs() + U * rows.abs())
    oh = torch.zeros_like(z)
    oh[ar, a] = 1.0
    gl, ge = (INV_B * R).abs()[:, None], beta * INV_B
    E_g = (gl * (p * eps_p + 3 * U * (oh - p).abs())
           + ge * p * ((eps_p + 4 * U) * (lp + Hc).abs() + E_lp + E_H) + U * dz.abs())
    out2 = torch.stack([loss.detach(), H.detach().mean()])
    E_out2 = torch.stack([INV_B * E_row.sum() + U * out2[0].abs(), E_H.mean() + U * out2[1].abs()])
    return {"out2": out2, "dz": dz, "rows": torch.stack([rows, H.detach()], 1),
            "E_out2": E_out2, "E_dz": E_g, "E_rows": torch.stack([E_row, E_H[:, 0]], 1)}


def _emulate_softmax(o, beta):
    """The row arithmetic of k_reinforce_loss in float32 torch on the CPU, loops over the action
    dimension in the kernel's order; the batch sums in float64."""
    z, a, R = o["z"], o["action"], o["ret"]
    M, A = z.shape
    f = torch.float32
    inv_b, beta = torch.tensor(INV_B, dtype=f), torch.tensor(beta, dtype=f)
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
    gl, ge = inv_b * (-R), beta * inv_b
    oh = torch.zeros_like(z)
    oh[torch.arange(M), a] = 1.0
    g = gl[:, None] * (oh - p) + torch.where(p > 0, ge * p * (lp + H[:, None]), torch.zeros_like(p))
    rows = (-R) * lpa - beta * H
    assert g.dtype == f and rows.dtype == f
    out2 = torch.stack([(rows.double().sum() * float(INV_B)).float(), (H.double().sum() / M).float()])
    return {"out2": out2, "dz": g, "rows": torch.stack([rows, H], 1)}


def _run_softmax(dev, o, M, A, beta, inv_b=INV_B):
    nb = _cd(M, 256)
    out = {"dz": _Guarded(M * A, dev), "ws": _Guarded(2 * nb, dev, F64), "out2": _Guarded(2, dev)}
    mt.check(_native.lib().pfrl_reinforce_loss(
        _p(o["z"]), _p(o["action"]), _p(o["ret"]), M, A, inv_b, beta, _p(out["dz"].t), _p(out["ws"].t),
        _p(out["out2"].t), _stream()), "reinforce_loss")
    torch.cuda.synchronize()
    return {k: t.guards(k) for k, t in out.items()}


def _check_softmax(name, tag, got, r, M, A):
    _within(name + " dlogits", tag, got["dz"], r["dz"], 2 * r["E_dz"] + 1e-300)
    _within(name + " out2", tag, got["out2"], r["out2"], 2 * r["E_out2"] + 1e-300)


# ================================================================== 2. pfrl_reinforce_gaussian_loss
@functools.lru_cache(maxsize=None)
def _gaussian_operands(M, A):
    g = torch.Generator().manual_seed(6007 * M + A)
    mean = torch.randn(M, A, generator=g)
    scale = torch.exp(0.3 * torch.randn(A, generator=g))
    return {"mean": mean, "scale": scale, "action": mean + scale * torch.randn(M, A, generator=g),
            "ret": 3 * torch.randn(M, generator=g)}


@functools.lru_cache(maxsize=None)
def _gaussian_reference(M, A, beta):
    o = _gaussian_operands(M, A)
    mean = o["mean"].double().requires_grad_(True)
    scale = o["scale"].double().requires_grad_(True)
    a, R = o["action"].double(), o["ret"].double()
    dist = Independent(Normal(mean, scale.expand_as(mean)), 1)
    lpa, H = dist.log_prob(a), dist.entropy()
    rows = -R * lpa - beta * H
    loss = rows.sum() * INV_B
    dmean, dscale = torch.autograd.grad(loss, [mean, scale])
    mean, s = mean.detach(), scale.detach()
    d = a - mean
    q = d * d / (2 * s * s)
    log_s = s.log()
    t = -q - log_s - C_LP
    E_t = 5 * U * q + 2 * U * log_s.abs() + U * (q + log_s).abs() + U * C_LP + U * t.abs()
    E_lp = E_t.sum(1) + 6 * U * t.abs().sum(1)
    Hd = H.detach()
    E_H = (2 * U * log_s.abs() + U * C_ENT + U * (C_ENT + log_s).abs()).sum() + U * Hd.abs()
    rows = rows.detach()
    E_row = R.abs() * E_lp + U * (R * lpa.detach()).abs() + beta * E_H + U * beta * Hd.abs() + U * rows.abs()
    g = (INV_B * R).abs()[:, None]
    E_dscale = (g * (U * (d * d / s ** 3 - 1 / s).abs() + 3 * U * d * d / s ** 3)).sum(0) + U * dscale.abs()
    out2 = torch.stack([loss.detach(), Hd.mean()])
    E_out2 = torch.stack([INV_B * E_row.sum() + U * out2[0].abs(), E_H.mean() + U * out2[1].abs()])
    return {"out2": out2, "dmean": dmean, "dscale": dscale, "E_out2": E_out2,
            "E_dmean": 5 * U * dmean.abs(), "E_dscale": E_dscale}


def _tree_sum(x):
    """csrc/gaussian_rows.h tree_sum on the last dimension of a float32 tensor."""
    A = x.shape[1]
    W = 1 << (A.bit_length() - 1)
    s = [x[:, t] + x[:, t + W] if t + W < A else x[:, t] for t in range(W)]
    off = 1
    while off < W:
        for i in range(0, W - off, 2 * off):
            s[i] = s[i] + s[i + off]
        off *= 2
    return s[0]


def _emulate_gaussian(o, beta):
    mean, s, a, R = o["mean"], o["scale"], o["action"], o["ret"]
    M, A = mean.shape
    f = torch.float32
    inv_b, beta = torch.tensor(INV_B, dtype=f), torch.tensor(beta, dtype=f)
    c_lp, c_ent = torch.tensor(C_LP, dtype=f), torch.tensor(C_ENT, dtype=f)
    d = a - mean
    log_s = torch.log(s)
    t = (-(d * d) / (2 * (s * s)) - log_s) - c_lp
    lpa = _tree_sum(t)
    H = (c_ent + log_s).double().sum().float()
    g = inv_b * (-R)
    rows = (-R) * lpa - beta * H
    dmean = g[:, None] * (d / (s * s))
    sd = s.double()
    terms = g.double()[:, None] * ((d * d).double() / (sd * sd * sd) - 1.0 / sd)
    dscale = (terms.sum(0) - float(beta) * M * float(INV_B) / sd).float()
    assert dmean.dtype == f and rows.dtype == f
    out2 = torch.stack([(rows.double().sum() * float(INV_B)).float(), H])
    return {"out2": out2, "dmean": dmean, "dscale": dscale}


def _run_gaussian(dev, o, M, A, beta, want_dscale, inv_b=INV_B):
    nb = _cd(M, 256)
    out = {"dmean": _Guarded(M * A, dev), "dscale": _Guarded(A, dev), "ws": _Guarded((2 + A) * nb, dev, F64),
           "out2": _Guarded(2, dev)}
    mt.check(_native.lib().pfrl_reinforce_gaussian_loss(
        _p(o["mean"]), _p(o["scale"]), _p(o["action"]), _p(o["ret"]), M, A, inv_b, beta,
        _p(out["dmean"].t), _p(out["dscale"].t) if want_dscale else None, _p(out["ws"].t),
        _p(out["out2"].t), _stream()), "reinforce_gaussian_loss")
    torch.cuda.synchronize()
    if not want_dscale:
        out.pop("dscale").untouched("dscale")
    return {k: t.guards(k) for k, t in out.items()}


def _check_gaussian(name, tag, got, r):
    _within(name + " dmean", tag, got["dmean"], r["dmean"], 2 * r["E_dmean"] + 1e-300)
    _within(name + " out2", tag, got["out2"], r["out2"], 2 * r["E_out2"] + 1e-300)
    if "dscale" in got:
        _within(name + " dscale", tag, got["dscale"], r["dscale"], 2 * r["E_dscale"] + 1e-300)


# ------------------------------------------------------------------ the bounds, before any GPU relies on them
@pytest.mark.parametrize("A", SOFTMAX_A)
def test_bounds_hold_for_a_float32_emulation_of_the_softmax_rows(A):
    for M in M_LIST:
        for beta in BETAS:
            r = _softmax_reference(M, A, beta)
            got = _emulate_softmax(_softmax_operands(M, A), beta)
            tag = "M%d-A%d-beta%g" % (M, A, beta)
            _check_softmax("emulated reinforce_loss", tag, got, r, M, A)
            _within("emulated reinforce_loss rows", tag, got["rows"], r["rows"], 2 * r["E_rows"] + 1e-300)


@pytest.mark.parametrize("A", GAUSSIAN_A)
def test_bounds_hold_for_a_float32_emulation_of_the_gaussian_rows(A):
    for M in M_LIST:
        for beta in BETAS:
            r = _gaussian_reference(M, A, beta)
            got = _emulate_gaussian(_gaussian_operands(M, A), beta)
            _check_gaussian("emulated reinforce_gaussian_loss", "M%d-A%d-beta%g" % (M, A, beta), got, r)


# ------------------------------------------------------------------ kernels against float64
@gpu
@pytest.mark.parametrize("A", SOFTMAX_A)
@pytest.mark.parametrize("M", M_LIST)
def test_reinforce_loss_matches_float64(M, A):
    dev = _dev()
    o = {k: t.to(dev).contiguous() for k, t in _softmax_operands(M, A).items()}
    nb = _cd(M, 256)
    for beta in BETAS:
        r = _softmax_reference(M, A, beta)
        tag = "M%d-A%d-beta%g" % (M, A, beta)
        got = _run_softmax(dev, o, M, A, beta)
        assert not bool(torch.isnan(got["dz"]).any()) and not bool(torch.isnan(got["out2"]).any())
        _check_softmax("reinforce_loss", tag, got, r, M, A)
        idx = torch.arange(M) // 256
        want = torch.zeros(nb, 2, dtype=F64).index_add_(0, idx, r["rows"])
        E = torch.zeros(nb, 2, dtype=F64).index_add_(0, idx, r["E_rows"])
        _within("reinforce_loss partials", tag, got["ws"].view(nb, 2), want, 2 * E + 1e-300)


@gpu
@pytest.mark.parametrize("A", GAUSSIAN_A)
@pytest.mark.parametrize("M", M_LIST)
def test_reinforce_gaussian_loss_matches_float64(M, A):
    dev = _dev()
    o = {k: t.to(dev).contiguous() for k, t in _gaussian_operands(M, A).items()}
    for beta in BETAS:
        r = _gaussian_reference(M, A, beta)
        for want_dscale in (True, False):
            tag = "M%d-A%d-beta%g-dscale%d" % (M, A, beta, want_dscale)
            got = _run_gaussian(dev, o, M, A, beta, want_dscale)
            assert not any(bool(torch.isnan(t).any()) for t in got.values())
            _check_gaussian("reinforce_gaussian_loss", tag, got, r)


@gpu
def test_ops_wrappers_return_what_the_entry_points_write():
    dev = _dev()
    M, A = 257, 9
    o = {k: t.to(dev) for k, t in _softmax_operands(M, A).items()}
    out2, dz = ops.reinforce_loss(o["z"], o["action"], o["ret"], INV_B, BETAS[1])
    raw = _run_softmax(dev, o, M, A, BETAS[1])
    assert torch.equal(out2, raw["out2"]) and torch.equal(dz.view(-1), raw["dz"]) and dz.shape == (M, A)
    M, A = 257, 3
    o = {k: t.to(dev) for k, t in _gaussian_operands(M, A).items()}
    out2, dmean, dscale = ops.reinforce_gaussian_loss(o["mean"], o["scale"], o["action"], o["ret"], INV_B,
                                                      BETAS[1])
    raw = _run_gaussian(dev, o, M, A, BETAS[1], True)
    assert torch.equal(out2, raw["out2"]) and torch.equal(dmean.view(-1), raw["dmean"])
    assert torch.equal(dscale, raw["dscale"])
    assert ops.reinforce_gaussian_loss(o["mean"], o["scale"], o["action"], o["ret"], INV_B, BETAS[1],
                                       want_dscale=False)[2] is None


# ------------------------------------------------------------------ exact cases
@gpu
def test_zero_returns_without_entropy_term_give_exact_zeros():
    dev = _dev()
    for M, A in ((65, 9), (257, 31)):
        o = {k: t.to(dev).contiguous() for k, t in _softmax_operands(M, A).items()}
        o["ret"] = torch.zeros(M, device=dev)
        got = _run_softmax(dev, o, M, A, 0.0)
        assert float(got["out2"][0]) == 0.0 and bool((got["dz"] == 0).all())
    for M, A in ((65, 3), (257, 32)):
        o = {k: t.to(dev).contiguous() for k, t in _gaussian_operands(M, A).items()}
        o["ret"] = torch.zeros(M, device=dev)
        got = _run_gaussian(dev, o, M, A, 0.0, True)
        assert float(got["out2"][0]) == 0.0
        assert bool((got["dmean"] == 0).all()) and bool((got["dscale"] == 0).all())


@gpu
@pytest.mark.parametrize("A", [1, 2, 4, 8, 16])
def test_uniform_logits_and_integer_returns_give_the_dyadic_gradient(A):
    """p_j = 1 / A exactly (expf(0) = 1, the sum A, one division by a power of two), inv_b = 1 / 4, R an
    integer, beta = 0: dlogits_j = -R (1[j = a] - 1 / A) / 4 holds in float32 without rounding."""
    dev = _dev()
    M = 300
    g = torch.Generator().manual_seed(A)
    o = {"z": torch.full((M, A), 0.5), "action": torch.randint(0, A, (M,), generator=g),
         "ret": torch.randint(-8, 9, (M,), generator=g).float()}
    oh = torch.nn.functional.one_hot(o["action"], A).double()
    want = (0.25 * -o["ret"].double()[:, None] * (oh - 1.0 / A)).float()
    assert torch.equal(want.double(), 0.25 * -o["ret"].double()[:, None] * (oh - 1.0 / A))
    got = _run_softmax(dev, {k: t.to(dev) for k, t in o.items()}, M, A, 0.0, inv_b=0.25)
    _same("reinforce_loss dyadic dlogits", "A%d" % A, got["dz"].view(M, A), want)


@gpu
def test_two_calls_on_the_same_operands_give_the_same_bits():
    dev = _dev()
    M = 2053
    o = {k: t.to(dev).contiguous() for k, t in _softmax_operands(M, 31).items()}
    a, b = _run_softmax(dev, o, M, 31, BETAS[1]), _run_softmax(dev, o, M, 31, BETAS[1])
    assert all(torch.equal(a[k], b[k]) for k in a)
    o = {k: t.to(dev).contiguous() for k, t in _gaussian_operands(M, 32).items()}
    a, b = _run_gaussian(dev, o, M, 32, BETAS[1], True), _run_gaussian(dev, o, M, 32, BETAS[1], True)
    assert all(torch.equal(a[k], b[k]) for k in a)


@gpu
def test_nan_return_reaches_the_loss_and_its_own_row_only():
    dev = _dev()
    M, bad = 257, 70
    for A in (1, 9):
        o = {k: t.to(dev).contiguous() for k, t in _softmax_operands(M, A).items()}
        clean = _run_softmax(dev, o, M, A, BETAS[1])
        o["ret"] = o["ret"].clone()
        o["ret"][bad] = float("nan")
        got = _run_softmax(dev, o, M, A, BETAS[1])
        dz, dz0 = got["dz"].view(M, A), clean["dz"].view(M, A)
        keep = torch.arange(M, device=dev) != bad
        assert bool(torch.isnan(got["out2"][0])) and torch.equal(got["out2"][1], clean["out2"][1])
        assert bool(torch.isnan(dz[bad]).all()) and torch.equal(dz[keep], dz0[keep])
    A = 3
    o = {k: t.to(dev).contiguous() for k, t in _gaussian_operands(M, A).items()}
    clean = _run_gaussian(dev, o, M, A, BETAS[1], True)
    o["ret"] = o["ret"].clone()
    o["ret"][bad] = float("nan")
    got = _run_gaussian(dev, o, M, A, BETAS[1], True)
    dm, dm0 = got["dmean"].view(M, A), clean["dmean"].view(M, A)
    keep = torch.arange(M, device=dev) != bad
    assert bool(torch.isnan(got["out2"][0])) and torch.equal(got["out2"][1], clean["out2"][1])
    assert bool(torch.isnan(dm[bad]).all()) and torch.equal(dm[keep], dm0[keep])
    assert bool(torch.isnan(got["dscale"]).all())       # (every row enters every dscale_j)


@gpu
def test_out_of_range_arguments_are_rejected_before_any_launch():
    dev = _dev()
    L = _native.lib()
    M, A = 8, 4
    o = {k: t.to(dev).contiguous() for k, t in _softmax_operands(M, A).items()}
    dz, ws, out2 = _Guarded(M * 32, dev), _Guarded(64, dev, F64), _Guarded(2, dev)
    a = [_p(o["z"]), _p(o["action"]), _p(o["ret"]), M, A, INV_B, 0.0, _p(dz.t), _p(ws.t), _p(out2.t), _stream()]
    for M_, A_ in ((M, 0), (M, 32), (0, A), (-1, A)):
        b = list(a)
        b[3], b[4] = M_, A_
        assert L.pfrl_reinforce_loss(*b) == PFRL_ERR_ARG
    for i in (0, 1, 2, 7, 8, 9):
        b = list(a)
        b[i] = None
        assert L.pfrl_reinforce_loss(*b) == PFRL_ERR_ARG
    g = {k: t.to(dev).contiguous() for k, t in _gaussian_operands(M, 3).items()}
    ga = [_p(g["mean"]), _p(g["scale"]), _p(g["action"]), _p(g["ret"]), M, 3, INV_B, 0.0, _p(dz.t), None,
          _p(ws.t), _p(out2.t), _stream()]
    for M_, A_ in ((M, 0), (M, 33), (0, 3)):
        b = list(ga)
        b[4], b[5] = M_, A_
        assert L.pfrl_reinforce_gaussian_loss(*b) == PFRL_ERR_ARG
    for i in (0, 1, 2, 3, 8, 10, 11):
        b = list(ga)
        b[i] = None
        assert L.pfrl_reinforce_gaussian_loss(*b) == PFRL_ERR_ARG
    torch.cuda.synchronize()
    for t in (dz, ws, out2):
        t.untouched("an output of a rejected call")


# ================================================================== 3. the agent on the device
@gpu
@pytest.mark.parametrize("prefix", sorted(CONFIGS))
def test_device_route_teacher_forced_on_the_reference_trace(prefix):
    """Every recorded update: the parameters before it loaded, its rows, actions and float32 returns
    pushed through the device route's forward / fused loss / backward, one call per recorded
    ``accumulate_grad`` call; then the agent's own clip and step."""
    g = _trace()
    ag = fixture_agent(g, prefix, gpu=0)
    assert ag.device_route
    dev = ag.device
    grad_tol, param_tol = float(g[prefix + "grad_tol"]), float(g[prefix + "param_tol"])
    params = list(ag.model.parameters())
    for k in range(UPDATES):
        u = update_of(g, prefix, k)
        _load_flat(params, u["params_before"])
        ag.optimizer.zero_grad()
        at = 0
        for n, want in zip(u["call_rows"], u["loss"]):
            rows = torch.from_numpy(u["rows"][at:at + n]).to(dev)
            actions = torch.from_numpy(u["actions"][at:at + n]).to(dev)
            ret = torch.from_numpy(u["returns"][at:at + n].astype(np.float32)).to(dev)
            got = float(ag.loss_and_backward(rows, actions, ret))
            print(prefix, k, "loss", got, float(want))
            assert abs(got - float(want)) <= TOL * max(1.0, abs(float(want))), (prefix, k, got, float(want))
            at += n
        assert ag._split[1] is not None and ag._split[1][0] == CONFIGS[prefix][0]
        grad = _flat_grads(params)
        print(prefix, k, "max gradient difference", np.abs(grad - u["grad"]).max(), "tol", grad_tol)
        np.testing.assert_allclose(grad, u["grad"], rtol=0, atol=grad_tol)
        ag.n_backward = ag.batchsize
        ag.update_with_accumulated_grad()
        after = _flat(params)
        print(prefix, k, "max parameter difference", np.abs(after - u["params_after"]).max(), "tol", param_tol)
        np.testing.assert_allclose(after, u["params_after"], rtol=0, atol=param_tol)


@gpu
@pytest.mark.parametrize("prefix", sorted(CONFIGS))
def test_recomputed_forward_against_retained_graphs_on_the_same_device(prefix):
    """The same state and seeds with ``recompute_forward`` True and False.  Up to the first update the
    two runs hold the same parameters and consume the same draws: the actions are equal bit for bit.
    After it the parameters agree within the fixture's measured ``param_tol``; discrete actions stay
    equal, continuous ones are mean + scale z of parameters that close -- a sum over at most
    (5 + 1) 16 + (16 + 1) paths of sensitivity <= 1 each: 128 param_tol."""
    g = _trace()
    param_tol = float(g[prefix + "param_tol"])
    runs = []
    for recompute in (True, False):
        ag = fixture_agent(g, prefix, gpu=0, recompute_forward=recompute)
        assert ag.device_route == recompute and ag.device.type == "cuda"
        runs.append(run_loop(ag, prefix, updates=3))
    (act_a, after_a), (act_b, after_b) = runs
    first = int(update_of(g, prefix, 0)["call_rows"].sum()) if CONFIGS[prefix][1] == 1 else 20
    assert act_a.shape == act_b.shape
    np.testing.assert_array_equal(act_a[:first], act_b[:first])
    if CONFIGS[prefix][0] == "softmax":
        np.testing.assert_array_equal(act_a, act_b)
    else:
        np.testing.assert_allclose(act_a, act_b, rtol=0, atol=128 * param_tol)
    for k in range(3):
        print(prefix, k, "max parameter difference", np.abs(after_a[k] - after_b[k]).max(), "tol", param_tol)
        np.testing.assert_allclose(after_a[k], after_b[k], rtol=0, atol=param_tol)


@gpu
def test_device_buffers_grow_without_changing_earlier_rows():
    """One episode of 150 steps against an initial capacity of 64: two doublings; every stored row is
    the observation fed at that step and every stored action the one returned."""
    ag = fixture_agent(_trace(), "ga_b1_", gpu=0)
    before = _flat(ag.model.parameters())
    rng = np.random.RandomState(3)
    fed, acted = [], []
    obs = rng.uniform(-1, 1, OBS).astype(np.float32)
    for t in range(150):
        fed.append(obs)
        acted.append(ag.act(obs))
        if t == 63:
            assert ag._rows.shape[0] == 64
            early_rows, early_acts = ag._rows.clone(), ag._acts.clone()
        obs = rng.uniform(-1, 1, OBS).astype(np.float32)
        if t < 149:
            ag.observe(obs, 0.5, False, False)
    assert ag._rows.shape[0] == 256 and ag._acts.shape[0] == 256 and ag._n_rows == 150
    assert torch.equal(ag._rows[:64], early_rows) and torch.equal(ag._acts[:64], early_acts)
    assert np.array_equal(ag._rows[:150].cpu().numpy(), np.stack(fed))
    assert np.array_equal(ag._acts[:150].cpu().numpy(), np.stack(acted))
    ag.observe(obs, 0.5, True, False)
    assert ag._n_rows == 0 and ag.n_backward == 0 and ag.reward_sequences == [[]]
    after = _flat(ag.model.parameters())
    assert np.isfinite(after).all() and not np.array_equal(after, before)


@gpu
def test_save_load_round_trip(tmp_path):
    g = _trace()
    ag = fixture_agent(g, "sm_b1_", gpu=0)
    run_loop(ag, "sm_b1_", updates=2)
    ag.save(str(tmp_path / "agent"))
    assert sorted(os.listdir(str(tmp_path / "agent"))) == ["model.pt", "optimizer.pt"]
    other = fixture_agent(g, "sm_b1_", gpu=0)
    other.load(str(tmp_path / "agent"))
    assert np.array_equal(_flat(other.model.parameters()), _flat(ag.model.parameters()))
    sa, sb = ag.optimizer.state_dict()["state"], other.optimizer.state_dict()["state"]
    assert sa.keys() == sb.keys() and len(sa) > 0
    for i in sa:
        for name in sa[i]:
            assert torch.equal(torch.as_tensor(sa[i][name]).cpu(), torch.as_tensor(sb[i][name]).cpu())
    # the two continue identically from the loaded state
    _, after_a = run_loop(ag, "sm_b1_", updates=1, seed=1)
    _, after_b = run_loop(other, "sm_b1_", updates=1, seed=1)
    assert np.array_equal(after_a[0], after_b[0])
