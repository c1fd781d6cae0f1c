"""csrc/iqn_embed.hip (``pfrl_iqn_embed_fwd`` / ``pfrl_iqn_embed_bwd``) through the C ABI against plain
float64 torch on the CPU, and the route of ``agents.iqn._quantile_head`` that uses it.

Reference and yardstick are one expression (``_composite``: cos, addmm, relu, product, autograd) in
float64 and in float32, both on the SAME float32 arguments ``taus[..., None] * i_pi``.  Condition, for
each of emb, out, dpsi, dW and db (COVERAGE rows a26 / a39), u = 2^-24:
    max |kernel - ref|  <=  max(4 max |composite - ref|, 8 u max |ref|).
The ReLU kink: ``g`` is zeroed where the float64 pre-activation lies within
64 u (sum_i |W cos| + |b|) of zero; that share must stay under 1e-3.

Shapes (B, N, n, H): M = B N at 1, around one MFMA tile (15 / 16 / 17) and around the 64-row tile
(63 / 64 / 65 / 66, the last with N = 3: batch row 21 straddles two forward tiles); n over the K tail and the
full K; H over the scalar path (1, 3, 67, 130), the 16-byte path (16, 20) and more than one column
block (67, 130); M = 256 / 257 around the dW row split; 341 / 342 row tiles at three column blocks
around the strip-width step of the forward and dpsi launches (341 * 3 / 512 = 1, 342 * 3 / 512 = 2).
"""
import numpy as np
import pytest
import torch

from pfrl_amd import _native, ops
from test_iqn_loss import PFRL_ERR_ARG, U, _Guarded, _p, _stream, _tf_agent, _tf_state, _train
from test_iqn_loss import recorder  # noqa: F401  (the recording proxy in front of the library)

gpu = pytest.mark.gpu
SHAPES = [(1, 1, 1, 1), (5, 3, 3, 3), (16, 1, 16, 16), (17, 1, 63, 20), (21, 3, 64, 67), (1, 64, 64, 16),
          (65, 1, 16, 67), (22, 3, 63, 130), (4, 64, 64, 20), (257, 1, 3, 3), (341, 64, 16, 130), (342, 64, 16, 130)]
FWD, BWD = "pfrl_iqn_embed_fwd", "pfrl_iqn_embed_bwd"


def _composite(arg, psi, W, b, g, N, dtype):
    """(emb, out, dpsi, dW, db) of the statements the launch replaces, in ``dtype``, on f32 arguments."""
    psi, W, b = (t.to(dtype).clone().requires_grad_() for t in (psi, W, b))
    emb = torch.cos(arg.to(dtype))
    out = (psi.unsqueeze(1) * torch.relu(torch.addmm(b, emb, W.t())).reshape(psi.shape[0], N, -1)).reshape(-1, W.shape[0])
    out.backward(g.to(dtype))
    return [t.detach().double() for t in (emb, out, psi.grad, W.grad, b.grad)]


def _case(B, N, n, H):
    gen = torch.Generator().manual_seed(0)
    taus = torch.rand(B, N, generator=gen)
    psi, W, b, g = (torch.randn(s, generator=gen) for s in ((B, H), (H, n), (H,), (B * N, H)))
    i_pi = torch.arange(1, n + 1, dtype=torch.float) * np.pi
    arg = (taus[..., None] * i_pi).reshape(-1, n)                 # f32 product, as the kernel forms it
    cos, W64 = torch.cos(arg.double()), W.double()
    near = (cos @ W64.t() + b.double()).abs() <= 64 * U * (cos.abs() @ W64.abs().t() + b.double().abs())
    assert float(near.float().mean()) < 1e-3
    g = g.masked_fill(near, 0.0)
    return dict(taus=taus, i_pi=i_pi, psi=psi, W=W, b=b, g=g, ref=_composite(arg, psi, W, b, g, N, torch.float64),
                yard=_composite(arg, psi, W, b, g, N, torch.float32))


def _launch(d, shape, dev, want_emb=True, **bad):
    """Both entry points on guarded outputs; ``bad`` overrides a size or NULLs an operand (``w=None``)."""
    B, N, n, H = shape
    k = dict(B=B, N=N, n=n, H=H, **{key: d[key] for key in ("taus", "i_pi", "W", "b", "psi", "g")})
    k.update(bad)
    o = {name: _Guarded(size, dev) for name, size in (("emb", B * N * n), ("out", B * N * H), ("dpsi", B * H),
                                                      ("dW", H * n), ("db", H))}
    floats = (B * N + 255) // 256 * ((H * n + 3) // 4 * 4 + (H + 3) // 4 * 4)
    part = torch.empty(floats, device=dev)
    lib = _native.lib()
    rc = [lib.pfrl_iqn_embed_fwd(_p(k["taus"]), _p(k["i_pi"]), _p(k["W"]), _p(k["b"]), _p(k["psi"]), _p(o["out"].t),
                                 _p(o["emb"].t) if want_emb else None, k["B"], k["N"], k["n"], k["H"], _stream())]
    emb = o["emb"].t if want_emb else torch.cos((d["taus"][..., None] * d["i_pi"]).reshape(-1, n)).contiguous()
    rc.append(lib.pfrl_iqn_embed_bwd(_p(k["g"]), _p(emb), _p(k["W"]), _p(k["b"]), _p(k["psi"]), _p(o["dpsi"].t),
                                     _p(o["dW"].t), _p(o["db"].t), _p(part), floats, k["B"], k["N"], k["n"], k["H"],
                                     _stream()))
    torch.cuda.synchronize()
    return rc, o


def _on(d, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in d.items()}


@gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d-N%d-n%d-H%d" % s)
def test_kernels_against_float64(shape):
    dev = torch.device("cuda")
    c = _case(*shape)
    d = _on(c, dev)
    rc, o = _launch(d, shape, dev)
    rc2, o2 = _launch(d, shape, dev)
    assert rc == rc2 == [0, 0]
    for name, ref, yard in zip(("emb", "out", "dpsi", "dW", "db"), c["ref"], c["yard"]):
        got = o[name].done(name).reshape(ref.shape)
        assert torch.equal(got.view(torch.int32), o2[name].done(name).reshape(ref.shape).view(torch.int32)), name
        err, err_c = float((got.cpu().double() - ref).abs().max()), float((yard - ref).abs().max())
        print("IQN EMBED %s %s: kernel %.3e composite %.3e max|ref| %.3e" % (shape, name, err, err_c, float(ref.abs().max())))
        assert err <= max(4 * err_c, 8 * U * float(ref.abs().max())), (shape, name, err, err_c)


@gpu
def test_gate_edges_are_refused_and_emb_is_optional():
    dev, shape = torch.device("cuda"), (5, 3, 3, 20)
    d = _on(_case(*shape), dev)
    edges = [dict(N=0), dict(N=65), dict(n=0), dict(n=65), dict(H=0), dict(B=0), dict(W=None), dict(psi=None)]
    for bad in edges:
        rc, o = _launch(d, shape, dev, **bad)
        assert rc == [PFRL_ERR_ARG, PFRL_ERR_ARG], bad
        for name in o:
            o[name].untouched("%s of a refused call (%s)" % (name, bad))
    (rc, with_emb), (rc2, without) = _launch(d, shape, dev), _launch(d, shape, dev, want_emb=False)
    assert rc == rc2 == [0, 0]
    without["emb"].untouched("emb = NULL")
    assert torch.equal(with_emb["out"].done(), without["out"].done())


@gpu
def test_autograd_wrapper_hands_back_the_kernels_gradients():
    """... bit for bit at ``g`` and at ``3 g``; the latter is 3 x the former up to the one extra
    rounding per term of sums of at most 66 terms: 66 u < 1e-5 of the largest entry."""
    dev, shape = torch.device("cuda"), (22, 3, 63, 20)
    d = _on(_case(*shape), dev)
    lin = torch.nn.Linear(63, 20).to(dev)
    with torch.no_grad():
        lin.weight.copy_(d["W"]), lin.bias.copy_(d["b"])
    grads = {}
    for scale in (1.0, 3.0):
        _, o = _launch(dict(d, g=d["g"] * scale), shape, dev)
        psi = d["psi"].clone().requires_grad_()
        lin.zero_grad()
        out = ops.iqn_embed(psi, d["taus"], lin)
        assert torch.equal(out.reshape(-1), o["out"].t)
        (out * d["g"]).sum().mul(scale).backward()
        grads[scale] = (psi.grad, lin.weight.grad.clone(), lin.bias.grad.clone())
        for got, name in zip(grads[scale], ("dpsi", "dW", "db")):
            assert torch.equal(got.reshape(-1), o[name].t), (name, scale)
    for one, three in zip(grads[1.0], grads[3.0]):
        assert torch.allclose(three, 3 * one, rtol=0, atol=1e-5 * float(three.abs().max()))


class _Sub(torch.nn.Sequential):
    pass


def _calls_of_one_update(rec, change=None):
    ag = _tf_agent()
    for m in (ag.model, ag.target_model):
        if change is not None:
            m.phi = change(m.phi)
    batch, _, _ = _tf_state(ag, 50)
    del rec.calls[:]
    ag._compute_loss(batch, errors_out=None)[0].backward()
    return rec.calls.count(FWD), rec.calls.count(BWD)


@gpu
def test_one_update_takes_three_forward_launches_and_one_backward(recorder, monkeypatch):  # noqa: F811
    from test_teacher_forced_loss import _check_iqn

    assert _calls_of_one_update(recorder) == (3, 1)
    assert _calls_of_one_update(recorder, lambda phi: _Sub(*phi)) == (0, 0)
    assert _calls_of_one_update(recorder, lambda phi: torch.nn.Sequential(*phi, torch.nn.Identity())) == (0, 0)
    monkeypatch.setenv("PFRL_IQN_EMBED", "0")
    assert _calls_of_one_update(recorder) == (0, 0)
    monkeypatch.delenv("PFRL_IQN_EMBED")
    _check_iqn(-1)                                     # a CPU agent, several updates
    assert recorder.calls.count(FWD) == recorder.calls.count(BWD) == 0


@gpu
def test_training_with_the_launch_equals_the_composite_eager_and_captured(recorder, monkeypatch):  # noqa: F811
    """Equal seeds: equal actions, losses and parameters within 1e-5 (the tolerance of
    tests/test_teacher_forced_loss.py), switch on against off, and captured against eager with the
    kernel seen by the proxy during capture."""
    fused = _train(200, use_graphs=False)
    n_fwd, n_bwd = recorder.calls.count(FWD), recorder.calls.count(BWD)
    assert n_bwd == len(fused["losses"]) > 10 and n_fwd >= 3 * n_bwd
    del recorder.calls[:]
    graph = _train(200)
    assert graph["agent"]._graphed is not None and 1 <= recorder.calls.count(BWD) < n_bwd
    monkeypatch.setenv("PFRL_IQN_EMBED", "0")
    del recorder.calls[:]
    plain = _train(200, use_graphs=False)
    assert recorder.calls.count(FWD) == 0
    for other in (plain, graph):
        np.testing.assert_array_equal(other["actions"], fused["actions"])
        np.testing.assert_allclose(other["losses"], fused["losses"], rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(other["final_params"], fused["final_params"], rtol=1e-5, atol=1e-5)
