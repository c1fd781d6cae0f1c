"""pfrl_mlp_wide_fwd / pfrl_mlp_wide_dx (csrc/mlp_wide.hip) through the C ABI against float64.

The project's accuracy rule (tests/test_mlp_fused.py): per output kind, the largest error against float64 over the table
is at most twice that of torch's float32 CPU evaluation.  Row independence bit for bit; there is one tile program."""
import ctypes
import math

import pytest
import torch

from pfrl_amd import _native

pytestmark = pytest.mark.gpu
V, I = ctypes.c_void_p, ctypes.c_int32
ACT = {"tanh": 0, "relu": 1}
GUARD, SENTINEL = 64, 12345.0

# (M, K1, K2, widths, activation, n_nets, col0, ncol)
TABLE = [
    (1, 3, 0, [65, 65, 1], "relu", 1, 0, 3),
    (16, 11, 6, [80, 272, 34], "tanh", 2, 11, 6),
    (17, 64, 0, [256, 256, 64], "relu", 1, 0, 64),
    (33, 65, 0, [400, 300, 1], "relu", 2, 1, 17),
    (33, 376, 17, [256, 256, 1], "relu", 2, 376, 17),
    (17, 11, 6, [512, 512, 34], "tanh", 1, 3, 5),
    (16, 376, 17, [512, 64], "relu", 2, 376, 17),
    (33, 3, 0, [65, 1], "tanh", 1, 0, 1),
    (1, 65, 0, [80, 272, 64], "relu", 2, 64, 1),
]


def guarded(*shape):
    n = math.prod(shape)
    buf = torch.full((n + 2 * GUARD,), SENTINEL, device="cuda")
    buf[GUARD:GUARD + n] = float("nan")
    return buf[GUARD:GUARD + n].view(*shape), buf


def guards_intact(buf):
    return bool((buf[:GUARD] == SENTINEL).all() and (buf[-GUARD:] == SENTINEL).all())


def make_case(seed, M, K1, K2, widths, n_nets):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K1 + K2, generator=g)
    params, dys = [], []
    for _ in range(n_nets):
        fan_in, layers = K1 + K2, []
        for n in widths:
            bound = 1 / math.sqrt(fan_in)
            layers.append(((torch.rand(n, fan_in, generator=g) * 2 - 1) * bound, (torch.rand(n, generator=g) * 2 - 1) * bound))
            fan_in = n
        params.append(layers)
        dys.append(torch.randn(M, widths[-1], generator=g))
    return x, params, dys


def torch_eval(x, params, dys, act, col0, ncol, dtype):
    out = {"y": [], "save": []}
    xs, total = x.to(dtype).clone().requires_grad_(), 0
    for layers, dy in zip(params, dys):
        h = xs
        for l, (w, b) in enumerate(layers):
            h = torch.nn.functional.linear(h, w.to(dtype), b.to(dtype))
            if l + 1 < len(layers):
                h = getattr(torch, act)(h)
                out["save"].append(h.detach())
        out["y"].append(h.detach())
        total = total + (h * dy.to(dtype)).sum()
    total.backward()
    out["dx"] = [xs.grad[:, col0:col0 + ncol]]
    return out


def launch(x, params, dys, K1, act, col0, ncol):
    lib, nn_, L, M = _native.lib(), len(params), len(params[0]), x.shape[0]
    K2 = x.shape[1] - K1
    x1, x2 = x[:, :K1].contiguous().cuda(), (x[:, K1:].contiguous().cuda() if K2 else None)
    pd = [[(w.cuda(), b.cuda()) for w, b in layers] for layers in params]
    W, B, N = (V * (3 * nn_))(), (V * (3 * nn_))(), (I * 3)(*[w.shape[0] for w, _ in params[0]])
    S, Y, DY = (V * (2 * nn_))(), (V * nn_)(), (V * nn_)()
    out, bufs, dyd = {"y": [], "save": [], "dx": []}, [], [dy.cuda() for dy in dys]
    for k in range(nn_):
        for l in range(L):
            W[3 * k + l], B[3 * k + l] = pd[k][l][0].data_ptr(), pd[k][l][1].data_ptr()
            if l + 1 < L:
                t, buf = guarded(M, N[l])
                S[2 * k + l] = t.data_ptr()
                out["save"].append(t), bufs.append(buf)
        t, buf = guarded(M, N[L - 1])
        Y[k], DY[k] = t.data_ptr(), dyd[k].data_ptr()
        out["y"].append(t), bufs.append(buf)
    stream = V(torch.cuda.current_stream().cuda_stream)
    assert lib.pfrl_mlp_wide_fwd(V(x1.data_ptr()), V(x2.data_ptr()) if K2 else None, M, K1, K2, L, nn_, W, B, N, ACT[act],
                                 S, Y, stream) == 0
    t, buf = guarded(M, ncol)
    out["dx"].append(t), bufs.append(buf)
    assert lib.pfrl_mlp_wide_dx(M, K1 + K2, L, nn_, W, N, ACT[act], S, DY, V(t.data_ptr()), col0, ncol, stream) == 0
    torch.cuda.synchronize()
    return {k: [t.cpu() for t in v] for k, v in out.items()}, all(guards_intact(b) for b in bufs)


@pytest.fixture(scope="module")
def table():
    rows = []
    for i, (M, K1, K2, widths, act, nn_, col0, ncol) in enumerate(TABLE):
        x, params, dys = make_case(200 + i, M, K1, K2, widths, nn_)
        rows.append((launch(x, params, dys, K1, act, col0, ncol), torch_eval(x, params, dys, act, col0, ncol, torch.float64),
                     torch_eval(x, params, dys, act, col0, ncol, torch.float32)))
    return rows


@pytest.mark.parametrize("kind", ["y", "save", "dx"])
def test_accuracy_against_float64(table, kind):
    err = lambda got, ref: max((g.double() - r).abs().max().item() for g, r in zip(got, ref))   # noqa: E731
    kernel = torch32 = 0.0
    for (out, ok), ref64, ref32 in table:
        assert ok, "guard zone overwritten"
        assert not any(torch.isnan(t).any() for t in out[kind])
        torch32 = max(torch32, err(ref32[kind], ref64[kind]))
        kernel = max(kernel, err(out[kind], ref64[kind]))
    print("%s: kernel %.3e, torch float32 %.3e" % (kind, kernel, torch32))
    assert kernel <= 2 * torch32


def test_row_and_network_independence_bit_for_bit():
    _, K1, K2, widths, act, _, col0, ncol = TABLE[1]
    x, params, dys = make_case(7, 33, K1, K2, widths, 2)
    both, _ = launch(x, params, dys, K1, act, col0, ncol)
    for k in range(2):
        one, _ = launch(x, params[k:k + 1], dys[k:k + 1], K1, act, col0, ncol)
        assert torch.equal(one["y"][0], both["y"][k])
        assert all(torch.equal(one["save"][l], both["save"][2 * k + l]) for l in range(2))
    for r in (0, 15, 16, 32):
        row, _ = launch(x[r:r + 1].clone(), params, [d[r:r + 1] for d in dys], K1, act, col0, ncol)
        for kind in ("y", "save", "dx"):
            assert all(torch.equal(a[0], b[r]) for a, b in zip(row[kind], both[kind])), (kind, r)


def test_refusals_and_empty_launch_write_nothing():
    lib = _native.lib()
    x = torch.randn(8, 8).cuda()
    ws = [torch.randn(513, 8).cuda(), torch.randn(65, 513).cuda()]
    b, a, dy = torch.randn(513).cuda(), torch.randn(8, 513).cuda(), torch.randn(8, 65).cuda()
    (y, ybuf), (dx, dxbuf) = guarded(8, 65), guarded(8, 65)
    stream = V(torch.cuda.current_stream().cuda_stream)

    def both(only=None, M=8, K=8, nn_=1, n=(80, 4), xp=x.data_ptr(), wp=ws[0].data_ptr(), yp=y.data_ptr(), col0=0, ncol=4):
        W, B, N = (V * 3)(wp, ws[1].data_ptr()), (V * 3)(b.data_ptr(), b.data_ptr()), (I * 3)(*n)
        fwd = lambda: lib.pfrl_mlp_wide_fwd(V(xp), None, M, K, 0, 2, nn_, W, B, N, 1, None, (V * 1)(yp), stream)   # noqa: E731
        dxf = lambda: lib.pfrl_mlp_wide_dx(M, K, 2, nn_, W, N, 1, (V * 2)(a.data_ptr()), (V * 1)(dy.data_ptr()),   # noqa: E731
                                           V(dx.data_ptr()), col0, ncol, stream)
        return fwd() if only == "fwd" else dxf() if only == "dx" else (fwd(), dxf())

    bad = [dict(n=(513, 4)), dict(n=(80, 65)), dict(K=1025), dict(M=0), dict(M=65537), dict(nn_=3), dict(wp=None),
           dict(wp=ws[0].data_ptr() + 2)]
    for kw in bad:
        assert both(**kw) == (-2, -2), kw
    assert both("dx", ncol=65) == -2 and both("dx", col0=5, ncol=4) == -2
    assert both("fwd", xp=None) == -2 and both("fwd", xp=x.data_ptr() + 2) == -2 and both("fwd", yp=y.data_ptr() + 2) == -2
    assert both(nn_=0) == (0, 0)
    torch.cuda.synchronize()
    assert torch.isnan(y).all() and torch.isnan(dx).all() and guards_intact(ybuf) and guards_intact(dxbuf)
    assert both() == (0, 0)
    torch.cuda.synchronize()
    wrote = lambda t: not torch.isnan(t.flatten()[:32]).any() and torch.isnan(t.flatten()[32:]).all()     # noqa: E731
    assert wrote(y) and wrote(dx) and guards_intact(ybuf) and guards_intact(dxbuf)
