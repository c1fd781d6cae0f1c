"""pfrl_mlp_fwd / pfrl_mlp_bwd (csrc/mlp.hip) through the C ABI against float64.

Accuracy follows the project's rule: per output kind, the largest absolute error against float64 over
the whole table is at most twice that of torch's float32 CPU evaluation of the same cases (the
yardstick is torch, never the kernel).  Row independence is checked bit for bit.

Measured on the MI355X (kernel / torch float32): y 2.1e-7 / 2.0e-7, save 8.8e-7 / 7.5e-7, dx 2.8e-7 / 3.8e-7, dW0
2.2e-6 / 3.1e-5, dW1 2.6e-6 / 3.9e-5, dW2 3.4e-6 / 3.3e-6, db0 2.0e-6 / 3.1e-6, db1 3.0e-6 / 7.6e-6, db2 1.1e-6 / 1.9e-6."""
import ctypes
import math

import pytest
import torch

from pfrl_amd import _native

pytestmark = pytest.mark.gpu
V, I = ctypes.c_void_p, ctypes.c_int32
ACT = {"tanh": 0, "relu": 1}
GUARD, SENTINEL = 64, 12345.0
BOTH = (0, 65536)          # small_m: every M on the 64-row program / on the 16-row program

# (M, in_features, [(widths, activation) per network], dx wanted)
TABLE = [
    (1, 1, [([1], "tanh")], True),
    (15, 3, [([16, 6], "relu")], False),
    (16, 4, [([17, 64, 32], "tanh")], True),
    (17, 5, [([64, 64, 1], "tanh"), ([1, 17, 6], "relu")], False),
    (63, 31, [([64, 1], "tanh")], True),
    (64, 32, [([16, 16, 64], "relu")], False),
    ("slabs", 33, [([64, 64, 6], "tanh"), ([64, 17, 1], "tanh")], True),   # smallest M with two slabs
    (130, 376, [([64, 64, 6], "tanh"), ([64, 64, 1], "tanh")], False),
    ("tiles", 4, [([17, 6], "relu"), ([16, 1], "tanh")], True),   # smallest M with two tiles a workgroup
]


def resolve_m(m):
    slabs = _native.lib().pfrl_mlp_bwd_slabs
    if m == "slabs":
        return next(v for v in range(1, 65537) if slabs(v) > 1)
    if m == "tiles":
        return next(v for v in range(1, 65537) if slabs(v) < -(-v // 64))
    return m


def guarded(*shape):
    """A NaN-filled device tensor of ``shape`` inside sentinel zones; returns (view, whole buffer)."""
    n = math.prod(shape)
    buf = torch.full((n + 2 * GUARD,), SENTINEL, device="cuda")
    buf[GUARD:GUARD + n] = float("nan")
    return buf[GUARD:GUARD + n].view(*shape), buf


def guards_intact(buf):
    return bool((buf[:GUARD] == SENTINEL).all() and (buf[-GUARD:] == SENTINEL).all())


def pad4(n):
    return (n + 3) & ~3


def make_case(seed, M, K0, nets):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K0, generator=g)
    params, dys = [], []
    for widths, _ in nets:
        fan_in, layers = K0, []
        for n in widths:
            bound = 1 / math.sqrt(fan_in)
            layers.append(((torch.rand(n, fan_in, generator=g) * 2 - 1) * bound,
                           (torch.rand(n, generator=g) * 2 - 1) * bound))
            fan_in = n
        params.append(layers)
        dys.append(torch.randn(M, widths[-1], generator=g))
    return x, params, dys


def torch_eval(x, params, dys, nets, dtype):
    """{kind: [tensors]} of the plain torch evaluation in ``dtype`` on the CPU."""
    out = {}
    for layers, dy, (_, act) in zip(params, dys, nets):
        leaf = lambda t: t.to(dtype).clone().requires_grad_()      # noqa: E731
        xs, ps = leaf(x), [(leaf(w), leaf(b)) for w, b in layers]
        h = xs
        for l, (w, b) in enumerate(ps):
            h = torch.nn.functional.linear(h, w, b)
            if l + 1 < len(ps):
                h = getattr(torch, act)(h)
                out.setdefault("save", []).append(h.detach())
        h.backward(dy.to(dtype))
        out.setdefault("y", []).append(h.detach())
        out.setdefault("dx", []).append(xs.grad)
        for l, (w, b) in enumerate(ps):
            out.setdefault("dW%d" % l, []).append(w.grad)
            out.setdefault("db%d" % l, []).append(b.grad)
    return out


def launch(x, params, dys, nets, small_m, want_dx=True, fwd_only=False):
    """Both launches on guarded outputs -> ({kind: [tensors]}, all guard zones intact)."""
    lib, nn_, L, (M, K0) = _native.lib(), len(nets), len(nets[0][0]), x.shape
    xd = x.cuda()
    pd = [[(w.cuda(), b.cuda()) for w, b in layers] for layers in params]
    W, B, N = (V * (3 * nn_))(), (V * (3 * nn_))(), (I * (3 * nn_))()
    S, Y, A = (V * (2 * nn_))(), (V * nn_)(), (I * nn_)(*[ACT[a] for _, a in nets])
    out, bufs = {"y": [], "save": [], "dx": []}, []
    for k, (widths, _) in enumerate(nets):
        for l, n in enumerate(widths):
            W[3 * k + l], B[3 * k + l], N[3 * k + l] = pd[k][l][0].data_ptr(), pd[k][l][1].data_ptr(), n
            if l + 1 < L:
                t, buf = guarded(M, n)
                S[2 * k + l] = t.data_ptr()
                out["save"].append(t), bufs.append(buf)
        t, buf = guarded(M, widths[-1])
        Y[k] = t.data_ptr()
        out["y"].append(t), bufs.append(buf)
    stream = V(torch.cuda.current_stream().cuda_stream)
    assert lib.pfrl_mlp_fwd(V(xd.data_ptr()), M, K0, L, nn_, W, B, N, A, S, Y, small_m, stream) == 0
    if not fwd_only:
        slabs = lib.pfrl_mlp_bwd_slabs(M)
        sizes = [sum(pad4(w.numel()) + pad4(b.numel()) for w, b in layers) for layers in params]
        stride = max(sizes)
        DY, DX, G, WS = (V * nn_)(), (V * nn_)(), (V * nn_)(), (V * nn_)()
        dyd = [dy.cuda() for dy in dys]
        parts = []
        for k in range(nn_):
            DY[k] = dyd[k].data_ptr()
            if want_dx:
                t, buf = guarded(M, K0)
                DX[k] = t.data_ptr()
                out["dx"].append(t), bufs.append(buf)
            t, buf = guarded(sizes[k])
            G[k] = t.data_ptr()
            parts.append(t), bufs.append(buf)
            if slabs > 1:
                t, buf = guarded(slabs * stride)
                WS[k] = t.data_ptr()
                bufs.append(buf)
        assert lib.pfrl_mlp_bwd(V(xd.data_ptr()), M, K0, L, nn_, W, N, A, S, DY, DX if want_dx else None, G, WS, stride,
                                stream) == 0
        for k, layers in enumerate(params):
            flat, off = parts[k], 0
            for l, (w, b) in enumerate(layers):
                out.setdefault("dW%d" % l, []).append(flat[off:off + w.numel()].view_as(w))
                off += pad4(w.numel())
                out.setdefault("db%d" % l, []).append(flat[off:off + b.numel()])
                off += pad4(b.numel())
    torch.cuda.synchronize()
    return {k: [t.cpu() for t in v] for k, v in out.items()}, all(guards_intact(b) for b in bufs)


@pytest.fixture(scope="module")
def table():
    """Every case once: the kernel's outputs on both tile programs, float64 and float32 torch."""
    rows = []
    for i, (m, K0, nets, want_dx) in enumerate(TABLE):
        M = resolve_m(m)
        x, params, dys = make_case(100 + i, M, K0, nets)
        runs = [launch(x, params, dys, nets, small_m, want_dx) for small_m in BOTH]
        rows.append((runs, torch_eval(x, params, dys, nets, torch.float64),
                     torch_eval(x, params, dys, nets, torch.float32)))
    return rows


@pytest.mark.parametrize("i", range(len(TABLE)))
def test_guards_and_tile_programs(table, i):
    (a, a_ok), (b, b_ok) = table[i][0]
    assert a_ok and b_ok, "guard zone overwritten"
    for kind in a:
        for u, v in zip(a[kind], b[kind]):
            assert not torch.isnan(u).any(), kind
            if kind in ("y", "save"):        # the forward has two programs; the backward one
                assert torch.equal(u, v), kind


@pytest.mark.parametrize("kind", ["y", "save", "dx", "dW0", "dW1", "dW2", "db0", "db1", "db2"])
def test_accuracy_against_float64(table, kind):
    err = lambda got, ref: max((g.double() - r).abs().max().item() for g, r in zip(got, ref))   # noqa: E731
    kernel = torch32 = 0.0
    for runs, ref64, ref32 in table:
        if not runs[0][0].get(kind):
            continue
        torch32 = max(torch32, err(ref32[kind], ref64[kind]))
        for out, _ in runs:
            kernel = max(kernel, err(out[kind], ref64[kind]))
    print("%s: kernel %.3e, torch float32 %.3e" % (kind, kernel, torch32))
    assert kernel <= 2 * torch32


def test_row_independence_bit_for_bit():
    nets = [([64, 64, 6], "tanh"), ([64, 17, 1], "relu")]
    x, params, dys = make_case(7, 130, 11, nets)
    rows = [0, 16, 64, 129]
    base, _ = launch(x, params[:1], dys[:1], nets[:1], BOTH[0], fwd_only=True)
    others = [launch(x, params[:1], dys[:1], nets[:1], BOTH[1], fwd_only=True)[0],
              launch(x, params, dys, nets, -1, fwd_only=True)[0]]
    for o in others:
        assert torch.equal(o["y"][0], base["y"][0]) and torch.equal(o["save"][1], base["save"][1])
    for r in rows:
        for small_m in BOTH:
            one, _ = launch(x[r:r + 1].clone(), params[:1], [dys[0][r:r + 1]], nets[:1], small_m, fwd_only=True)
            assert torch.equal(one["y"][0][0], base["y"][0][r])
            assert torch.equal(one["save"][0][0], base["save"][0][r])


def test_refusals_and_empty_launch_write_nothing():
    lib = _native.lib()
    x, (w, b) = torch.randn(8, 4).cuda(), (torch.randn(3, 4).cuda(), torch.randn(3).cuda())
    big = torch.randn(65, 4).cuda()
    (y, ybuf), (g, gbuf), dy = guarded(8, 3), guarded(16), torch.randn(8, 3).cuda()
    one = lambda t: (V * 3)(t.data_ptr())      # noqa: E731
    stream = V(torch.cuda.current_stream().cuda_stream)

    def both(M=8, K0=4, L=1, nn_=1, xp=x.data_ptr(), wp=w.data_ptr(), n=3, act=0, yp=y.data_ptr()):
        W, N, A = (V * 3)(wp), (I * 3)(n), (I * 1)(act)
        return (lib.pfrl_mlp_fwd(V(xp), M, K0, L, nn_, W, one(b), N, A, None, (V * 1)(yp), -1, stream),
                lib.pfrl_mlp_bwd(V(xp), M, K0, L, nn_, W, N, A, None, one(dy), None, (V * 1)(g.data_ptr()), None, 16,
                                 stream))

    bad = [dict(M=0), dict(M=65537), dict(K0=0), dict(K0=513), dict(L=0), dict(L=4), dict(nn_=3), dict(n=0),
           dict(n=65, wp=big.data_ptr()), dict(act=2), dict(xp=None), dict(wp=None), dict(xp=x.data_ptr() + 2)]
    for kw in bad:
        assert both(**kw) == (-2, -2), kw
    assert lib.pfrl_mlp_fwd(V(x.data_ptr()), 8, 4, 1, 1, one(w), one(b), (I * 3)(3), (I * 1)(0), None,
                            (V * 1)(y.data_ptr() + 2), -1, stream) == -2
    assert both(nn_=0) == (0, 0)
    torch.cuda.synchronize()
    assert torch.isnan(y).all() and torch.isnan(g).all() and guards_intact(ybuf) and guards_intact(gbuf)
    assert both() == (0, 0)
    torch.cuda.synchronize()
    assert not torch.isnan(y).any() and not torch.isnan(g).any() and guards_intact(ybuf) and guards_intact(gbuf)
