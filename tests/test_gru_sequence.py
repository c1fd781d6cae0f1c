"""pfrl_gru_seq_fwd / pfrl_gru_seq_bwd (csrc/gru_seq.hip) against the step formulas in float64 with autograd, as a loop over the
time steps of the packed rows.  Yardstick per case and quantity: the maximum error of the same loop in float32 on the CPU; the
kernels may err twice as much (+ 1e-7 where gates saturate and the yardstick can be exactly 0).  The objective weights Y and hn
with fixed random numbers, so dhn is not zero.  Every output sits between NaN guard rows.  Measured on the MI355X (pytest -s
prints every figure): worst kernel / yardstick ratio per quantity in COVERAGE a38."""
import ctypes
import functools

import pytest
import torch

from pfrl_amd import _native, ops

pytestmark = pytest.mark.gpu
CASES = {   # id: (batch_sizes, H[, h0 given, dhn given, b_hn given, scale of P])
    "T1-one-row": ([1], 1), "equal-lengths-unit-tail-scalar-loads": ([3, 3, 3], 5),
    "sequences-end-at-three-steps": ([5, 3, 3, 1], 4), "M-tile-edge-vector-loads": ([17, 16, 1], 20),
    "row-block-edge": ([65, 64, 2], 16), "envelope-edge-scalar-loads": ([256, 1], 3), "recurrent-PPO-shape": ([4] * 10, 16),
    "example-width": ([8] * 3, 512), "no-initial-state": ([17, 16, 1], 20, False), "no-final-state-gradient": ([5, 3, 3, 1], 4, True, False),
    "no-b_hn": ([5, 3, 3, 1], 4, True, True, False), "saturated": ([4] * 10, 16, True, True, True, 20)}


def _loop(dtype, sizes, P, h0, W, b_hn, dy, dhn):     # the formulas and their gradients in ``dtype`` on the CPU
    P, W, H = P.to(dtype).requires_grad_(), W.to(dtype), W.shape[1]
    h0 = None if h0 is None else h0.to(dtype).requires_grad_()
    h = P.new_zeros(sizes[0], H) if h0 is None else h0
    off, ys, hend, saved, pre = 0, [], [], [], []
    for t, n in enumerate(sizes):
        s, p = h[:n] @ W.T, P[off:off + n]                # d objective / d s is dQ
        s = s if s.requires_grad else s.requires_grad_()  # (zeros W^T at step 0 without h0)
        r, z = torch.sigmoid(p[:, :H] + s[:, :H]), torch.sigmoid(p[:, H:2 * H] + s[:, H:2 * H])
        q = s[:, 2 * H:] + (0 if b_hn is None else b_hn.to(dtype))
        c = torch.tanh(p[:, 2 * H:] + r * q)
        h = (1 - z) * c + z * h[:n]
        nxt = sizes[t + 1] if t + 1 < len(sizes) else 0   # rows nxt .. n end here: the highest rows end first
        ys, hend, saved, pre, off = ys + [h], [h[nxt:]] + hend, saved + [torch.cat([r, z, c, q], 1)], pre + [s], off + n
    out = dict(zip(("Y", "hn", "saved"), (torch.cat(v) for v in (ys, hend, saved))))
    obj = (out["Y"] * dy.to(dtype)).sum() + (0 if dhn is None else (out["hn"] * dhn.to(dtype)).sum())
    grads = torch.autograd.grad(obj, pre + [P] + ([] if h0 is None else [h0]))
    out.update(zip(("dP", "dh0"), grads[len(pre):]), dQ=torch.cat(grads[:len(pre)]))
    return {k: v.detach().double() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def _case(name):    # inputs (f32, CPU), the float64 results, the yardstick's maximum errors
    sizes, H, state, final, bias, scale = CASES[name] + (True, True, True, 1)[len(CASES[name]) - 2:]
    g = torch.Generator().manual_seed(sorted(CASES).index(name))
    R, n0 = sum(sizes), sizes[0]
    W = (torch.rand((3 * H, H), generator=g) * 2 - 1) / H ** 0.5
    P, h0, b_hn, dy, dhn = (torch.randn(s, generator=g) for s in ((R, 3 * H), (n0, H), (H,), (R, H), (n0, H)))
    inputs = (sizes, P * scale, h0 if state else None, W, b_hn / H ** 0.5 if bias else None, dy, dhn if final else None)
    want, f32 = _loop(torch.float64, *inputs), _loop(torch.float32, *inputs)
    return inputs, want, {k: float((f32[k] - want[k]).abs().max()) for k in want}


def _guarded(rows, width):      # a [rows, width] view between two NaN guard rows
    buf = torch.full((rows + 2, width), float("nan"), device="cuda")
    return buf, buf[1:rows + 1]


def _run(sizes, P, h0, W, b_hn, dy, dhn, p_null=False):     # both entries on guarded buffers -> return codes, the buffers
    (R, G), n0 = P.shape, sizes[0] if h0 is None else h0.shape[0]
    dev = [None if t is None else t.cuda() for t in (P, h0, W, b_hn, dy, dhn)]
    P, h0, W, b_hn, dy, dhn = [None if t is None else t.data_ptr() for t in dev]
    H = G // 3
    shapes = dict(Y=(R, H), saved=(R, 4 * H), hn=(n0, H), dP=(R, G), dQ=(R, G), carry=(n0, H))
    if h0 is not None:
        shapes["dh0"] = (n0, H)
    bufs = {k: _guarded(*s) for k, s in shapes.items()}
    b = {k: v[1].data_ptr() for k, v in bufs.items()}
    bs, lib = (ctypes.c_int32 * max(len(sizes), 1))(*sizes), _native.lib()
    rc = [lib.pfrl_gru_seq_fwd(None if p_null else P, h0, W, b_hn, b["Y"], b["saved"], b["hn"], bs, len(sizes), H, ops._stream())]
    rc.append(lib.pfrl_gru_seq_bwd(dy, dhn, W, None if p_null else b["saved"], b["Y"], h0, b["dP"], b["dQ"], b.get("dh0"), b["carry"],
                                   bs, len(sizes), H, ops._stream()))
    return rc, bufs


@pytest.mark.parametrize("name", CASES)
def test_kernels_against_float64_twice_and_guarded(name):
    inputs, want, yard = _case(name)
    (rc, bufs), (_, again) = _run(*inputs), _run(*inputs)
    assert rc == [0, 0]
    for k, (buf, view) in bufs.items():
        assert torch.equal(view, again[k][1]), "two runs differ in " + k
        assert bool(torch.isnan(buf[0]).all() and torch.isnan(buf[-1]).all()) and not bool(torch.isnan(view).any()), k
    for k in want:
        err = float((bufs[k][1].cpu().double() - want[k]).abs().max())
        print("GRU sequence %s %s f32_loop_max_err %.3e kernel_max_err %.3e" % (name, k, yard[k], err))
        assert err <= 2 * yard[k] + (1e-7 if name == "saturated" else 0), (name, k, err, yard[k])


@pytest.mark.parametrize("sizes,p_null", [([], False), ([2, 3], False), ([2, 0], False), ([257], False), ([2, 1], True)],
                         ids=["T=0", "increasing", "zero-size", "257-rows", "NULL-p-and-saved"])
def test_refusals_launch_nothing(sizes, p_null):
    R, t = max(sum(sizes), 1), torch.zeros
    rc, bufs = _run(sizes, t(R, 12), t(max(sizes + [1]), 4), t(12, 4), None, t(R, 4), None, p_null)
    assert rc[0] != 0 and rc[1] != 0 and all(bool(torch.isnan(buf).all()) for buf, _ in bufs.values())
    assert p_null or not ops.gru_sequence_supported(sizes, 4, 4)
