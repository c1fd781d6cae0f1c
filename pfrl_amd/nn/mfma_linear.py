"""``nn.Linear`` (+ ReLU) of the MLP agents as gfx950 MFMA kernels at minibatch size.

The MLPs of the replay actor-critic agents (256-256 policy and twin Q of
``examples/mujoco/reproduction/soft_actor_critic/train_soft_actor_critic.py:172-243``, the
400-300 nets of TD3 / DDPG) are evaluated ~26 times per update at B = 100-256
(``pfrl/agents/soft_actor_critic.py:213-330``).  Measured on MI355X inside a captured graph
(``tools/linear_check.py``), the library picks one-workgroup tiles for these shapes: an
``F.linear`` with a 256 x 256 output takes 63-96 us, and so do the 256 x 256 gradients.  The
implicit-GEMM engine of ``csrc/qnet.hip`` runs the same layers (the 1 x 1 case) in 5-7 us with
the bias and ReLU in its epilogue and the ReLU mask folded into both gradient kernels.

``accelerate_mlp(model)`` changes no parameter, name or state_dict key: plain ``nn.Linear``
children become ``_LinearSlot`` (an ``nn.Linear`` subclass around the same tensors) and plain
``nn.Sequential`` containers become ``_MlpSequential`` (same children) so that a ``Linear``
followed by ``nn.ReLU`` is one node.  Inputs outside what the kernels cover (CPU tensors,
other dtypes, batches above ``PFRL_MFMA_LINEAR_MAX_BATCH``) take ``F.linear`` as before.

Numerics: f32 in, f32 accumulate (exact fmaf chains); only the summation order differs from
hipBLASLt's.
"""
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from pfrl_amd import _native
from pfrl_amd._native import check
from pfrl_amd.nn import mfma_trunk as _t
from pfrl_amd.nn.branched import Branched
from pfrl_amd.nn.empirical_normalization import _normalize_with_current
from pfrl_amd.nn.mfma_trunk import _ceil_div, _p, _stream

_ENABLED = os.environ.get("PFRL_MFMA_LINEAR", "1") != "0"
_MAX_BATCH = int(os.environ.get("PFRL_MFMA_LINEAR_MAX_BATCH", "1024"))
# output tiles (16 x 32) from which a layer is launched without split-K
_DIRECT_TILES = int(os.environ.get("PFRL_MFMA_LINEAR_DIRECT_TILES", "96"))
MIN_OUT = 17   # narrower layers are the narrow-head kernels' (mfma_trunk._SmallLinear)


# While a ``slab_sink()`` is open, weight / bias gradients that the backward kernels leave as
# split-K slabs are NOT folded (pfrl_splitk_reduce) and NOT returned: the slabs are recorded as
# {parameter data_ptr: (slabs, stride, n)} for an optimizer that sums them inside its own launch
# (FusedAdam.step(slabs=...), pfrl_adam_step_ex).  The caller owns the contract: ``.grad`` of those
# parameters stays None, so nothing between backward and the step may read it.
_SLAB_SINK = None


class slab_sink:
    def __enter__(self):
        global _SLAB_SINK
        self._prev = _SLAB_SINK
        _SLAB_SINK = self.slabs = {}
        return self.slabs

    def __exit__(self, *exc):
        global _SLAB_SINK
        _SLAB_SINK = self._prev
        return False


def _fold_or_sink(part, stride, splits, w_ptr, b_ptr, dw, db, nW, Fo):
    """Returns (dw, db) after folding the slabs -- or (None, None) with the slabs in the sink."""
    sink = _SLAB_SINK
    if sink is not None and b_ptr is not None:
        sink[w_ptr] = (part, stride, splits)
        sink[b_ptr] = (part[nW:], stride, splits)
        return None, None
    _t._reduce([(part, dw, None, stride, nW, splits, 4, 0),
                (part[nW:], db, None, stride, Fo, splits, 4, 0)])
    return dw, db


def _fwd_splits(M, Fo, K):
    nch = _ceil_div(K, 32)
    tiles16 = _ceil_div(M, 16) * _ceil_div(Fo, 32)
    if tiles16 >= _DIRECT_TILES or Fo % 4 != 0:   # (the fold kernel moves float4 columns)
        return 1
    want = min(max(448 // tiles16, _ceil_div(nch, 16), 1), nch)
    cps = _ceil_div(nch, want)
    return _ceil_div(nch, cps)


def _bwd_kernels_cover(M, K, Fo):
    """Both gradient kernels need a whole number of 32-chunks in their reductions."""
    return K % 32 == 0 and Fo % 32 == 0


class _Linear(torch.autograd.Function):
    """y = act(x w^T + b), act = ReLU or identity, as one autograd node."""

    @staticmethod
    def forward(ctx, x, w, b, relu, splits=None):
        M, K = x.shape
        Fo = w.shape[0]
        x = x.contiguous()
        lib = _native.lib()
        y = torch.empty((M, Fo), dtype=torch.float32, device=x.device)
        splits = _fwd_splits(M, Fo, K) if splits is None else int(splits)
        if splits == 1:
            check(lib.pfrl_linear_fwd(_p(x), _p(w), _p(b), _p(y), M, K, Fo, int(relu), 1, _stream()),
                  "linear_fwd")
        else:
            part = torch.empty((splits, M, Fo), dtype=torch.float32, device=x.device)
            check(lib.pfrl_linear_fwd(_p(x), _p(w), None, _p(part), M, K, Fo, 0, splits, _stream()),
                  "linear_fwd_splitk")
            _t._reduce([(part, y, b, M * Fo, M * Fo, splits, Fo, int(relu))])
        ctx.relu = bool(relu)
        ctx.b_ptr = b.data_ptr() if b is not None else None
        ctx.save_for_backward(x, w, y if relu else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, y = ctx.saved_tensors
        M, K = x.shape
        Fo = w.shape[0]
        need_dx = ctx.needs_input_grad[0]
        dev = x.device
        if (not _bwd_kernels_cover(M, K, Fo) and not ctx.relu and Fo <= 64 and Fo % 16 != 0
                and _ceil_div(M, 16) * 16 * (_ceil_div(Fo, 16) * 16 + 1) * 4 <= 65536
                and ctx.needs_input_grad[1]):
            # the 2 * action_size policy head (Linear(256, 34) of SAC): dx, dw and db from the
            # narrow-head launch (library route below: two products and a column sum)
            dyc = dy.contiguous()
            dx = torch.empty_like(x) if need_dx else None
            dw = torch.empty_like(w)
            db = torch.empty(Fo, dtype=torch.float32, device=dev)
            check(_native.lib().pfrl_linear_small_bwd(_p(dyc), _p(x), _p(w), _p(dx), _p(dw), _p(db), M, K,
                                                      Fo, _stream()), "linear_small_bwd")
            return dx, dw, db, None, None
        if not _bwd_kernels_cover(M, K, Fo):
            # ragged layers (first layer of an MLP, 2 * action_size heads)
            need_w = ctx.needs_input_grad[1]
            dx = dw = db = None
            g = None
            if need_dx or not (need_w and Fo % 16 == 0):
                # library products: their outputs are not the 256 x 256 shapes that the
                # library's heuristics mishandle
                g = torch.ops.aten.threshold_backward(dy, y, 0.0) if ctx.relu else dy
            if need_dx:
                dx = g @ w
            if need_w and Fo % 16 == 0:
                # any in_features: the TAIL weight-gradient kernel, ReLU mask and db folded in
                dyc = dy.contiguous()
                dw = torch.empty_like(w)
                db = torch.empty(Fo, dtype=torch.float32, device=dev)
                splits = _t._wgrad_splits(M, Fo, _ceil_div(K, 32) * 32)
                nW = w.numel()
                stride = nW + Fo
                if splits == 1:
                    pw, pb, st = dw, db, 0
                else:
                    part = torch.empty(splits * stride, dtype=torch.float32, device=dev)
                    pw, pb, st = part, part[nW:], stride
                check(_native.lib().pfrl_linear_bwd_weight(_p(dyc), _p(y), _p(x), _p(pw), _p(pb), st, st,
                                                           M, K, Fo, splits, _stream()),
                      "linear_bwd_weight")
                if splits > 1:
                    dw, db = _fold_or_sink(part, stride, splits, w.data_ptr(), ctx.b_ptr, dw, db, nW, Fo)
            elif need_w:
                dw = g.t() @ x
                db = g.sum(0) if ctx.needs_input_grad[2] else None
            return dx, dw, db, None, None
        dy = dy.contiguous()
        lib = _native.lib()
        if not ctx.needs_input_grad[1]:
            # frozen weights (e.g. the Q-networks under the SAC policy loss): input gradient only
            dx = None
            if need_dx:
                dx = torch.empty_like(x)
                check(lib.pfrl_conv2d_nhwc_bwd_data(_p(dy), _p(y), _p(w), None, _p(dx), M, 1, 1, K, Fo,
                                                    1, 1, 1, 0, 0, _stream()), "linear_bwd_data")
            return dx, None, None, None, None
        dw = torch.empty_like(w)
        db = torch.empty(Fo, dtype=torch.float32, device=dev)
        splits = _t._wgrad_splits(M, Fo, K)
        nW = w.numel()
        stride = nW + Fo
        if splits == 1:
            pw, pb, st = dw, db, 0
        else:
            part = torch.empty(splits * stride, dtype=torch.float32, device=dev)
            pw, pb, st = part, part[nW:], stride
        dx = None
        if need_dx:
            dx = torch.empty_like(x)
            if _t._fused_bwd_ok(M, 1, 1, K, 1):
                check(lib.pfrl_conv2d_nhwc_bwd(_p(dy), _p(y), _p(w), None, _p(x), _p(dx), _p(pw), _p(pb),
                                               st, st, M, 1, 1, K, Fo, 1, 1, 1, 0, 0, splits, _stream()),
                      "linear_bwd")
            else:
                check(lib.pfrl_conv2d_nhwc_bwd_data(_p(dy), _p(y), _p(w), None, _p(dx), M, 1, 1, K, Fo,
                                                    1, 1, 1, 0, 0, _stream()), "linear_bwd_data")
                check(lib.pfrl_conv2d_nhwc_bwd_weight(_p(dy), _p(y), _p(x), _p(pw), _p(pb), st, st, M, 1,
                                                      1, K, Fo, 1, 1, 1, splits, _stream()),
                      "linear_bwd_weight")
        else:
            check(lib.pfrl_conv2d_nhwc_bwd_weight(_p(dy), _p(y), _p(x), _p(pw), _p(pb), st, st, M, 1, 1,
                                                  K, Fo, 1, 1, 1, splits, _stream()),
                  "linear_bwd_weight")
        if splits > 1:
            dw, db = _fold_or_sink(part, stride, splits, w.data_ptr(), ctx.b_ptr, dw, db, nW, Fo)
        return dx, dw, db, None, None


def _reduce_noisy(part, y, mu_b, sigma_b, r_out, n, splits, ncol, relu):
    import ctypes

    V = ctypes.c_void_p
    one = lambda t: (V * 1)(t.data_ptr())    # noqa: E731
    check(_native.lib().pfrl_splitk_reduce_noisy(
        1, one(part), one(y), one(mu_b), one(sigma_b), one(r_out), (ctypes.c_int64 * 1)(n),
        (ctypes.c_int32 * 1)(n), (ctypes.c_int32 * 1)(splits), (ctypes.c_int32 * 1)(ncol),
        (ctypes.c_int32 * 1)(int(relu)), _stream()), "splitk_reduce_noisy")


class _Ctx:
    """What ``_Linear.backward`` reads from its context."""

    def __init__(self, saved, needs, relu):
        self.saved_tensors, self.needs_input_grad, self.relu, self.b_ptr = saved, needs, relu, None


class _NoisyLinear(torch.autograd.Function):
    """``act(x W^T + b)`` of a factorised NoisyNet layer as one node that never writes W in its
    forward pass (pfrl_linear_noisy_fwd: the perturbed weights are formed inside the kernel's
    operand loader; bit-identical to noisy_weights + _Linear).  The no-grad passes of an update
    (target network, Double-DQN action selection, acting) need nothing else; a pass that is
    differentiated builds W once in its BACKWARD (where the launch is off the path the next
    minibatch waits for) and continues as _Linear.backward / pfrl_noisy_weights_bwd do."""

    @staticmethod
    def forward(ctx, x, mu_w, sigma_w, mu_b, sigma_b, r, relu):
        M, K = x.shape
        Fo = mu_w.shape[0]
        x = x.contiguous()
        lib = _native.lib()
        y = torch.empty((M, Fo), dtype=torch.float32, device=x.device)
        splits = noisy_fwd_splits(M, Fo, K)
        if splits == 1:
            check(lib.pfrl_linear_noisy_fwd(_p(x), _p(mu_w), _p(sigma_w), _p(mu_b), _p(sigma_b), _p(r),
                                            _p(y), M, K, Fo, int(relu), 1, _stream()), "linear_noisy_fwd")
        else:
            part = torch.empty((splits, M, Fo), dtype=torch.float32, device=x.device)
            check(lib.pfrl_linear_noisy_fwd(_p(x), _p(mu_w), _p(sigma_w), None, None, _p(r), _p(part), M,
                                            K, Fo, 0, splits, _stream()), "linear_noisy_fwd_splitk")
            _reduce_noisy(part, y, mu_b, sigma_b, r[K:], M * Fo, splits, Fo, relu)
        ctx.relu = bool(relu)
        ctx.save_for_backward(x, mu_w, sigma_w, r, y if relu else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, mu_w, sigma_w, r, y = ctx.saved_tensors
        Fo, K = mu_w.shape
        lib = _native.lib()
        w = torch.empty_like(mu_w)
        check(lib.pfrl_noisy_weights_fwd(_p(mu_w), _p(sigma_w), None, None, _p(r), _p(w), None, Fo, K,
                                         _stream()), "noisy_weights_fwd")
        need_w = any(ctx.needs_input_grad[1:5])
        dx, dw, db, _, _ = _Linear.backward(
            _Ctx((x, w, y), (ctx.needs_input_grad[0], need_w, need_w, False), ctx.relu), dy)
        if not need_w:
            return dx, None, None, None, None, None, None
        dw, db = dw.contiguous(), db.contiguous()
        g_sw, g_sb = torch.empty_like(dw), torch.empty_like(db)
        check(lib.pfrl_noisy_weights_bwd(_p(dw), _p(db), _p(r), _p(g_sw), _p(g_sb), Fo, K, _stream()),
              "noisy_weights_bwd")
        return dx, dw, g_sw, db, g_sb, None, None


class _NoisyLinearPair(torch.autograd.Function):
    """Two NoisyNet layers on the two halves of one activation tensor -- the advantage and value
    streams of the distributional dueling head -- as ONE forward launch reading the halves in place
    (pfrl_linear_noisy_fwd_pair).  Backward: what the two single-layer nodes and the split of ``h``
    do (contiguous halves, _NoisyLinear.backward each, the two input gradients side by side)."""

    @staticmethod
    def forward(ctx, h, mu_w0, sigma_w0, mu_b0, sigma_b0, r0, mu_w1, sigma_w1, mu_b1, sigma_b1, r1):
        import ctypes

        M, K2 = h.shape
        K = K2 // 2
        h = h.contiguous()
        N0, N1 = mu_w0.shape[0], mu_w1.shape[0]
        y0 = torch.empty((M, N0), dtype=torch.float32, device=h.device)
        y1 = torch.empty((M, N1), dtype=torch.float32, device=h.device)
        V = ctypes.c_void_p
        two = lambda a, b: (V * 2)(a, b)                                  # noqa: E731
        check(_native.lib().pfrl_linear_noisy_fwd_pair(
            two(h.data_ptr(), h.data_ptr() + 4 * K), K2, two(_p(mu_w0), _p(mu_w1)),
            two(_p(sigma_w0), _p(sigma_w1)), two(_p(mu_b0), _p(mu_b1)), two(_p(sigma_b0), _p(sigma_b1)),
            two(_p(r0), _p(r1)), two(_p(y0), _p(y1)), M, K, (ctypes.c_int32 * 2)(N0, N1), 0, _stream()),
            "linear_noisy_fwd_pair")
        ctx.save_for_backward(h, mu_w0, sigma_w0, r0, mu_w1, sigma_w1, r1)
        return y0, y1

    @staticmethod
    def backward(ctx, dy0, dy1):
        h, mu_w0, sigma_w0, r0, mu_w1, sigma_w1, r1 = ctx.saved_tensors
        M, K2 = h.shape
        K = K2 // 2
        halves = h.view(M, 2, K).transpose(0, 1).contiguous()
        need = ctx.needs_input_grad
        outs, dxs = [], []
        for x, mu_w, sigma_w, r, dy, ni in ((halves[0], mu_w0, sigma_w0, r0, dy0, 1),
                                            (halves[1], mu_w1, sigma_w1, r1, dy1, 6)):
            if dy is None:
                dy = torch.zeros((M, mu_w.shape[0]), dtype=torch.float32, device=h.device)
            sub = _Ctx((x, mu_w, sigma_w, r, None), (need[0],) + tuple(need[ni:ni + 4]) + (False, False),
                       False)
            g = _NoisyLinear.backward(sub, dy)
            dxs.append(g[0])
            outs.append(g[1:5])
        dh = torch.cat(dxs, dim=1) if need[0] else None
        return (dh,) + tuple(outs[0]) + (None,) + tuple(outs[1]) + (None,)


def noisy_pair_supported(h, a, v):
    """Both streams are factorised-noise layers on the halves of ``h`` and fall into the
    narrow-output tile program of the forward kernel (what pfrl_linear_noisy_fwd_pair covers)."""
    if not (h.is_cuda and h.dim() == 2 and h.shape[1] % 2 == 0 and a.hasbias and v.hasbias):
        return False
    K = h.shape[1] // 2
    ma, mv = a.mu.weight, v.mu.weight
    if ma.shape[1] != K or mv.shape[1] != K or K % 32 != 0:
        return False
    M = h.shape[0]
    narrow = all(w.shape[0] % 32 != 0 and _ceil_div(M, 64) * _ceil_div(w.shape[0], 16) < 512
                 and _fwd_splits(M, w.shape[0], K) == 1 for w in (ma, mv))
    return (narrow and os.environ.get("PFRL_NOISY_PAIR", "1") != "0"
            and noisy_supported(h[:, :K], ma, a.sigma.weight, a.mu.bias, a.sigma.bias)
            and noisy_supported(h[:, :K], mv, v.sigma.weight, v.mu.bias, v.sigma.bias))


def noisy_fwd_splits(M, Fo, K):
    """Split-K of a NoisyNet layer's forward: twice the plain layer's (the loader streams mu AND
    sigma: 25.7 MB for the 3136 x 1024 layer of the Rainbow head, and the launch is bound by how
    many workgroups have loads in flight -- 7 -> 14 splits: Rainbow +4 %, 28: +0.6 % more).  Used by
    both noisy paths (in-loader and materialised), so that they stay bit-identical."""
    s = _fwd_splits(M, Fo, K)
    if s == 1:
        return 1
    if os.environ.get("PFRL_NOISY_SPLITS"):      # (A/B experiments)
        return max(1, min(_ceil_div(K, 32), int(os.environ["PFRL_NOISY_SPLITS"])))
    nch = _ceil_div(K, 32)
    cps = _ceil_div(nch, min(nch, 2 * s))
    return _ceil_div(nch, cps)


def noisy_supported(x, mu_w, sigma_w, mu_b, sigma_b):
    """The in-kernel NoisyNet forward covers minibatch- and acting-sized batches of layers whose
    in_features are a multiple of 32 (PFRL_NOISY_IN_LOADER=0: materialised weights as before)."""
    return (_ENABLED and os.environ.get("PFRL_NOISY_IN_LOADER", "1") != "0" and x.is_cuda
            and x.dim() == 2 and x.dtype == torch.float32 and 0 < x.shape[0] <= _MAX_BATCH
            and mu_b is not None and sigma_b is not None and mu_w.shape[0] >= MIN_OUT
            and mu_w.shape[1] % 32 == 0 and mu_w.is_contiguous() and sigma_w.is_contiguous()
            and mu_w.dtype == torch.float32 and _native.available())


def supported(layer, x):
    return (_ENABLED and x.is_cuda and x.dim() == 2 and x.dtype == torch.float32
            and layer.bias is not None and layer.out_features >= MIN_OUT
            and layer.weight.dtype == torch.float32 and layer.weight.is_contiguous()
            and 0 < x.shape[0] <= _MAX_BATCH and _native.available())


def supported_tensors(x, weight, bias):
    """``supported`` for a weight / bias pair that is not an ``nn.Linear`` (noisy weights)."""
    return (_ENABLED and x.is_cuda and x.dim() == 2 and x.dtype == torch.float32
            and bias is not None and weight.shape[0] >= MIN_OUT and weight.dtype == torch.float32
            and weight.is_contiguous() and 0 < x.shape[0] <= _MAX_BATCH and _native.available())


class _LinearSlot(nn.Linear):
    """An ``nn.Linear`` (same class family, parameter names and state_dict) around the
    tensors of an existing layer; forward takes the MFMA kernels where ``supported``."""

    def __init__(self, linear):
        nn.Module.__init__(self)
        self.__dict__.update({k: v for k, v in linear.__dict__.items()
                              if k not in ("_parameters", "_buffers", "_modules")})
        self._parameters = linear._parameters
        self._buffers = linear._buffers
        self._modules = linear._modules

    def forward(self, x, relu=False):
        if supported(self, x):
            return _Linear.apply(x, self.weight, self.bias, relu)
        y = nn.Linear.forward(self, x)
        return F.relu(y) if relu else y


def _run_children(mods, x):
    """The children ``mods`` one after the other, a ``_LinearSlot`` followed by a plain ``nn.ReLU``
    as one node."""
    i, n = 0, len(mods)
    while i < n:
        m = mods[i]
        if (isinstance(m, _LinearSlot) and i + 1 < n and type(mods[i + 1]) is nn.ReLU
                and torch.is_tensor(x) and supported(m, x)):
            x = m(x, relu=True)
            i += 2
            continue
        x = m(x)
        i += 1
    return x


class _MlpSequential(nn.Sequential):
    """An ``nn.Sequential`` (same children, indices, state_dict) that runs a ``_LinearSlot``
    followed by a plain ``nn.ReLU`` as one node."""

    def forward(self, x):
        from pfrl_amd import ops

        mods = list(self._modules.values())
        # gradients off (acting, target networks): a wide Linear, act, ..., Linear stretch as ONE launch
        run = _find_mlp_run(mods, wide=True) if not torch.is_grad_enabled() and ops.mlp_wide_enabled() else None
        if run is None:
            return _run_children(mods, x)
        s, e, act = run
        x = _run_children(mods[:s], x)
        layers = [(m.weight, m.bias) for m in mods[s:e:2]]
        if not (torch.is_tensor(x) and ops.mlp_wide_supported((x,), [layers], act)):
            return _run_children(mods[s:], x)
        return _run_children(mods[e:], ops.mlp_wide_fwd((x,), [layers], act)[0])


# -------------------------------------------------------------------------------------------------
# Whole small MLPs as one launch (ops.mlp_fused, csrc/mlp.hip): the 64-64 tanh policy and value
# networks of the on-policy continuous-control agents, where every layer is one tile and a launch per
# layer is all launch.
# -------------------------------------------------------------------------------------------------
_MLP_ACTS = {nn.Tanh: "tanh", nn.ReLU: "relu"}
_MLP_LINEARS = (nn.Linear, _LinearSlot, _t._SmallLinearSlot)


def _mlp_linear(m):
    return type(m) in _MLP_LINEARS and m.bias is not None and m.weight.dtype == torch.float32


def _find_mlp_run(mods, wide=False):
    """(start, end, activation) of the first maximal ``Linear, act, ..., Linear`` stretch of ``mods``
    with at least one ``act`` (plain ``nn.Tanh`` / ``nn.ReLU``; ``Linear`` of the plain class or one of
    its slots, float32, with bias) -- or None when there is no such stretch or that stretch is outside
    what one launch covers: 2 or 3 layers, one kind of activation, widths up to 64, up to 512 inputs
    (``ops.mlp_fused``); with ``wide``, instead: a hidden width above 64, none above 512, last width up to
    64, up to 1024 inputs (``ops.mlp_wide_fwd``).  (A lone ``Linear`` is no MLP: it keeps the kernels it
    has.)"""
    from pfrl_amd import ops

    n = len(mods)
    for s in range(n):
        if not _mlp_linear(mods[s]):
            continue
        e = s
        while e + 2 < n and type(mods[e + 1]) in _MLP_ACTS and _mlp_linear(mods[e + 2]):
            e += 2
        if e == s:
            continue
        lins = mods[s:e + 1:2]
        if len({type(m) for m in mods[s + 1:e:2]}) != 1 or len(lins) > ops.MLP_MAX_LAYERS:
            return None
        widths = [m.out_features for m in lins]
        if wide:
            inside = (lins[0].in_features <= ops.MLP_WIDE_MAX_IN and widths[-1] <= ops.MLP_WIDE_MAX_LAST
                      and ops.MLP_MAX_WIDTH < max(widths[:-1]) <= ops.MLP_WIDE_MAX_HIDDEN)
        else:
            inside = lins[0].in_features <= ops.MLP_MAX_IN and max(widths) <= ops.MLP_MAX_WIDTH
        return (s, e + 1, _MLP_ACTS[type(mods[s + 1])]) if inside else None
    return None


def _mlp_route_open(seq):
    """Differentiated calls take the route only where the container was made ``first_order``."""
    return seq._mlp_first_order or not torch.is_grad_enabled()


class _FusedMlpSequential(_MlpSequential):
    """An ``nn.Sequential`` (same children, indices, state_dict; also the head-less views that
    ``agents/_policy_split`` makes of one) whose ``Linear, act, ..., Linear`` stretch is ONE launch
    where ``ops.mlp_fused_supported``; otherwise the children run as in ``_MlpSequential``."""

    _mlp_first_order = True     # (instances carry their own; a copy made through the class starts here)

    def forward(self, x):
        from pfrl_amd import ops

        mods = list(self._modules.values())
        run = _find_mlp_run(mods) if _mlp_route_open(self) else None
        if run is None:
            return _run_children(mods, x)
        s, e, act = run
        x = _run_children(mods[:s], x)
        layers = [(m.weight, m.bias) for m in mods[s:e:2]]
        if not ops.mlp_fused_supported(x, layers, act):
            return _run_children(mods[s:], x)
        return _run_children(mods[e:], ops.mlp_fused(x, layers, act))

    def forward_normalized(self, x, normalizer):
        """``self(normalizer(x, update=False))`` on the RAW observations ``x``: where the stretch starts at
        the first child and ``ops.mlp_fused_supported(..., in_norm=normalizer)``, the launch normalises in
        its loader (same bits); otherwise the normaliser runs in front as torch launches and ``forward``
        follows.  Exactly one of the two, always."""
        from pfrl_amd import ops

        mods = list(self._modules.values())
        run = _find_mlp_run(mods) if _mlp_route_open(self) else None
        if run is not None and run[0] == 0:
            layers = [(m.weight, m.bias) for m in mods[:run[1]:2]]
            if ops.mlp_fused_supported(x, layers, run[2], in_norm=normalizer):
                return _run_children(mods[run[1]:], ops.mlp_fused(x, layers, run[2], in_norm=normalizer))
        return self.forward(_normalize_with_current(normalizer, x))


class _FusedBranched(Branched):
    """A ``Branched`` (same children) of two ``_FusedMlpSequential`` that begin with stretches of
    equal depth: both stretches as ONE launch on the shared input, then what follows in each."""

    def forward(self, *args, **kwargs):
        if len(args) == 1 and not kwargs:
            out = self._both(args[0], None)
            if out is not None:
                return out
        return Branched.forward(self, *args, **kwargs)

    def forward_normalized(self, x, normalizer):
        """``self(normalizer(x, update=False))`` on the RAW observations ``x`` (see
        ``_FusedMlpSequential.forward_normalized``): the one launch of both stretches normalises in its
        loader where it can; otherwise the normaliser runs once in front of ``forward``."""
        out = self._both(x, normalizer)
        return self.forward(_normalize_with_current(normalizer, x)) if out is None else out

    def _both(self, x, norm):
        """Both stretches as one launch on ``x`` (normalised by the launch with ``norm``), or None."""
        from pfrl_amd import ops

        kids = list(self.child_modules)
        if len(kids) == 2 and all(type(k) is _FusedMlpSequential and _mlp_route_open(k) for k in kids):
            mods = [list(k._modules.values()) for k in kids]
            runs = [_find_mlp_run(m) for m in mods]
            if all(r is not None and r[0] == 0 for r in runs) and runs[0][1] == runs[1][1]:
                layers = [[(m.weight, m.bias) for m in ms[:r[1]:2]] for ms, r in zip(mods, runs)]
                acts = (runs[0][2], runs[1][2])
                if ops.mlp_fused_supported(x, layers, acts, in_norm=norm):
                    ys = ops.mlp_fused(x, layers, acts, in_norm=norm)
                    return tuple(_run_children(ms[r[1]:], y) for ms, r, y in zip(mods, runs, ys))
        return None


def _fuse_small_mlps(model, first_order=True):
    """Only the whole-MLP route of :func:`accelerate_mlp`, for agents whose other layers keep the
    kernels they have: every plain ``nn.Sequential`` inside ``model`` with a stretch that
    ``_find_mlp_run`` accepts becomes a ``_FusedMlpSequential``, and a plain ``Branched`` of exactly two
    of them that begin with stretches of equal depth a ``_FusedBranched``.  ``first_order=False``: the
    route is taken under ``torch.no_grad()`` only (a model that is differentiated twice).  Returns
    ``model`` (classes of containers change; children, parameters and state_dict keys do not)."""
    from pfrl_amd import ops

    if model is None or not ops.mlp_fused_enabled():
        return model
    for seq in [m for m in model.modules() if type(m) is nn.Sequential]:
        if _find_mlp_run(list(seq._modules.values())) is not None:
            seq.__class__ = _FusedMlpSequential
            object.__setattr__(seq, "_mlp_first_order", bool(first_order))
    for br in [m for m in model.modules() if type(m) is Branched]:
        kids = list(br.child_modules)
        if len(kids) == 2 and all(type(k) is _FusedMlpSequential for k in kids):
            runs = [_find_mlp_run(list(k._modules.values())) for k in kids]
            if runs[0][0] == 0 and runs[1][0] == 0 and runs[0][1] == runs[1][1]:
                br.__class__ = _FusedBranched
    return model


def accelerate_mlp(model, first_order=True):
    """Route the ``nn.Linear`` layers of ``model`` (plain class, with bias, out_features >= 17)
    through the MFMA kernels and fuse ``Linear, ReLU`` neighbours of plain ``nn.Sequential``
    containers; narrower layers get the narrow-head kernels (``accelerate_heads``).  Before that,
    small MLPs (2 or 3 layers up to 64 wide, all ``nn.Tanh`` or all ``nn.ReLU``) become one launch
    each way (``_fuse_small_mlps``; ``first_order=False``: only with gradients off).  Returns
    ``model`` (modified in place; parameters, names and state_dict keys unchanged)."""
    if model is None:
        return model
    _fuse_small_mlps(model, first_order)
    for parent in list(model.modules()):
        for name, child in list(parent._modules.items()):
            if type(child) is nn.Linear and child.bias is not None and child.out_features >= MIN_OUT:
                parent._modules[name] = _LinearSlot(child)
    for seq in [m for m in model.modules() if type(m) is nn.Sequential]:
        if any(isinstance(c, _LinearSlot) for c in seq._modules.values()):
            seq.__class__ = _MlpSequential
    _t.accelerate_heads(model)
    return model
