"""csrc/qnet.hip -- the f32 MFMA convolution kernels -- over the whole geometry envelope that
``mfma_trunk._conv_ok`` / ``plan_for`` admit, against ``torch.nn.functional.conv2d`` in FLOAT64 on
the CPU (autograd for the gradients), through the C ABI and the ``mt.*`` helpers.

Two checks per kernel result:

(a) exact.  Operands are small integers stored as f32 (x, w, b, dy in -3..3; a_prev and dy_mask in
    -2..2 and forced to hold both 0.0 and -0.0).  The test asserts the premise -- the reference
    evaluated on the ABSOLUTE operands stays below 2^24, so every partial sum in any order is an
    integer that f32 holds exactly -- and then the kernel output must be ``torch.equal`` to the f64
    reference cast to f32: no tolerance, whatever the tile program, split count or fold.

(b) rounded.  Operands are randn.  Per element |out - ref64| <= 2 (n + 2) 2^-24 ref64_abs, where
    ref64_abs is the same reference on absolute operands (plus |b|) and n the number of summed
    terms of that output: (n + 2) 2^-24 sum|terms| is the textbook forward-error bound of an f32
    dot product in any order, the factor 2 is margin for the two-accumulator interleave and the
    slab fold.  Each test prints the largest err / bound it saw (``RATIO <kernel> <value>``).

Every output buffer, split-K / weight-gradient slabs included, is carved out of a NaN-filled
allocation with 4096 guard floats on either side; after the launch the guards must still be all
NaN and the payload must hold none.

Whole trunks (several layers, section "trunks" below): the integer operands are sparse (-1, 0, 1)
so that the premise of (a) still holds after five layers; the bound of (b) is the first-order
composition of the per-layer bounds, 2 * 2^-24 * sum over the layers of (fan-in + 2) against the
f64 reference on absolute operands, and is applied to the FORWARD pass only (ReLU is 1-Lipschitz,
so the composition is rigorous).  For a gradient it is not: a pre-activation of the reference
within rounding distance of zero flips a ReLU mask, which moves the gradient by a whole term, and
with randn operands some of the 10^5 pre-activations always lie inside any bound that can be
proven.  The gradient kernels get check (b) layer by layer instead: the layer geometries of these
trunks are part of the kernel matrix above.
"""
import copy
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from pfrl_amd.nn import mfma_trunk as mt

gpu = pytest.mark.gpu

GUARD = 4096
U = 2.0 ** -24
PFRL_ERR_ARG = -2

# (C, Cout, R, S, stride, H, W)
FIRST = [
    (4, 48, 8, 8, 3, 42, 37),      # Cout = 48, stride 3, 1 leftover input row and 2 columns
    (8, 32, 6, 4, 2, 30, 21),      # non-square kernel and image, leftover column
    (12, 16, 3, 8, 1, 7, 12),      # C = 12, OH * OW = 25: pix_mode 0
    (4, 32, 8, 8, 2, 64, 64),      # OH * OW = 841: pix_mode 0 on the large side
    (16, 80, 2, 2, 2, 10, 6),      # Cout = 80, kernel == stride
    (4, 32, 8, 8, 4, 84, 88),      # OH * OW = 420, one step past Nature's 400
    (32, 32, 1, 1, 1, 8, 4),       # OH * OW = 32 and 31: the lower border of pix_mode 2 ...
    (32, 32, 1, 1, 1, 31, 1),
    (128, 32, 1, 1, 1, 8, 4),      # ... and the same border with K = 128, where the 32 x 128
    (128, 32, 1, 1, 1, 31, 1),     # program (the one that reads pix_mode) is eligible
    (4, 48, 8, 8, 4, 44, 36),      # the first layers of the trunks below
    (4, 32, 8, 8, 4, 44, 36),
]
UPPER = [
    (16, 32, 2, 2, 2, 12, 8),      # C = 16, one tap
    (48, 64, 4, 2, 2, 10, 14),     # C = 48, TH = 2, TW = 1
    (32, 96, 6, 3, 3, 12, 9),      # stride 3
    (64, 64, 3, 3, 1, 7, 5),       # stride 1, non-square map, dgrad reduction of 18 chunks
    (32, 64, 8, 8, 4, 24, 16),     # stride 4: merge and pos-class programs eligible
    (128, 32, 1, 1, 1, 3, 5),      # 1x1 convolution on a map (not the linear special case)
    (32, 64, 4, 2, 2, 10, 8),      # the upper layers of the trunks below
    (64, 32, 3, 3, 1, 4, 4),
    (48, 32, 4, 2, 2, 10, 8),
    (32, 64, 4, 4, 2, 10, 8),
]
BATCHES = [1, 5, 67]               # 67: ragged against 16-, 32-, 64- and 128-row tiles


def _gid(g):
    return "C%d-Co%d-k%dx%d-s%d-%dx%d" % g


# ------------------------------------------------------------------ eligibility (the rules of
# fwd_program / dgrad_program / pfrl_conv2d_nhwc_bwd_weight for a FORCED program id)
# These three are COPIES of the C rules in csrc/qnet.hip and must be kept in step with them by
# hand: the C functions fall back to their default program, silently, when a forced id is not
# eligible, so if a copy here admitted more than the C rule the forced test would run the default
# program and the coverage assertion below would still hold.  Nothing detects that drift.
def fwd_programs(geom):
    C, Co, R, S, ST, H, W = geom
    if Co % 32:
        return [0, 1]
    return [p for p in range(2, 9) if p not in (2, 7) or Co % 64 == 0]


def dgrad_programs(geom):
    C, Co, R, S, ST, H, W = geom
    if C % 32:
        return [5]                 # (the only program of 16-wide channel blocks: chosen, not forced)
    z, taps = ST * ST, (R // ST) * (S // ST)
    progs = [p for p in range(0, 5) if p != 0 or C % 64 == 0]
    merge64 = ST > 1 and 64 % C == 0 and (z * C) % 64 == 0
    if merge64:
        progs += [6, 9]
    if ST > 1 and 128 % C == 0 and (z * C) % 128 == 0:
        progs.append(7)
    if ST == 1 and taps > 1 and C % 64 == 0:
        progs.append(8)
    return progs


def wgrad_programs(geom):
    C, Co, R, S, ST, H, W = geom
    if Co % 32:
        return [1]
    K = R * S * C
    tiles = {0: (32, 32), 2: (64, 64), 3: (64, 128), 4: (32, 128), 5: (32, 256)}
    return [p for p, (bi, bj) in tiles.items() if Co % bi == 0 and K % bj == 0]


def test_every_tile_program_is_reached_by_some_geometry():
    """The table behind test_every_eligible_tile_program_matches_the_reference: over the whole
    matrix every id of the three switch statements is forced (or, for dgrad 5, chosen) at least
    once.  (No GPU: the bookkeeping is by the ids the tests request and the rule they apply.)"""
    fwd, dg, wg = set(), set(), set()
    for g in FIRST + UPPER:
        fwd |= set(fwd_programs(g))
        wg |= set(wgrad_programs(g))
    for g in UPPER:
        dg |= set(dgrad_programs(g))
    assert fwd == set(range(9)) and dg == set(range(10)) and wg == set(range(6)), (fwd, dg, wg)


# ------------------------------------------------------------------ operands and reference
def _with_zeros(t):
    f = t.view(-1)
    f[0] = 0.0
    f[f.numel() // 2] = -0.0
    return t


class _Case:
    """Operands (f32, CPU, NCHW) of one geometry and batch, and the f64 reference of every kernel
    on them and on their absolute values.  Built once per (geometry, batch, kind), never modified."""

    def __init__(self, geom, B, kind):
        C, Co, R, S, ST, H, W = geom
        OH, OW = (H - R) // ST + 1, (W - S) // ST + 1
        g = torch.Generator().manual_seed(1000 * B + 7 * H + W + (0 if kind == "int" else 1))
        if kind == "int":
            def draw(a, *shape):
                return torch.randint(-a, a + 1, shape, generator=g).float()
            self.x, self.w = draw(3, B, C, H, W), draw(3, Co, C, R, S)
            self.b, self.dy = draw(3, Co), draw(3, B, Co, OH, OW)
            self.aprev, self.mask = _with_zeros(draw(2, B, C, H, W)), _with_zeros(draw(2, B, Co, OH, OW))
            assert (self.mask.view(-1)[0] == 0 and torch.signbit(self.mask.view(-1)[self.mask.numel() // 2])
                    and torch.signbit(self.aprev.view(-1)[self.aprev.numel() // 2]))
        else:
            def draw(*shape):
                return torch.randn(shape, generator=g)
            self.x, self.w = draw(B, C, H, W), draw(Co, C, R, S)
            self.b, self.dy = draw(Co), draw(B, Co, OH, OW)
            self.aprev, self.mask = draw(B, C, H, W), draw(B, Co, OH, OW)
        self.geom, self.B, self.kind, self.OH, self.OW = geom, B, kind, OH, OW
        self.n = {"y": R * S * C, "dw": B * OH * OW, "db": B * OH * OW,
                  "dx": (R // ST) * (S // ST) * Co}
        # ref[masked]: y (no ReLU), dw, db, dx (a_prev mask applied); abs[masked] likewise
        self.ref, self.abs = {}, {}
        for masked in (False, True):
            keep = (self.mask.double() > 0) if masked else torch.ones_like(self.mask, dtype=torch.bool)
            below = self.aprev.double() > 0
            self.ref[masked] = self._eval(self.x.double(), self.w.double(), self.b.double(),
                                          self.dy.double() * keep, below, ST)
            self.abs[masked] = self._eval(self.x.double().abs(), self.w.double().abs(), self.b.double().abs(),
                                          self.dy.double().abs() * keep, below, ST)
        if kind == "int":
            # the premise of the exact check
            top = max(float(v.max()) for r in self.abs.values() for v in r.values())
            assert top < 2 ** 24, top

    @staticmethod
    def _eval(x, w, b, dy, below, ST):
        x, w, b = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
        y = F.conv2d(x, w, b, stride=ST)
        y.backward(dy)
        return {"y": y.detach(), "dw": w.grad, "db": b.grad, "dx": x.grad * below}


# (bounded: the parametrisation walks kind, then batch, then geometry, so the six cases of one
# geometry are what neighbouring tests share; a case met again by a later test function is rebuilt)
@functools.lru_cache(maxsize=6)
def _case(geom, B, kind):
    return _Case(geom, B, kind)


def _nhwc(t, dev):
    return t.permute(0, 2, 3, 1).contiguous().to(dev)


class _Dev:
    """The operands of a _Case on the device, in the kernels' layouts."""

    def __init__(self, case, dev):
        self.x, self.w = _nhwc(case.x, dev), _nhwc(case.w, dev)
        self.b, self.dy = case.b.to(dev), _nhwc(case.dy, dev)
        self.aprev, self.mask = _nhwc(case.aprev, dev), _nhwc(case.mask, dev)


class _Guarded:
    """n floats between two guard zones, everything NaN until a kernel writes it."""

    def __init__(self, n, dev):
        self.n = n
        self.full = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32, device=dev)
        self.t = self.full[GUARD:GUARD + n]

    def done(self, what=""):
        assert bool(torch.isnan(self.full[:GUARD]).all()), "guard zone before %s was written" % what
        assert bool(torch.isnan(self.full[GUARD + self.n:]).all()), "guard zone after %s was written" % what
        assert not bool(torch.isnan(self.t).any()), "%s: payload not fully written" % what
        return self.t


_RATIO = {}


def _note(name, ratio):
    _RATIO[name] = max(_RATIO.get(name, 0.0), ratio)


@pytest.fixture(scope="module", autouse=True)
def _ratio_summary():
    """One line per kernel after the module's last test (``pytest -s``): the largest err / bound
    of check (b) -- the figures of the COVERAGE.md row."""
    yield
    for name in sorted(_RATIO):
        print("MAX RATIO %s %.4f" % (name, _RATIO[name]))


def _verify(name, out, case, key, masked, relu=False, permute=True):
    """Check (a) or (b), by the kind of the case, of kernel output ``out`` (device; NHWC-like for
    y / dw / dx when ``permute``) against reference entry ``key``."""
    ref, ab = case.ref[masked][key], case.abs[masked][key]
    if relu:
        ref = ref.clamp(min=0)
    out = out.detach().cpu()
    if permute and ref.dim() == 4:
        out = out.view(ref.shape[0], ref.shape[2], ref.shape[3], ref.shape[1]).permute(0, 3, 1, 2)
    out = out.reshape(ref.shape)
    if case.kind == "int":
        want = ref.float()
        if not torch.equal(out, want):
            bad = (out != want).nonzero()
            i = tuple(bad[0].tolist())
            raise AssertionError("%s %s: %d elements differ, first at %s: got %r, want %r" % (
                name, _gid(case.geom), len(bad), i, float(out[i]), float(want[i])))
        return
    bound = 2 * (case.n[key] + 2) * U * ab
    err = (out.double() - ref).abs()
    ratio = float((err / bound.clamp(min=1e-300)).max())
    _note(name, ratio)
    print("RATIO %s %s B=%d %.4f" % (name, _gid(case.geom), case.B, ratio))
    assert bool((err <= bound).all()), "%s %s: err / bound = %.3f" % (name, _gid(case.geom), ratio)


# ------------------------------------------------------------------ launches
def _fwd(d, geom, B, relu, planar=False, splits=1):
    C, Co, R, S, ST, H, W = geom
    OH, OW = (H - R) // ST + 1, (W - S) // ST + 1
    M = B * OH * OW
    lib, dev = mt._native.lib(), d.x.device
    y = _Guarded(M * Co, dev)
    if splits == 1:
        mt.check(lib.pfrl_conv2d_nhwc_fwd(mt._p(d.x), mt._p(d.w), mt._p(d.b), mt._p(y.t), B, H, W, C, Co, R, S,
                                          ST, int(relu), int(planar), 1, mt._stream()), "fwd")
        return y.done("y")
    part = _Guarded(splits * M * Co, dev)
    mt.check(lib.pfrl_conv2d_nhwc_fwd(mt._p(d.x), mt._p(d.w), None, mt._p(part.t), B, H, W, C, Co, R, S, ST,
                                      0, 0, splits, mt._stream()), "fwd split-K")
    part.done("forward slabs")
    mt._reduce([(part.t, y.t, d.b, M * Co, M * Co, splits, Co, int(relu))])
    return y.done("y")


def _wgrad_out(d, geom, splits, fold, launch):
    C, Co, R, S, ST, H, W = geom
    nW, dev = Co * R * S * C, d.x.device
    dw, db = _Guarded(nW, dev), _Guarded(Co, dev)
    if splits == 1 and not fold:
        launch(dw.t, db.t, 0)
        return dw.done("dw"), db.done("db"), None
    stride = nW + Co
    part = _Guarded(splits * stride, dev)
    launch(part.t, part.t[nW:], stride)
    part.done("weight-gradient slabs")
    mt._reduce([(part.t, dw.t, None, stride, nW, splits, 4, 0), (part.t[nW:], db.t, None, stride, Co, splits, 4, 0)])
    return dw.done("dw"), db.done("db"), part.t


def _wgrad(d, geom, B, splits, masked, fold=False):
    C, Co, R, S, ST, H, W = geom
    lib = mt._native.lib()

    def launch(pw, pb, st):
        mt.check(lib.pfrl_conv2d_nhwc_bwd_weight(mt._p(d.dy), mt._p(d.mask) if masked else None, mt._p(d.x),
                                                 mt._p(pw), mt._p(pb), st, st, B, H, W, C, Co, R, S, ST,
                                                 splits, mt._stream()), "wgrad")
    return _wgrad_out(d, geom, splits, fold, launch)


def _dgrad(d, geom, B, masked):
    C, Co, R, S, ST, H, W = geom
    dx = _Guarded(B * H * W * C, d.x.device)
    mt.check(mt._native.lib().pfrl_conv2d_nhwc_bwd_data(
        mt._p(d.dy), mt._p(d.mask) if masked else None, mt._p(d.w), mt._p(d.aprev), mt._p(dx.t), B, H, W, C,
        Co, R, S, ST, 0, 0, mt._stream()), "dgrad")
    return dx.done("dx")


def _fused(d, geom, B, splits, masked):
    C, Co, R, S, ST, H, W = geom
    dx = _Guarded(B * H * W * C, d.x.device)

    def launch(pw, pb, st):
        mt.check(mt._native.lib().pfrl_conv2d_nhwc_bwd(
            mt._p(d.dy), mt._p(d.mask) if masked else None, mt._p(d.w), mt._p(d.aprev), mt._p(d.x),
            mt._p(dx.t), mt._p(pw), mt._p(pb), st, st, B, H, W, C, Co, R, S, ST, 0, 0, splits,
            mt._stream()), "fused bwd")
    dw, db, part = _wgrad_out(d, geom, splits, False, launch)
    return dx.done("dx"), dw, db, part


def _split_counts(geom, B):
    C, Co, R, S, ST, H, W = geom
    M = B * ((H - R) // ST + 1) * ((W - S) // ST + 1)
    return sorted({1, 3, mt._wgrad_splits(M, Co, R * S * C)})


# ------------------------------------------------------------------ sections 1 + 2
@gpu
@pytest.mark.parametrize("kind", ["int", "randn"])
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("geom", FIRST + UPPER, ids=_gid)
def test_forward_and_weight_gradient_match_float64(geom, B, kind):
    dev = torch.device("cuda:0")
    case = _case(geom, B, kind)
    d = _Dev(case, dev)
    C, Co, R, S, ST, H, W = geom
    for relu in (False, True):
        y = _fwd(d, geom, B, relu)
        _verify("fwd", y, case, "y", False, relu=relu)
        yp = _fwd(d, geom, B, relu, planar=True)
        assert torch.equal(yp.view(B, Co, case.OH, case.OW), y.view(B, case.OH, case.OW, Co).permute(0, 3, 1, 2))
        _verify("fwd split-K", _fwd(d, geom, B, relu, splits=3), case, "y", False, relu=relu)
    for masked in (False, True):
        for splits in _split_counts(geom, B):
            dw, db, _ = _wgrad(d, geom, B, splits, masked)
            assert dw.numel() == case.w.numel()
            _verify("wgrad dw", dw.view(Co, R, S, C), case, "dw", masked)
            _verify("wgrad db", db, case, "db", masked)


@gpu
@pytest.mark.parametrize("kind", ["int", "randn"])
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("geom", UPPER, ids=_gid)
def test_input_gradient_and_fused_launch_match_float64(geom, B, kind):
    dev = torch.device("cuda:0")
    case = _case(geom, B, kind)
    d = _Dev(case, dev)
    C, Co, R, S, ST, H, W = geom
    assert mt._fused_bwd_ok(B, H, W, C, ST, (R // ST) * (S // ST))
    for masked in (False, True):
        dx = _dgrad(d, geom, B, masked)
        _verify("dgrad", dx, case, "dx", masked)
        for splits in _split_counts(geom, B):
            dw, db, part = _wgrad(d, geom, B, splits, masked)
            fdx, fdw, fdb, fpart = _fused(d, geom, B, splits, masked)
            # one launch == the two launches, bit for bit (slabs included) ...
            assert torch.equal(fdx, dx) and torch.equal(fdw, dw) and torch.equal(fdb, db)
            assert part is None or torch.equal(fpart, part)
            # ... and right
            _verify("fused dx", fdx, case, "dx", masked)
            _verify("fused dw", fdw.view(Co, R, S, C), case, "dw", masked)
            _verify("fused db", fdb, case, "db", masked)


# ------------------------------------------------------------------ section 3
@gpu
@pytest.mark.parametrize("kind", ["int", "randn"])
@pytest.mark.parametrize("geom", FIRST + UPPER, ids=_gid)
def test_every_eligible_tile_program_matches_the_reference(geom, kind, monkeypatch):
    """Each tile program a geometry is eligible for, forced through the per-call hooks, at B = 67
    (the last tile of every program is partial) against the f64 reference -- not against another
    program.  test_every_tile_program_is_reached_by_some_geometry asserts that the matrix covers
    every id."""
    dev = torch.device("cuda:0")
    B = 67
    case = _case(geom, B, kind)
    d = _Dev(case, dev)
    C, Co, R, S, ST, H, W = geom
    for prog in fwd_programs(geom):
        monkeypatch.setenv("PFRL_QNET_FWD", str(prog))
        _verify("fwd[%d]" % prog, _fwd(d, geom, B, True), case, "y", False, relu=True)
        _verify("fwd[%d]" % prog, _fwd(d, geom, B, False, splits=3), case, "y", False)
    monkeypatch.delenv("PFRL_QNET_FWD")
    for prog in wgrad_programs(geom):
        monkeypatch.setenv("PFRL_QNET_WGRAD", str(prog))
        for splits in (1, 3):
            dw, db, _ = _wgrad(d, geom, B, splits, True, fold=True)
            _verify("wgrad[%d] dw" % prog, dw.view(Co, R, S, C), case, "dw", True)
            _verify("wgrad[%d] db" % prog, db, case, "db", True)
    monkeypatch.delenv("PFRL_QNET_WGRAD")
    if geom in UPPER:
        for prog in dgrad_programs(geom):
            monkeypatch.setenv("PFRL_QNET_DGRAD", str(prog))
            for masked in (False, True):
                _verify("dgrad[%d]" % prog, _dgrad(d, geom, B, masked), case, "dx", masked)
        monkeypatch.delenv("PFRL_QNET_DGRAD")


# ------------------------------------------------------------------ section 4: host rules
@pytest.mark.parametrize("geom", FIRST + UPPER, ids=_gid)
def test_predicted_wgrad_tile_divides_the_problem(geom):
    C, Co, R, S, ST, H, W = geom
    K = R * S * C
    for M in (100, 16384, 262144):
        bi, bj = mt._wgrad_tile(M, Co, K)
        assert Co % bi == 0 and K % bj == 0, (M, bi, bj)
        s = mt._wgrad_splits(M, Co, K)
        nch = -(-M // 32)
        cps = -(-nch // s)
        assert 1 <= s <= nch and cps * s >= nch and cps * (s - 1) < nch


def test_fused_backward_rule_follows_the_position_tiled_programs():
    """dgrad_program() picks the position-tiled programs (8, 9) from 1 024 images up whatever the
    workgroup count; pfrl_conv2d_nhwc_bwd refuses those, so the host rule must too."""
    assert mt._fused_bwd_ok(1023, 4, 4, 64, 1, 9) and not mt._fused_bwd_ok(1024, 4, 4, 64, 1, 9)
    assert mt._fused_bwd_ok(1024, 3, 5, 128, 1, 1)          # one tap: not position-tiled
    assert mt._fused_bwd_ok(1023, 4, 4, 32, 2, 1) and not mt._fused_bwd_ok(1024, 4, 4, 32, 2, 1)
    assert mt._fused_bwd_ok(1024, 6, 3, 32, 3, 1)           # 9 * 32 % 64 != 0: no merged classes
    assert mt._fused_bwd_ok(1024, 1, 1, 512, 1)             # a linear layer


def _sparse_int(shape, density, g):
    keep = torch.rand(shape, generator=g) < density
    return (torch.randint(0, 2, shape, generator=g).float() * 2 - 1) * keep


def _set_sparse_int(model, density, g):
    with torch.no_grad():
        for p in model.parameters():
            p.copy_(_sparse_int(p.shape, density, g))


def _f64_grads(model, x, gy, absolute=False):
    m = copy.deepcopy(model).double()
    x, gy = x.double(), gy.double()
    if absolute:
        with torch.no_grad():
            for p in m.parameters():
                p.abs_()
        x, gy = x.abs(), gy.abs()
    out = m(x)
    out.backward(gy)
    return out.detach(), [p.grad for p in m.parameters()]


def _to_dut(model, dev, fuse=True):
    dut = copy.deepcopy(model).to(dev).to(memory_format=torch.channels_last)
    if fuse:
        mt.fuse_sequential_trunk(dut)
        mt.accelerate_heads(dut)
    return dut


def _exact_trunk(model, x, gy, dev, run=None):
    """Check (a) of a whole model with sparse integer parameters: output and every gradient."""
    top_out, top_g = _f64_grads(model, x, gy, absolute=True)
    top = max([float(top_out.max())] + [float(t.max()) for t in top_g])
    assert top < 2 ** 24, top                                  # the premise
    want, want_g = _f64_grads(model, x, gy)
    dut = _to_dut(model, dev, fuse=run is None)
    xg = x.to(dev).contiguous(memory_format=torch.channels_last)
    out = dut(xg) if run is None else run(dut, xg)
    assert torch.equal(out.cpu(), want.float())
    out.backward(gy.to(dev))
    for (name, p), w in zip(dut.named_parameters(), want_g):
        assert p.grad is not None and torch.equal(p.grad.cpu(), w.float()), name
    return out, [p.grad for p in dut.parameters()]


def _conv_only(dut, xg):
    convs = [m for m in dut if isinstance(m, nn.Conv2d)]
    specs = mt.plan_for(convs, None, xg)
    assert specs is not None
    return mt.trunk_forward(xg, specs, convs, None)


def _border(fn):
    n = 1
    while fn(n):
        n += 1
    return n


@gpu
def test_trunk_backward_on_either_side_of_the_fused_launch_borders():
    """_fused_bwd_ok against dgrad_program(): a two-convolution stack just below and just above
    the batch at which the second layer's gradients stop sharing a launch -- the 1 024-workgroup
    border of a stride-4 layer, the 384-workgroup border of a stride-1 layer (it switches between
    two programs the fused launch both has), and the 1 024-image border
    of the position-tiled programs on maps too small to reach the workgroup counts."""
    dev = torch.device("cuda:0")
    stacks = [
        # (32, 64, 8, 8, 4) on 24 x 16
        (nn.Sequential(nn.Conv2d(4, 32, 8, 1), nn.ReLU(), nn.Conv2d(32, 64, 8, 4), nn.ReLU()), (31, 23),
         lambda n: mt._fused_bwd_ok(n, 24, 16, 32, 4, 4), (160, 180)),
        # (64, 64, 3, 3, 1) on 7 x 5: 384 workgroups of 32 x 32 from B = 175, position-tiled from 1 024.
        # This border is no host rule: the lambda restates blocks(32, 32) >= 384 of dgrad_program()
        # by hand, and the fused launch has the programs on both sides, so _fused_bwd_ok says yes at
        # 174 and at 175.  The case checks that neither batch raises and both are exact; nothing ties
        # the 175 to the C code.
        (nn.Sequential(nn.Conv2d(8, 64, 4, 1), nn.ReLU(), nn.Conv2d(64, 64, 3, 1), nn.ReLU()), (10, 8),
         lambda n: -(-35 * n // 32) * 2 < 384, (175, 175)),
        # (64, 64, 3, 3, 1) on 4 x 4
        (nn.Sequential(nn.Conv2d(8, 64, 4, 1), nn.ReLU(), nn.Conv2d(64, 64, 3, 1), nn.ReLU()), (7, 7),
         lambda n: mt._fused_bwd_ok(n, 4, 4, 64, 1, 9), (1024, 1024)),
        # (32, 64, 2, 2, 2) on 4 x 4: position-tiled by class from 1 024 images
        (nn.Sequential(nn.Conv2d(8, 32, 4, 1), nn.ReLU(), nn.Conv2d(32, 64, 2, 2), nn.ReLU()), (7, 7),
         lambda n: mt._fused_bwd_ok(n, 4, 4, 32, 2, 1), (1024, 1024)),
    ]
    for model, (H, W), rule, (lo, hi) in stacks:
        edge = _border(rule)
        assert lo <= edge <= hi, edge
        for B in (edge - 1, edge):
            g = torch.Generator().manual_seed(B)
            _set_sparse_int(model, 0.125, g)
            x = _sparse_int((B, model[0].in_channels, H, W), 0.5, g)
            with torch.no_grad():
                shape = model(x).shape
            gy = _sparse_int(shape, 0.03, g)
            _exact_trunk(model, x, gy, dev, run=_conv_only)


def _near_misses(dev):
    """(name, convs, linear, input shape) that plan_for must refuse."""
    def cl(conv):
        return conv.to(dev).to(memory_format=torch.channels_last)
    c1 = lambda: cl(nn.Conv2d(4, 32, 8, 4))                        # noqa: E731  44 x 36 -> 10 x 8
    return [
        ("H % stride at layer 2", [cl(nn.Conv2d(4, 32, 8, 1)), cl(nn.Conv2d(32, 64, 2, 2))], None, (2, 4, 16, 15)),
        ("S * C % 32", [cl(nn.Conv2d(4, 32, 6, 2))], None, (2, 4, 20, 20)),
        ("padding 1", [cl(nn.Conv2d(4, 32, 8, 4, padding=1))], None, (2, 4, 44, 36)),
        ("dilation 2", [cl(nn.Conv2d(4, 32, 8, 4, dilation=2))], None, (2, 4, 44, 36)),
        ("groups 2", [cl(nn.Conv2d(8, 32, 8, 4, groups=2))], None, (2, 8, 44, 36)),
        ("Cout = 24", [cl(nn.Conv2d(4, 24, 8, 4))], None, (2, 4, 44, 36)),
        ("stride (2, 1)", [cl(nn.Conv2d(4, 32, 8, (2, 1)))], None, (2, 4, 44, 36)),
        ("no bias", [cl(nn.Conv2d(4, 32, 8, 4, bias=False))], None, (2, 4, 44, 36)),
        ("in_features", [c1()], nn.Linear(32 * 10 * 8 + 32, 64).to(dev), (2, 4, 44, 36)),
    ]


@gpu
def test_plan_for_admits_the_matrix_and_refuses_the_near_misses():
    dev = torch.device("cuda:0")
    for geom in UPPER:
        C, Co, R, S, ST, H, W = geom
        first = nn.Conv2d(4, C, 8, 1).to(dev).to(memory_format=torch.channels_last)
        conv = nn.Conv2d(C, Co, (R, S), ST).to(dev).to(memory_format=torch.channels_last)
        x = torch.zeros(3, 4, H + 7, W + 7, device=dev)
        specs = mt.plan_for([first, conv], None, x)
        assert specs is not None and (specs[1].H, specs[1].W, specs[1].ST) == (H, W, ST), geom
        lin = nn.Linear(Co * specs[1].OH * specs[1].OW, 64).to(dev)
        assert (lin.in_features % 32 != 0) or mt.plan_for([first, conv], lin, x) is not None, geom
    for name, convs, linear, shape in _near_misses(dev):
        assert mt.plan_for(convs, linear, torch.zeros(shape, device=dev)) is None, name


@gpu
def test_c_entries_refuse_the_near_misses_without_launching():
    """The near-misses that the C ABI can express (it has no padding, dilation, groups or second
    stride argument: plan_for is the only gate for those) return PFRL_ERR_ARG and write nothing."""
    dev = torch.device("cuda:0")
    lib = mt._native.lib()
    buf = torch.zeros(1 << 18, device=dev)
    out = torch.full((1 << 18,), float("nan"), device=dev)
    p, o, s = mt._p(buf), mt._p(out), mt._stream
    rcs = {
        # layer 2 with H % stride != 0 (15 rows, stride 2)
        "dgrad H % stride": lib.pfrl_conv2d_nhwc_bwd_data(p, None, p, p, o, 2, 15, 8, 32, 64, 2, 2, 2, 0, 0, s()),
        "fused H % stride": lib.pfrl_conv2d_nhwc_bwd(p, None, p, p, p, o, o, o, 0, 0, 2, 15, 8, 32, 64, 2, 2, 2, 0,
                                                     0, 1, s()),
        # S * C = 24
        "fwd S * C % 32": lib.pfrl_conv2d_nhwc_fwd(p, p, p, o, 2, 20, 20, 4, 32, 6, 6, 2, 1, 0, 1, s()),
        "wgrad S * C % 32": lib.pfrl_conv2d_nhwc_bwd_weight(p, None, p, o, o, 0, 0, 2, 20, 20, 4, 32, 6, 6, 2, 1,
                                                            s()),
        "wgrad Cout = 24": lib.pfrl_conv2d_nhwc_bwd_weight(p, None, p, o, o, 0, 0, 2, 44, 36, 4, 24, 8, 8, 4, 1,
                                                           s()),
        "fwd no bias": lib.pfrl_conv2d_nhwc_fwd(p, p, None, o, 2, 44, 36, 4, 32, 8, 8, 4, 1, 0, 1, s()),
        # the linear layer's input gradient with a flatten that is not p * c columns
        "dgrad flatten": lib.pfrl_conv2d_nhwc_bwd_data(p, None, p, p, o, 2, 1, 1, 2592, 64, 1, 1, 1, 80, 32, 0, s()),
        # layer 2 with Cout = 48 / C = 24
        "dgrad Cout % 32": lib.pfrl_conv2d_nhwc_bwd_data(p, None, p, p, o, 2, 8, 8, 32, 48, 2, 2, 2, 0, 0, s()),
        "dgrad C % 16": lib.pfrl_conv2d_nhwc_bwd_data(p, None, p, p, o, 2, 8, 8, 24, 64, 2, 2, 2, 0, 0, s()),
    }
    assert all(rc == PFRL_ERR_ARG for rc in rcs.values()), rcs
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


# ------------------------------------------------------------------ section 5: trunks
def _stack():
    # [B, 4, 44, 36] -> 10 x 8 -> 4 x 4 -> 2 x 2
    return nn.Sequential(nn.Conv2d(4, 32, 8, 4), nn.ReLU(), nn.Conv2d(32, 64, (4, 2), 2), nn.ReLU(),
                         nn.Conv2d(64, 32, 3, 1), nn.ReLU(), nn.Flatten(), nn.Linear(128, 64), nn.ReLU(),
                         nn.Linear(64, 5))


def _odd_stack():
    # Cout = 48 first layer, C = 48 second layer: [B, 4, 44, 36] -> 10 x 8 -> 4 x 4
    return nn.Sequential(nn.Conv2d(4, 48, 8, 4), nn.ReLU(), nn.Conv2d(48, 32, (4, 2), 2), nn.ReLU(),
                         nn.Flatten(), nn.Linear(512, 64), nn.ReLU(), nn.Linear(64, 5))


def _fwd_terms(model):
    """sum of (fan-in + 2) over the layers: ReLU is 1-Lipschitz, so the forward error bounds of
    the layers add up to first order (relative to the reference on absolute operands)."""
    return sum((m.in_channels * m.kernel_size[0] * m.kernel_size[1] + 2) if isinstance(m, nn.Conv2d)
               else (m.in_features + 2) for m in model if isinstance(m, (nn.Conv2d, nn.Linear)))


def _rounded_trunk_forward(build, B, dev, run=None, name="trunk"):
    """Check (b) of a whole model's forward pass: randn input, composed bound."""
    torch.manual_seed(100 + B)
    model = build()
    if run is not None:
        model = nn.Sequential(*list(model)[:[isinstance(m, nn.Flatten) for m in model].index(True)])
    x = torch.randn(B, 4, 44, 36)
    m64 = copy.deepcopy(model).double()
    a64 = copy.deepcopy(m64)
    with torch.no_grad():
        for p in a64.parameters():
            p.abs_()
        want, top = m64(x.double()), a64(x.double().abs())
        dut = _to_dut(model, dev, fuse=run is None)
        xg = x.to(dev).contiguous(memory_format=torch.channels_last)
        out = dut(xg) if run is None else run(dut, xg)
    bound = 2 * _fwd_terms(model) * U * top
    err = (out.cpu().double() - want).abs()
    r = float((err / bound.clamp(min=1e-300)).max())
    _note(name + " fwd", r)
    print("RATIO %s fwd B=%d %.4f" % (name, B, r))
    assert bool((err <= bound).all()), r
    return out


def _int_trunk_case(build, B, seed=0, dy_density=0.06):
    g = torch.Generator().manual_seed(seed + B)
    model = build()
    with torch.no_grad():
        for m in model:
            if isinstance(m, nn.Conv2d):
                m.weight.copy_(_sparse_int(m.weight.shape, 0.125, g))
                m.bias.copy_(_sparse_int(m.bias.shape, 0.125, g))
            elif isinstance(m, nn.Linear):
                m.weight.copy_(_sparse_int(m.weight.shape, 0.0625, g))
                m.bias.copy_(_sparse_int(m.bias.shape, 0.0625, g))
    x = _sparse_int((B, 4, 44, 36), 0.5, g)
    with torch.no_grad():
        shape = model(x).shape
    return model, x, _sparse_int(shape, dy_density, g)


@gpu
@pytest.mark.parametrize("B", [1, 7, 67])
@pytest.mark.parametrize("build", [_stack, _odd_stack], ids=["stack", "odd-width"])
def test_non_atari_trunks_match_float64(build, B):
    dev = torch.device("cuda:0")
    model, x, gy = _int_trunk_case(build, B, dy_density=0.5 if B < 67 else 0.1)
    dut = _to_dut(model, dev)
    assert type(dut).__name__ == "_TrunkSequential"
    start, end, conv_idx, lin_idx = dut._trunk_run
    mods = list(dut)
    xg = x.to(dev).contiguous(memory_format=torch.channels_last)
    assert mt.plan_for([mods[k] for k in conv_idx], mods[lin_idx], xg) is not None     # the kernels do run
    _exact_trunk(model, x, gy, dev)
    _rounded_trunk_forward(build, B, dev, name=build.__name__)
    # the convolutions alone (linear=None)
    convs = nn.Sequential(*list(model)[:[isinstance(m, nn.Flatten) for m in model].index(True)])
    with torch.no_grad():
        shape = convs(x).shape
    gyc = _sparse_int(shape, 0.1, torch.Generator().manual_seed(B))
    _exact_trunk(convs, x, gyc, dev, run=_conv_only)
    _rounded_trunk_forward(build, B, dev, run=_conv_only, name=build.__name__ + " conv-only")


def _nhwc_stack():
    # [B, 4, 44, 36] -> 10 x 8 -> 4 x 3: the final map is not square
    return nn.Sequential(nn.Conv2d(4, 32, 8, 4), nn.ReLU(), nn.Conv2d(32, 64, 4, 2), nn.ReLU(), nn.Flatten(),
                         nn.Linear(768, 64), nn.ReLU(), nn.Linear(64, 5))


@gpu
def test_nhwc_route_with_a_non_square_map_equals_the_planar_route(monkeypatch):
    dev = torch.device("cuda:0")
    B = 1056
    assert B >= mt._NHWC_FC_MIN_BATCH > 0
    model, x, gy = _int_trunk_case(_nhwc_stack, B, dy_density=0.02)
    out, grads = _exact_trunk(model, x, gy, dev)                  # NHWC route, check (a)
    rout = _rounded_trunk_forward(_nhwc_stack, B, dev, name="nhwc route")       # and (b) of the forward pass
    monkeypatch.setattr(mt, "_NHWC_FC_MIN_BATCH", 0)
    pout, pgrads = _exact_trunk(model, x, gy, dev)                # planar route of the same batch
    prout = _rounded_trunk_forward(_nhwc_stack, B, dev, name="planar route")
    assert rout.shape == prout.shape
    assert torch.equal(out, pout) and all(torch.equal(a, b) for a, b in zip(grads, pgrads))


@gpu
def test_u8_first_layer_off_the_nature_shape_is_exact():
    """pfrl_conv2d_u8nhwc4_fwd / _bwd_weight with divisor 1.0 on bytes 0..3 (so the operands are
    the small integers of check (a)): Conv(4, 32, 8, 2) on 64 x 64 at B = 16 is 13 456 rows, 421
    tiles of 32 x 32."""
    from pfrl_amd import ops

    dev = torch.device("cuda:0")
    assert ops.u8_division_exact(1.0)
    B, H, W, Co, R, ST = 16, 64, 64, 32, 8, 2
    conv = nn.Conv2d(4, Co, R, ST).to(dev).to(memory_format=torch.channels_last)
    assert mt.u8_first_layer_shape_ok(conv, B, H, W, 1.0)
    g = torch.Generator().manual_seed(16)
    px = torch.randint(0, 4, (B, H, W, 4), generator=g, dtype=torch.uint8)
    w = torch.randint(-3, 4, (Co, 4, R, R), generator=g).float()
    b = torch.randint(-3, 4, (Co,), generator=g).float()
    OH = (H - R) // ST + 1
    dy = torch.randint(-3, 4, (B, Co, OH, OH), generator=g).float()
    mask = _with_zeros(torch.randint(-2, 3, (B, Co, OH, OH), generator=g).float())
    x64 = px.permute(0, 3, 1, 2).double()
    below = torch.ones_like(x64, dtype=torch.bool)
    lib = mt._native.lib()
    pxg, wg, bg = px.to(dev), _nhwc(w, dev), b.to(dev)
    for relu in (0, 1):
        y = _Guarded(B * OH * OH * Co, dev)
        mt.check(lib.pfrl_conv2d_u8nhwc4_fwd(mt._p(pxg), 1.0, mt._p(wg), mt._p(bg), mt._p(y.t), B, H, W, Co, R, R,
                                             ST, relu, 0, mt._stream()), "u8 fwd")
        ref = _Case._eval(x64, w.double(), b.double(), dy.double(), below, ST)["y"]
        assert float(_Case._eval(x64, w.double().abs(), b.double().abs(), dy.double().abs(), below, ST)["y"].max()) < 2 ** 24
        want = (ref.clamp(min=0) if relu else ref).float()
        assert torch.equal(y.done("y").cpu().view(B, OH, OH, Co).permute(0, 3, 1, 2), want)
    nW, M = Co * R * R * 4, B * OH * OH
    for masked in (False, True):
        keep = (mask.double() > 0) if masked else torch.ones_like(mask, dtype=torch.bool)
        ref = _Case._eval(x64, w.double(), b.double(), dy.double() * keep, below, ST)
        top = _Case._eval(x64, w.double().abs(), b.double().abs(), dy.double().abs() * keep, below, ST)
        assert max(float(top["dw"].max()), float(top["db"].max())) < 2 ** 24
        dyg, mg = _nhwc(dy, dev), _nhwc(mask, dev)
        for splits in sorted({1, 3, mt._wgrad_splits(M, Co, R * R * 4)}):
            stride = nW + Co
            part, dw, db = _Guarded(splits * stride, dev), _Guarded(nW, dev), _Guarded(Co, dev)
            mt.check(lib.pfrl_conv2d_u8nhwc4_bwd_weight(mt._p(dyg), mt._p(mg) if masked else None, mt._p(pxg), 1.0,
                                                        mt._p(part.t), mt._p(part.t[nW:]), stride, stride, B, H, W,
                                                        Co, R, R, ST, splits, mt._stream()), "u8 wgrad")
            part.done("u8 slabs")
            mt._reduce([(part.t, dw.t, None, stride, nW, splits, 4, 0),
                        (part.t[nW:], db.t, None, stride, Co, splits, 4, 0)])
            assert torch.equal(dw.done("dw").cpu().view(Co, R, R, 4).permute(0, 3, 1, 2), ref["dw"].float())
            assert torch.equal(db.done("db").cpu(), ref["db"].float())
