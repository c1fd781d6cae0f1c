"""csrc/qnet.hip -- the linear-layer kernels (TAIL forward and weight gradient, the narrow-head
kernels, the MFMA narrow backward, the twin launches) -- over what their host gates admit, against
``torch.float64`` on the CPU, through the C ABI; and which entry points ``mfma_linear._Linear`` /
``mfma_trunk._SmallLinear`` call for a given layer, through the module.

Reference:  y = act(x w^T + b),  dx = (dy * mask) w,  dw = (dy * mask)^T x,  db = sum_m (dy * mask),
mask = (dy_mask > 0); the mask tensor is an operand (it holds +0.0 and -0.0 entries) and both sides
get the same one.

Two checks per kernel result, the method of tests/test_conv_geometry.py:

(a) exact.  Operands are small integers stored as f32 (x in -3..3, w and dy in -2..2, b in -4..4,
    about a third of the entries zero).  Every partial sum in any order is an integer far below
    2^24 (the case asserts it on the absolute operands), so outputs and slab sums must be
    ``torch.equal`` to the f64 reference cast to f32.

(b) rounded.  Operands are randn.  Per element |out - ref64| <= 2 (n + 2) 2^-24 ref64_abs, n the
    number of summed terms and ref64_abs the reference on absolute operands: the forward-error
    bound of an f32 dot product in any order with a factor 2 of margin.  ``RATIO`` lines per case,
    ``MAX RATIO <entry>`` lines after the last test (``pytest -s``).

Every output and slab buffer lies between two NaN guard zones of 4096 floats which must still be
NaN after the launch, and the payload must hold no NaN.  "Misaligned" cases base x, dy, y and dx
one float past a 16-byte boundary (odd K / N, so that the rows are misaligned too); weights stay
aligned, as parameters are.  The TAIL weight-gradient kernel loads dy and the mask 16 bytes at a
time (out_features % 16 == 0 rows of a fresh allocation), so only its x is misaligned.

Two questions this file settled on the kernels' own code:
* ``pfrl_linear_fwd`` / ``pfrl_linear_bwd_weight`` with more splits than 32-chunks: run_pipeline()
  returns at once for an empty range and the epilogue stores the zero accumulators, so the trailing
  slabs are zero slabs.  Such split counts are part of the matrix (``nch + 2``).
* ``k_linear_narrow_bwd`` at the edge of its gate (up to 65 472 bytes of dynamic LDS next to
  NT * 2 KB static) and ``k_linear_small_bwd<24..64>`` at their largest batch (static + dynamic up
  to 107 520 bytes): see test_narrow_backward_at_the_edge_of_its_gate and COVERAGE.md row a23.
"""
import functools

import pytest
import torch
import torch.nn as nn

from pfrl_amd import _native
from pfrl_amd.nn import mfma_linear as ml
from pfrl_amd.nn import mfma_trunk as mt
from pfrl_amd.nn.twin_mlp import _pair

gpu = pytest.mark.gpu

GUARD = 4096
U = 2.0 ** -24
PFRL_ERR_ARG = -2
_p, _stream, _cd = mt._p, mt._stream, mt._ceil_div


# ------------------------------------------------------------------ the shape matrices
FWD_K = [1, 3, 31, 33, 63, 65, 100, 393]
FWD_M = [1, 5, 16, 17, 67, 256, 1000]
FWD_N = [1, 5, 16, 17, 31, 33, 50, 62, 64, 96, 353]
WG_N = [16, 32, 48, 64, 256]
WG_K = [1, 3, 33, 65, 100, 393]
WG_M = [1, 5, 31, 33, 67, 256, 1000]
SMALL_MK = [(1, 1), (7, 33), (67, 256), (640, 40)]
SMALL_EDGES = [(4096, 33, 2), (2560, 9, 4), (1024, 5, 10), (4096, 300, 1)]     # M * N <= 10240, M <= 4096
WIDE_DX_N = [17, 24, 25, 40, 41, 49, 57, 64]     # (41, 49: the <48> and <56> instantiations)
NARROW_N = [17, 29, 32, 33, 34, 47, 48, 49, 64]
NARROW_K = [1, 15, 17, 40, 256, 393]
NARROW_M = [1, 5, 16, 17, 33, 256, 257, 272, 300]
NARROW_EDGE = [(496, 17), (496, 18), (496, 32), (320, 33), (320, 48), (240, 49), (240, 64)]
TWIN_M, TWIN_K, TWIN_N = [1, 17, 256], [32, 43, 393], [32, 96, 256]
TIG_NCOL, TIG_N = [1, 17, 32], [32, 128, 300, 512]


# ------------------------------------------------------------------ the dispatch rules, restated
# COPIES of the C rules in csrc/qnet.hip (and of the route conditions of mfma_linear._Linear.backward),
# kept in step by hand.  The GPU routing test compares route_entries() with the entry points a layer
# really calls, which ties the Python half to the code; the C half is tied by the results only.
def fwd_tail_program(M, N, z):
    """pfrl_linear_fwd, K % 32 != 0."""
    if N % 32 != 0 and N <= 16:
        return "32x16"
    return "32x32" if _cd(M, 32) * _cd(N, 32) * z >= 384 else "16x32"


def wgrad_tail_program(N):
    """pfrl_linear_bwd_weight, K % 32 != 0 (N % 16 == 0)."""
    return "32x32" if N % 32 == 0 else "16x32"


def small_bwd_width(N):
    """The k_linear_small_bwd instantiation small_bwd_launch picks."""
    return N if N <= 16 else _cd(N, 8) * 8


def small_bwd_admits(M, N):
    return 1 <= N <= 64 and M >= 1 and M * small_bwd_width(N) * 4 <= 40 * 1024


NARROW_STATIC_PER_NT = 2 * 64 * 4 * 4          # comb[2][NT][64][4]


def narrow_lds(M, N):
    """(dynamic, static) bytes of LDS of k_linear_narrow_bwd<ceil(N / 16)>."""
    NT, M16 = _cd(N, 16), _cd(M, 16) * 16
    return M16 * (16 * NT + 1) * 4, NT * NARROW_STATIC_PER_NT


def narrow_c_gate(M, N):
    """PFRL_CHECK_ARG of pfrl_linear_small_bwd for dw != NULL, N > 16."""
    return 17 <= N <= 64 and M >= 1 and narrow_lds(M, N)[0] <= 64 * 1024 and M * N <= 256 * 64


def narrow_py_gate(M, K, N, relu, need_w=True):
    """The first condition of mfma_linear._Linear.backward."""
    return (not ml._bwd_kernels_cover(M, K, N) and not relu and N <= 64 and N % 16 != 0
            and _cd(M, 16) * 16 * (_cd(N, 16) * 16 + 1) * 4 <= 65536 and need_w)


def linear_route(M, K, N, relu, need_dx, need_w):
    """Which branch of _Linear.backward a layer takes."""
    if narrow_py_gate(M, K, N, relu, need_w):
        return "narrow"
    if not ml._bwd_kernels_cover(M, K, N):
        if need_w and N % 16 == 0:
            return "tail wgrad"
        return "library"
    if not need_w:
        return "frozen"
    if not need_dx:
        return "wgrad only"
    return "fused" if mt._fused_bwd_ok(M, 1, 1, K, 1) else "two launches"


def route_entries(M, K, N, relu, need_dx, need_w):
    """(entry points of forward, entry points of backward) for an ml._LinearSlot layer."""
    fwd = {"pfrl_linear_fwd"} | ({"pfrl_splitk_reduce"} if ml._fwd_splits(M, N, K) > 1 else set())
    r = linear_route(M, K, N, relu, need_dx, need_w)
    fold = {"pfrl_splitk_reduce"}
    if r == "narrow":
        return fwd, {"pfrl_linear_small_bwd"}
    if r == "library":
        return fwd, set()
    if r == "tail wgrad":
        return fwd, {"pfrl_linear_bwd_weight"} | (fold if mt._wgrad_splits(M, N, _cd(K, 32) * 32) > 1 else set())
    if r == "frozen":
        return fwd, {"pfrl_conv2d_nhwc_bwd_data"} if need_dx else set()
    bwd = fold if mt._wgrad_splits(M, N, K) > 1 else set()
    if r == "fused":
        return fwd, bwd | {"pfrl_conv2d_nhwc_bwd"}
    if r == "two launches":
        return fwd, bwd | {"pfrl_conv2d_nhwc_bwd_data", "pfrl_conv2d_nhwc_bwd_weight"}
    return fwd, bwd | {"pfrl_conv2d_nhwc_bwd_weight"}


def _fwd_split_counts(M, K, N):
    nch = _cd(K, 32)
    # 1, the host rule's, 2, the most without an empty split, and two empty splits on top
    return sorted({1, ml._fwd_splits(M, N, K), 2, nch, nch + 2})


def _wgrad_split_counts(M, K, N):
    nch = _cd(M, 32)
    return sorted({1, mt._wgrad_splits(M, N, _cd(K, 32) * 32), 2, nch, nch + 2})


def _fwd_shapes():
    """A covering subset of FWD_M x FWD_K x FWD_N (+ the 6-split 32 x 32 case): a third of the
    product, chosen so that test_every_linear_program_is_reached_by_the_matrix holds."""
    out = []
    for i, M in enumerate(FWD_M):
        for j, K in enumerate(FWD_K):
            for k, N in enumerate(FWD_N):
                if (i + j + k) % 3 == 0 or (M, N) == (1000, 353) or (M >= 67 and K == 393 and (N == 353 or M == 1000)):
                    out.append((M, K, N))
    return out + [(256, K, 256) for K in FWD_K]


def _wgrad_shapes():
    return [(M, K, N) for i, M in enumerate(WG_M) for j, K in enumerate(WG_K) for k, N in enumerate(WG_N)
            if (i + j + k) % 2 == 0]


def _narrow_shapes():
    out = [(M, K, N) for i, M in enumerate(NARROW_M) for j, K in enumerate(NARROW_K)
           for k, N in enumerate(NARROW_N) if (i + j + k) % 3 == 0 and narrow_c_gate(M, N)]
    return out + [(M, K, N) for M, N in NARROW_EDGE for K in (17, 40)]


def _fwd_coverage(shapes):
    """{(axis, value, program, 'direct' | 'split')} over shapes x their split counts."""
    cov = set()
    for M, K, N in shapes:
        for z in _fwd_split_counts(M, K, N) + ([6] if (M, N) == (256, 256) else []):
            tag = (fwd_tail_program(M, N, z), "direct" if z == 1 else "split")
            cov |= {("M", M) + tag, ("K", K) + tag, ("N", N) + tag}
    return cov


def test_every_linear_program_is_reached_by_the_matrix():
    """No GPU: the bookkeeping behind the matrix tests, by the rules restated above."""
    # forward TAIL: the pruned matrix reaches, for every listed M, K and N, every (program, direct /
    # split) that the whole product reaches for that value -- and every program both ways at all
    full = [(M, K, N) for M in FWD_M for K in FWD_K for N in FWD_N]
    got, want = _fwd_coverage(_fwd_shapes()), _fwd_coverage(full)
    assert want <= got, sorted(want - got)
    assert {c[2:] for c in got} == {(p, d) for p in ("32x16", "32x32", "16x32") for d in ("direct", "split")}
    assert fwd_tail_program(1000, 353, 1) == "32x32" and fwd_tail_program(256, 256, 6) == "32x32"
    assert fwd_tail_program(256, 256, 5) == "16x32"
    # weight gradient TAIL: both programs for every M and K, direct and split
    wg = {(axis, v, wgrad_tail_program(N), "direct" if z == 1 else "split")
          for M, K, N in _wgrad_shapes() for z in _wgrad_split_counts(M, K, N) for axis, v in (("M", M), ("K", K))}
    assert wg == {(a, v, p, d) for a, vs in (("M", WG_M), ("K", WG_K)) for v in vs for p in ("32x32", "16x32")
                  for d in ("direct", "split")}
    assert {N for _, _, N in _wgrad_shapes()} == set(WG_N)
    # small kernels: every width 1..16, the six wide widths of the input-gradient form
    assert {small_bwd_width(N) for N in range(1, 17)} == set(range(1, 17))
    assert {small_bwd_width(N) for N in WIDE_DX_N} == {24, 32, 40, 48, 56, 64}
    for N in WIDE_DX_N:
        M = 10240 // small_bwd_width(N)
        assert small_bwd_admits(M, N) and not small_bwd_admits(M + 1, N)
    assert all(M * N <= 10240 and M <= 4096 and small_bwd_admits(M, N) for M, _, N in SMALL_EDGES)
    assert small_bwd_admits(640, 16) and not small_bwd_admits(641, 16)
    # narrow backward: every NT, every listed value, the reload loop (M16 > 256) and the gate's edge per NT
    ns = _narrow_shapes()
    assert {_cd(N, 16) for _, _, N in ns} == {2, 3, 4}
    assert ({M for M, _, _ in ns} >= set(NARROW_M) and {K for _, K, _ in ns} >= set(NARROW_K)
            and {N for _, _, N in ns} >= set(NARROW_N))
    for NT in (2, 3, 4):
        edge = max(M for M in range(1, 1025) if narrow_c_gate(M, 16 * NT))
        assert (edge, 16 * NT) in NARROW_EDGE and edge == {2: 496, 3: 320, 4: 240}[NT]
        assert not narrow_c_gate(edge + 1, 16 * NT - 15)
    assert any(_cd(M, 16) * 16 > 256 and N <= 32 for M, _, N in ns)          # the s0 > 0 loop
    assert any(_cd(M, 16) * 16 > 256 and 32 < N <= 48 for M, _, N in ns)
    # routes of _Linear.backward
    routes = {linear_route(*c) for c in ROUTE_CASES}
    assert routes == {"narrow", "tail wgrad", "library", "frozen", "fused", "two launches", "wgrad only"}


def test_python_narrow_route_admits_only_what_the_c_gate_admits():
    """Every (M, N) in [1, 1024] x [17, 64] that _Linear.backward sends to pfrl_linear_small_bwd
    passes that entry's own argument check (M * N <= 16384 and the LDS formula)."""
    n = 0
    for M in range(1, 1025):
        for N in range(17, 65):
            if narrow_py_gate(M, 33, N, False):
                n += 1
                assert narrow_c_gate(M, N), (M, N)
    assert n > 0
    # the first sizes the C gate refuses, per NT
    assert [max(M for M in range(1, 1025) if narrow_c_gate(M, N)) for N in (32, 48, 64)] == [496, 320, 240]


# ------------------------------------------------------------------ operands and reference
def _with_zeros(t):
    f = t.view(-1)
    f[0] = 0.0
    f[f.numel() // 2] = -0.0
    return t


class _Case:
    """Operands (f32, CPU) of one (M, K, N) and kind and the f64 reference of every product on them
    and on their absolute values.  Built once, never modified."""

    def __init__(self, M, K, N, kind, seed=0):
        g = torch.Generator().manual_seed(100003 * M + 1009 * K + 7 * N + seed + (0 if kind == "int" else 1))
        if kind == "int":
            def draw(a, *shape):
                keep = torch.rand(shape, generator=g) < 0.75         # ~ a third zero with the drawn zeros
                return torch.randint(-a, a + 1, shape, generator=g).float() * keep
            self.x, self.w, self.b = draw(3, M, K), draw(2, N, K), draw(4, N)
            self.dy, self.mask = draw(2, M, N), _with_zeros(draw(2, M, N))
        else:
            def draw(*shape):
                return torch.randn(shape, generator=g)
            self.x, self.w, self.b = draw(M, K), draw(N, K), draw(N)
            self.dy, self.mask = draw(M, N), _with_zeros(draw(M, N))
        if M * N >= 2:
            assert torch.signbit(self.mask.view(-1)[M * N // 2]) and self.mask.view(-1)[0] == 0
        self.M, self.K, self.N, self.kind = M, K, N, kind
        self.n = {"y": K, "y0": K, "dx": N, "dw": M, "db": M}
        X, W, B, DY = self.x.double(), self.w.double(), self.b.double(), self.dy.double()
        self.ref, self.abs = {}, {}
        for masked in (False, True):
            keep = (self.mask.double() > 0) if masked else torch.ones_like(DY, dtype=torch.bool)
            self.ref[masked] = self._eval(X, W, B, DY * keep)
            self.abs[masked] = self._eval(X.abs(), W.abs(), B.abs(), DY.abs() * keep)
        if kind == "int":
            top = max(float(v.max()) for r in self.abs.values() for v in r.values())
            assert top < 2 ** 24, top                                  # the premise of the exact check

    @staticmethod
    def _eval(X, W, B, G):
        y0 = X @ W.t()
        return {"y": y0 + B, "y0": y0, "dx": G @ W, "dw": G.t() @ X, "db": G.sum(0)}

    def tag(self):
        return "M%d-K%d-N%d" % (self.M, self.K, self.N)


@functools.lru_cache(maxsize=8)
def _case(M, K, N, kind, seed=0):
    return _Case(M, K, N, kind, seed)


class _Guarded:
    """n floats between two guard zones, everything NaN until a kernel writes it.  off = 1 bases the
    payload one float past a 16-byte boundary."""

    def __init__(self, n, dev, off=0):
        self.n, self.lo = n, GUARD + off
        self.full = torch.full((n + 2 * GUARD + 4,), float("nan"), dtype=torch.float32, device=dev)
        assert self.full.data_ptr() % 16 == 0
        self.t = self.full[self.lo:self.lo + n]

    def done(self, what=""):
        assert bool(torch.isnan(self.full[:self.lo]).all()), "guard zone before %s was written" % what
        assert bool(torch.isnan(self.full[self.lo + self.n:]).all()), "guard zone after %s was written" % what
        assert not bool(torch.isnan(self.t).any()), "%s: payload not fully written" % what
        return self.t

    def untouched(self, what=""):
        assert bool(torch.isnan(self.full).all()), "%s was written" % what


def _put(t, dev, off=0):
    """A device copy of CPU tensor t, contiguous, optionally one float past a 16-byte boundary."""
    if not off:
        return t.to(dev).contiguous()
    buf = torch.zeros(t.numel() + 8, dtype=torch.float32, device=dev)
    out = buf[off:off + t.numel()].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 4 * off and out.is_contiguous()
    return out


class _Dev:
    def __init__(self, case, dev, off=0, off_dy=None):
        off_dy = off if off_dy is None else off_dy
        self.x, self.dy, self.mask = _put(case.x, dev, off), _put(case.dy, dev, off_dy), _put(case.mask, dev, off_dy)
        self.w, self.b = case.w.to(dev), case.b.to(dev)


_RATIO = {}


@pytest.fixture(scope="module", autouse=True)
def _ratio_summary():
    yield
    for name in sorted(_RATIO):
        print("MAX RATIO %s %.4f" % (name, _RATIO[name]))


def _verify(name, out, case, key, masked=False, relu=False, ref=None, ab=None, n=None, tag=None):
    """Check (a) or (b), by the kind of the case, of ``out`` against reference entry ``key``."""
    ref = case.ref[masked][key] if ref is None else ref
    ab = case.abs[masked][key] if ab is None else ab
    n = case.n[key] if n is None else n
    tag = tag or case.tag()
    if relu:
        ref = ref.clamp(min=0)
    out = out.detach().cpu().reshape(ref.shape)
    if case.kind == "int":
        want = ref.float()
        if not torch.equal(out, want):
            bad = (out != want).nonzero()
            i = tuple(bad[0].tolist())
            raise AssertionError("%s %s: %d elements differ, first at %s: got %r, want %r" % (
                name, tag, len(bad), i, float(out[i]), float(want[i])))
        return
    bound = 2 * (n + 2) * U * ab
    err = (out.double() - ref).abs()
    ratio = float((err / bound.clamp(min=1e-300)).max())
    _RATIO[name] = max(_RATIO.get(name, 0.0), ratio)
    print("RATIO %s %s %.4f" % (name, tag, ratio))
    assert bool((err <= bound).all()), "%s %s: err / bound = %.3f" % (name, tag, ratio)


def _slab_sum(part, splits, stride, n, case):
    """Sum of the slabs: in f32 on integer operands (exact), in f64 otherwise."""
    slabs = part.view(splits, stride)[:, :n] if stride else part.view(splits, n)
    return slabs.sum(0) if case.kind == "int" else slabs.double().sum(0)


# ------------------------------------------------------------------ CPU: the reference against itself
@pytest.mark.parametrize("shape", [(5, 33, 17), (67, 100, 16), (17, 393, 34), (256, 65, 8)], ids=str)
def test_float64_reference_on_integer_operands_is_what_f32_computes(shape):
    """The premise of check (a), without a GPU: on the integer operands plain f32 arithmetic on the
    CPU reproduces the f64 reference bit for bit, masks with +0.0 / -0.0 included."""
    c = _case(*shape, "int")
    assert abs(float((c.x == 0).float().mean()) - 1 / 3) < 0.12 or c.x.numel() < 50
    keep = (c.mask > 0).float()
    g = c.dy * keep
    assert torch.equal(c.x @ c.w.t() + c.b, c.ref[False]["y"].float())
    assert torch.equal(g @ c.w, c.ref[True]["dx"].float())
    assert torch.equal(g.t() @ c.x, c.ref[True]["dw"].float())
    assert torch.equal(g.sum(0), c.ref[True]["db"].float())
    assert torch.equal(c.dy.t() @ c.x, c.ref[False]["dw"].float())


# ------------------------------------------------------------------ pfrl_linear_fwd, TAIL
def _linear_fwd(d, case, relu, splits, off=0):
    M, K, N = case.M, case.K, case.N
    lib, dev = _native.lib(), d.x.device
    y = _Guarded(M * N, dev, off)
    if splits == 1:
        mt.check(lib.pfrl_linear_fwd(_p(d.x), _p(d.w), _p(d.b), _p(y.t), M, K, N, int(relu), 1, _stream()), "fwd")
        return y.done("y"), None
    part = _Guarded(splits * M * N, dev, off)
    mt.check(lib.pfrl_linear_fwd(_p(d.x), _p(d.w), None, _p(part.t), M, K, N, 0, splits, _stream()), "fwd split-K")
    part.done("forward slabs")
    if N % 4 or off:
        return None, part.t              # (the fold kernel moves aligned float4 columns: slab sum only)
    mt._reduce([(part.t, y.t, d.b, M * N, M * N, splits, N, int(relu))])
    return y.done("y"), part.t


def _check_linear_fwd(case, dev, off=0):
    M, K, N = case.M, case.K, case.N
    d = _Dev(case, dev, off)
    extra = [6] if (M, N) == (256, 256) else []
    for z in sorted(set(_fwd_split_counts(M, K, N) + extra)):
        name = "linear_fwd %s %s" % (fwd_tail_program(M, N, z), "direct" if z == 1 else "split-K")
        for relu in ((False, True) if z == 1 else (True,)):
            y, part = _linear_fwd(d, case, relu, z, off)
            if y is not None:
                _verify(name, y, case, "y", relu=relu)
            if part is not None:
                _verify(name + " slabs", _slab_sum(part, z, 0, M * N, case), case, "y0")
                nch = _cd(K, 32)
                if z > nch:          # trailing splits without a chunk: zero slabs
                    cps = _cd(nch, z)
                    used = _cd(nch, cps)
                    assert not bool(part.view(z, M * N)[used:].any())


@gpu
@pytest.mark.parametrize("kind", ["int", "randn"])
@pytest.mark.parametrize("K", FWD_K)
def test_linear_forward_tail_matches_float64(K, kind):
    dev = torch.device("cuda:0")
    for M, KK, N in _fwd_shapes():
        if KK == K:
            _check_linear_fwd(_case(M, K, N, kind), dev)


@gpu
@pytest.mark.parametrize("kind", ["int", "randn"])
def test_linear_forward_tail_with_misaligned_rows(kind):
    """x and y one float past a 16-byte boundary, odd K and N: every row is misaligned (what
    ``x[1:]`` of a contiguous tensor with odd K hands to _Linear.forward)."""
    dev = torch.device("cuda:0")
    for M, K, N in [(5, 33, 5), (67, 65, 17), (17, 393, 33), (1000, 31, 353), (256, 63, 15), (67, 3, 31)]:
        _check_linear_fwd(_case(M, K, N, kind), dev, off=1)


# ------------------------------------------------------------------ pfrl_linear_bwd_weight, TAIL
def _linear_wgrad(d, case, splits, masked):
    M, K, N = case.M, case.K, case.N
    lib, dev = _native.lib(), d.x.device
    nW = N * K
    dw, db = _Guarded(nW, dev), _Guarded(N, dev)
    mk = _p(d.mask) if masked else None
    if splits == 1:
        mt.check(lib.pfrl_linear_bwd_weight(_p(d.dy), mk, _p(d.x), _p(dw.t), _p(db.t), 0, 0, M, K, N, 1, _stream()),
                 "wgrad")
        return dw.done("dw"), db.done("db"), None
    stride = nW + N
    part = _Guarded(splits * stride, dev)
    mt.check(lib.pfrl_linear_bwd_weight(_p(d.dy), mk, _p(d.x), _p(part.t), _p(part.t[nW:]), stride, stride, M, K, N,
                                        splits, _stream()), "wgrad slabs")
    part.done("weight-gradient slabs")
    mt._reduce([(part.t, dw.t, None, stride, nW, splits, 4, 0), (part.t[nW:], db.t, None, stride, N, splits, 4, 0)])
    return dw.done("dw"), db.done("db"), part.t


def _check_linear_wgrad(case, dev, off=0):
    M, K, N = case.M, case.K, case.N
    d = _Dev(case, dev, off, off_dy=0)
    prog = wgrad_tail_program(N)
    for z in _wgrad_split_counts(M, K, N):
        for masked in ((False, True) if z == 1 else (True,)):
            name = "linear_bwd_weight %s %s" % (prog, "direct" if z == 1 else "slabs")
            dw, db, part = _linear_wgrad(d, case, z, masked)
            _verify(name + " dw", dw, case, "dw", masked)
            _verify(name + " db", db, case, "db", masked)
            if part is not None:
                stride = N * K + N
                _verify(name + " dw", _slab_sum(part, z, stride, N * K, case), case, "dw", masked)
                _verify(name + " db", _slab_sum(part.view(z, stride)[:, N * K:].contiguous(), z, 0, N, case),
                        case, "db", masked)


@gpu
@pytest.mark.parametrize("kind", ["int", "randn"])
@pytest.mark.parametrize("K", WG_K)
def test_linear_weight_gradient_tail_matches_float64(K, kind):
    dev = torch.device("cuda:0")
    for M, KK, N in _wgrad_shapes():
        if KK == K:
            _check_linear_wgrad(_case(M, K, N, kind), dev)


@gpu
@pytest.mark.parametrize("kind", ["int", "randn"])
def test_linear_weight_gradient_tail_with_misaligned_x(kind):
    dev = torch.device("cuda:0")
    for M, K, N in [(5, 33, 16), (67, 65, 48), (33, 393, 32), (1000, 3, 64)]:
        _check_linear_wgrad(_case(M, K, N, kind), dev, off=1)


# ------------------------------------------------------------------ narrow-head kernels (N <= 16)
def _small_fwd(d, case, bias, off=0, twin=None):
    M, K, N = case.M, case.K, case.N
    y = _Guarded(M * N, d.x.device, off)
    mt.check(_native.lib().pfrl_linear_small_fwd(_p(d.x), _p(d.w), _p(d.b) if bias else None, _p(y.t), M, K, N,
                                                 _stream()), "small fwd")
    return y.done("y")


def _small_bwd(d, case, want_dx, want_dw, off=0, want_db=True):
    """pfrl_linear_small_bwd (no mask argument: the head has no activation).  -> dx, dw, db"""
    M, K, N = case.M, case.K, case.N
    dev = d.x.device
    dx = _Guarded(M * K, dev, off) if want_dx else None
    dw = _Guarded(N * K, dev) if want_dw else None
    db = _Guarded(N, dev) if want_dw and want_db else None
    mt.check(_native.lib().pfrl_linear_small_bwd(
        _p(d.dy), _p(d.x), _p(d.w), _p(dx.t) if dx else None, _p(dw.t) if dw else None, _p(db.t) if db else None,
        M, K, N, _stream()), "small bwd")
    return tuple(g.done(n) if g is not None else None for g, n in ((dx, "dx"), (dw, "dw"), (db, "db")))


def _check_small(case, dev, off=0):
    d = _Dev(case, dev, off)
    name = "linear_small"
    _verify(name + "_fwd", _small_fwd(d, case, True, off), case, "y")
    _verify(name + "_fwd", _small_fwd(d, case, False, off), case, "y0")
    for want_dx, want_dw, want_db in ((True, True, True), (True, False, False), (False, True, True),
                                      (True, True, False)):
        dx, dw, db = _small_bwd(d, case, want_dx, want_dw, off, want_db)
        for key, got in (("dx", dx), ("dw", dw), ("db", db)):
            if got is not None:
                _verify("%s_bwd %s" % (name, key), got, case, key)


@gpu
@pytest.mark.parametrize("kind", ["int", "randn"])
@pytest.mark.parametrize("N", range(1, 17))
def test_small_linear_every_width_matches_float64(N, kind):
    """k_linear_small_fwd<N> / k_linear_small_bwd<N>: with and without bias, the three backward
    call forms (and the one without db); (640, 40, 16) is the edge of both gates."""
    dev = torch.device("cuda:0")
    for M, K in SMALL_MK:
        _check_small(_case(M, K, N, kind), dev)
    if N % 2:
        _check_small(_case(7, 33, N, kind), dev, off=1)
        _check_small(_case(67, 255, N, kind), dev, off=1)


@gpu
@pytest.mark.parametrize("kind", ["int", "randn"])
def test_small_linear_at_the_edges_of_its_gates(kind):
    dev = torch.device("cuda:0")
    for M, K, N in SMALL_EDGES:
        _check_small(_case(M, K, N, kind), dev)


@gpu
@pytest.mark.parametrize("kind", ["int", "randn"])
@pytest.mark.parametrize("N", WIDE_DX_N)
def test_small_backward_wide_input_gradient_matches_float64(N, kind):
    """dw == NULL with N in 17..64: k_linear_small_bwd<24 | 32 | 40 | 48 | 56 | 64> with the LDS
    copy of dy zero-padded to the instantiated width, each at the largest batch its gate admits."""
    dev = torch.device("cuda:0")
    Mmax = 10240 // small_bwd_width(N)
    for M, K, off in ((Mmax, 33, 0), (Mmax, 300, 0), (7, 1, 0), (67, 257, 1 if N % 2 else 0)):
        case = _case(M, K, N, kind)
        dx, _, _ = _small_bwd(_Dev(case, dev, off), case, True, False, off)
        _verify("linear_small_bwd<%d> dx" % small_bwd_width(N), dx, case, "dx")


@gpu
def test_small_backward_refuses_the_first_size_past_its_gate():
    dev = torch.device("cuda:0")
    lib = _native.lib()
    buf = torch.zeros(1 << 16, device=dev)
    out = _Guarded(1 << 16, dev)
    p, o = _p(buf), _p(out.t)
    rcs = {"M * N": lib.pfrl_linear_small_bwd(p, p, p, o, o, o, 641, 4, 16, _stream()),
           "wide dx": lib.pfrl_linear_small_bwd(p, p, p, o, None, None, 161, 4, 64, _stream()),
           "N = 65": lib.pfrl_linear_small_bwd(p, p, p, o, None, None, 4, 4, 65, _stream()),
           "nothing": lib.pfrl_linear_small_bwd(p, p, p, None, None, None, 4, 4, 4, _stream()),
           "fwd N = 17": lib.pfrl_linear_small_fwd(p, p, p, o, 4, 4, 17, _stream())}
    assert all(rc == PFRL_ERR_ARG for rc in rcs.values()), rcs
    torch.cuda.synchronize()
    out.untouched("an output of a refused call")


# ------------------------------------------------------------------ k_linear_narrow_bwd (N in 17..64, dw wanted)
def _check_narrow(case, dev, off=0):
    d = _Dev(case, dev, off)
    NT = _cd(case.N, 16)
    for want_dx in (True, False):
        dx, dw, db = _small_bwd(d, case, want_dx, True, off)
        for key, got in (("dx", dx), ("dw", dw), ("db", db)):
            if got is not None:
                _verify("linear_narrow_bwd<%d> %s" % (NT, key), got, case, key)


@gpu
@pytest.mark.parametrize("kind", ["int", "randn"])
@pytest.mark.parametrize("N", NARROW_N)
def test_narrow_backward_matches_float64(N, kind):
    dev = torch.device("cuda:0")
    for M, K, NN in _narrow_shapes():
        if NN == N and (M, N) not in NARROW_EDGE:
            _check_narrow(_case(M, K, N, kind), dev)
    if N % 2:
        for M, K in ((5, 17), (257 if narrow_c_gate(257, N) else 33, 15)):
            _check_narrow(_case(M, K, N, kind), dev, off=1)


@gpu
@pytest.mark.parametrize("kind", ["int", "randn"])
@pytest.mark.parametrize("MN", NARROW_EDGE, ids=lambda mn: "M%d-N%d" % mn)
def test_narrow_backward_at_the_edge_of_its_gate(MN, kind):
    """The largest batch the gate admits per NT: the s0 > 0 reload loop (M16 > 256) and the full
    LDS request -- up to 65 472 bytes dynamic on top of NT * 2 KB static."""
    dev = torch.device("cuda:0")
    M, N = MN
    assert narrow_c_gate(M, N) and not narrow_c_gate(M + 16, N) and narrow_py_gate(M, 17, N, False) == (N % 16 != 0)
    for K in (17, 40):
        _check_narrow(_case(M, K, N, kind), dev)


@gpu
def test_narrow_backward_refuses_the_first_size_past_its_gate():
    dev = torch.device("cuda:0")
    lib = _native.lib()
    buf = torch.zeros(1 << 16, device=dev)
    out = _Guarded(1 << 16, dev)
    p, o = _p(buf), _p(out.t)
    rcs = {(M, N): lib.pfrl_linear_small_bwd(p, p, p, o, o, o, M, 16, N, _stream())
           for M, N in ((497, 17), (497, 32), (321, 33), (321, 48), (241, 49), (241, 64), (16, 65))}
    assert all(rc == PFRL_ERR_ARG for rc in rcs.values()), rcs
    torch.cuda.synchronize()
    out.untouched("an output of a refused call")


# ------------------------------------------------------------------ twin launches
def _twin_cases(M, K, N, kind):
    return _case(M, K, N, kind, 0), _case(M, K, N, kind, 50)


def _split_cols(x, K1, dev):
    return x[:, :K1].contiguous().to(dev), x[:, K1:].contiguous().to(dev)


def _twin_fwd(cases, devs, K1, relu):
    M, K, N = cases[0].M, cases[0].K, cases[0].N
    dev = devs[0].w.device
    ys = [_Guarded(M * N, dev) for _ in range(2)]
    if K1:
        halves = [_split_cols(c.x, K1, dev) for c in cases]
        xa, xb = _pair(halves[0][0], halves[1][0]), _pair(halves[0][1], halves[1][1])
    else:
        xa, xb = _pair(devs[0].x, devs[1].x), None
    mt.check(_native.lib().pfrl_linear_fwd_twin(xa, xb, K1, _pair(devs[0].w, devs[1].w), _pair(devs[0].b, devs[1].b),
                                                _pair(ys[0].t, ys[1].t), M, K, N, int(relu), _stream()), "fwd twin")
    return [y.done("y") for y in ys]


@gpu
@pytest.mark.parametrize("kind", ["int", "randn"])
@pytest.mark.parametrize("K", TWIN_K)
def test_twin_forward_matches_float64_and_the_single_launches(K, kind):
    """pfrl_linear_fwd_twin, aligned and TAIL, with and without the x2 / K1 column split.  The
    single-network entry runs the same 16 x 32 program (stages of 4) for all of these shapes --
    K % 32 != 0: fewer than 384 tiles of 32 x 32; K = 32: fwd_program() 6 -- so the twin launch is
    also bit-identical to two pfrl_linear_fwd calls; a column split of an ALIGNED layer takes the
    TAIL loaders, which the single entry does not, and is checked against float64 only."""
    dev = torch.device("cuda:0")
    for M in TWIN_M:
        for N in TWIN_N:
            cases = _twin_cases(M, K, N, kind)
            devs = [_Dev(c, dev) for c in cases]
            assert fwd_tail_program(M, N, 1) == "16x32" and (K % 32 or _cd(K, 32) < 12)
            for K1 in [0] + sorted({k for k in (1, K - 1, 376) if 1 <= k < K}):
                relu = (M + N + K1) % 2 == 0 or K1 == 0
                ys = _twin_fwd(cases, devs, K1, relu)
                for c, d, y in zip(cases, devs, ys):
                    _verify("linear_fwd_twin %s" % ("TAIL" if K % 32 or K1 else "aligned"), y, c, "y", relu=relu)
                    if K % 32 or not K1:
                        single, _ = _linear_fwd(d, c, relu, 1)
                        assert torch.equal(y, single), (M, K, N, K1)


def _twin_bwd(cases, devs, K1, want_dx, want_dw, splits, masked):
    M, K, N = cases[0].M, cases[0].K, cases[0].N
    dev = devs[0].w.device
    nW, stride = N * K, N * K + N
    dxs = [_Guarded(M * K, dev) for _ in range(2)] if want_dx else None
    parts = [_Guarded(splits * stride, dev) for _ in range(2)] if want_dw else None
    xa = xb = None
    if want_dw:
        if K1:
            halves = [_split_cols(c.x, K1, dev) for c in cases]
            xa, xb = _pair(halves[0][0], halves[1][0]), _pair(halves[0][1], halves[1][1])
        else:
            xa = _pair(devs[0].x, devs[1].x)
    mt.check(_native.lib().pfrl_linear_bwd_twin(
        _pair(devs[0].dy, devs[1].dy), _pair(devs[0].mask, devs[1].mask) if masked else None,
        _pair(devs[0].w, devs[1].w), xa, xb, K1, _pair(dxs[0].t, dxs[1].t) if want_dx else None,
        _pair(parts[0].t, parts[1].t) if want_dw else None,
        _pair(parts[0].t[nW:], parts[1].t[nW:]) if want_dw else None, stride, stride, M, K, N, splits, _stream()),
        "bwd twin")
    return ([g.done("dx") for g in dxs] if want_dx else None,
            [g.done("twin slabs") for g in parts] if want_dw else None)


@gpu
@pytest.mark.parametrize("kind", ["int", "randn"])
@pytest.mark.parametrize("form", ["fused", "dgrad", "wgrad aligned", "wgrad TAIL"])
def test_twin_backward_in_its_four_forms_matches_float64(form, kind):
    dev = torch.device("cuda:0")
    if form == "wgrad TAIL":
        shapes = [(M, K, N, K1) for M in TWIN_M for K, N in ((43, 32), (393, 96), (393, 256), (32, 96))
                  for K1 in sorted({k for k in (0, 1, K - 1, 376) if k < K}) if K % 32 or K1]
    else:
        shapes = [(M, K, N, 0) for M in TWIN_M + [67] for K, N in ((32, 32), (64, 96), (256, 256), (96, 32))]
    want_dx, want_dw = form in ("fused", "dgrad"), form != "dgrad"
    for M, K, N, K1 in shapes:
        cases = _twin_cases(M, K, N, kind)
        devs = [_Dev(c, dev) for c in cases]
        zs = sorted({1, mt._wgrad_splits(M, N, _cd(K, 32) * 32), _cd(M, 32)}) if want_dw else [1]
        for z in zs:
            for masked in ((False, True) if z == zs[0] else (True,)):
                dxs, parts = _twin_bwd(cases, devs, K1, want_dx, want_dw, z, masked)
                for t, c in enumerate(cases):
                    name = "linear_bwd_twin %s" % form
                    if want_dx:
                        _verify(name + " dx", dxs[t], c, "dx", masked)
                    if want_dw:
                        stride = N * K + N
                        _verify(name + " dw", _slab_sum(parts[t], z, stride, N * K, c), c, "dw", masked)
                        _verify(name + " db", _slab_sum(parts[t].view(z, stride)[:, N * K:].contiguous(), z, 0, N, c),
                                c, "db", masked)


@gpu
@pytest.mark.parametrize("kind", ["int", "randn"])
def test_small_twin_launches_equal_the_single_launches_bit_for_bit(kind):
    dev = torch.device("cuda:0")
    lib = _native.lib()
    for M, K, N in [(1, 1, 1), (7, 33, 3), (67, 256, 6), (256, 256, 1), (640, 40, 16), (17, 300, 11)]:
        cases = _twin_cases(M, K, N, kind)
        devs = [_Dev(c, dev) for c in cases]
        for bias in (True, False):
            ys = [_Guarded(M * N, dev) for _ in range(2)]
            mt.check(lib.pfrl_linear_small_fwd_twin(
                _pair(devs[0].x, devs[1].x), _pair(devs[0].w, devs[1].w),
                _pair(devs[0].b, devs[1].b) if bias else _pair(None, None), _pair(ys[0].t, ys[1].t), M, K, N,
                _stream()), "small fwd twin")
            for c, d, y in zip(cases, devs, ys):
                assert torch.equal(y.done("y"), _small_fwd(d, c, bias))
                _verify("linear_small_fwd_twin", y.t, c, "y" if bias else "y0")
        for want_dx, want_dw in ((True, True), (True, False), (False, True)):
            outs = [[_Guarded(n, dev) if want else None for n, want in
                     ((M * K, want_dx), (N * K, want_dw), (N, want_dw))] for _ in range(2)]

            def pair(i):
                return _pair(outs[0][i].t, outs[1][i].t) if outs[0][i] is not None else None
            mt.check(lib.pfrl_linear_small_bwd_twin(
                _pair(devs[0].dy, devs[1].dy), _pair(devs[0].x, devs[1].x), _pair(devs[0].w, devs[1].w), pair(0),
                pair(1), pair(2), M, K, N, _stream()), "small bwd twin")
            for c, d, o in zip(cases, devs, outs):
                single = _small_bwd(d, c, want_dx, want_dw)
                for key, got, ref in zip(("dx", "dw", "db"), o, single):
                    if got is not None:
                        assert torch.equal(got.done(key), ref), (M, K, N, key)
                        _verify("linear_small_bwd_twin " + key, got.t, c, key)


@gpu
@pytest.mark.parametrize("kind", ["int", "randn"])
@pytest.mark.parametrize("N", TIG_N)
def test_twin_input_gradient_matches_float64(N, kind):
    """pfrl_twin_input_grad: dx[m][j] = sum over both networks and n of (dy * mask)[m][n] w[n][col0 + j]:
    the 16-wave MFMA kernel (N % 128 == 0), the 4-wave one (N % 32 == 0) and the scalar one (N = 300)."""
    dev = torch.device("cuda:0")
    lib = _native.lib()
    for ncol in TIG_NCOL:
        if 2 * N * ncol * 4 > 60 * 1024:
            buf, out = torch.zeros(1 << 16, device=dev), _Guarded(1024, dev)
            two = _pair(buf, buf)
            assert lib.pfrl_twin_input_grad(two, two, two, 64, 0, ncol, _p(out.t), 4, N, _stream()) == PFRL_ERR_ARG
            torch.cuda.synchronize()
            out.untouched("dx of a refused call")
            continue
        for M in (1, 17, 67, 256):
            for masked in (False, True):
                ldw = 40 + ncol                                     # the first layer's in_features
                col0 = ldw - ncol
                cases = _twin_cases(M, ldw, N, kind)
                devs = [_Dev(c, dev) for c in cases]
                dx = _Guarded(M * ncol, dev)
                mt.check(lib.pfrl_twin_input_grad(
                    _pair(devs[0].dy, devs[1].dy), _pair(devs[0].mask, devs[1].mask) if masked else None,
                    _pair(devs[0].w, devs[1].w), ldw, col0, ncol, _p(dx.t), M, N, _stream()), "twin input grad")
                ref = sum(c.ref[masked]["dx"][:, col0:] for c in cases)
                ab = sum(c.abs[masked]["dx"][:, col0:] for c in cases)
                _verify("twin_input_grad", dx.done("dx"), cases[0], "dx", ref=ref, ab=ab, n=2 * N,
                        tag="M%d-N%d-ncol%d" % (M, N, ncol))


# ------------------------------------------------------------------ routing
# (M, K, N, relu, need_dx, need_w)
ROUTE_CASES = [
    (256, 256, 256, True, True, True),       # fused launch
    (1024, 2048, 32, True, True, True),      # _fused_bwd_ok false: two launches
    (256, 256, 256, True, True, False),      # frozen weights
    (256, 256, 256, True, False, True),      # first layer of an aligned MLP: weight gradient only
    (256, 393, 256, True, True, True),       # tail wgrad + library dx
    (256, 393, 256, True, False, True),
    (256, 256, 34, False, True, True),       # narrow
    (256, 256, 34, True, True, True),        # library (the narrow kernel has no mask)
    (256, 256, 50, False, True, True),       # library (66 560 bytes of LDS)
    (67, 393, 48, False, True, True),        # tail wgrad, 16 x 32
]


class _Recorder:
    """Stands in for the object _native.lib() returns: records the names of the pfrl_* entries used."""

    def __init__(self, lib):
        self._lib, self.names = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name.startswith("pfrl_") and name != "pfrl_amd_last_error":
            self.names.append(name)
        return fn

    def take(self):
        out, self.names = set(self.names), []
        return out


def _int_layer(case, dev, need_w):
    layer = nn.Linear(case.K, case.N)
    with torch.no_grad():
        layer.weight.copy_(case.w)
        layer.bias.copy_(case.b)
    layer = layer.to(dev)
    for p in layer.parameters():
        p.requires_grad_(need_w)
    return layer


def _route_reference(case, relu):
    """f64 forward and gradients of act(x w^T + b) for dy; the mask comes from the layer's own output."""
    y = case.ref[False]["y"]
    keep = (y > 0) if relu else torch.ones_like(y, dtype=torch.bool)
    g = case.dy.double() * keep
    return ((y.clamp(min=0) if relu else y).float(), (g @ case.w.double()).float(),
            (g.t() @ case.x.double()).float(), g.sum(0).float())


@gpu
@pytest.mark.parametrize("sink", [False, True], ids=["fold", "slab_sink"])
@pytest.mark.parametrize("case_", ROUTE_CASES, ids=lambda c: "M%d-K%d-N%d-relu%d-dx%d-w%d" % c)
def test_linear_slot_calls_the_entries_its_route_names_and_is_exact(case_, sink, monkeypatch):
    dev = torch.device("cuda:0")
    M, K, N, relu, need_dx, need_w = case_
    case = _case(M, K, N, "int")
    rec = _Recorder(_native.lib())
    monkeypatch.setattr(_native, "lib", lambda: rec)
    slot = ml._LinearSlot(_int_layer(case, dev, need_w))
    x = case.x.to(dev).requires_grad_(need_dx)
    assert ml.supported(slot, x)
    want_fwd, want_bwd = route_entries(M, K, N, relu, need_dx, need_w)
    y_ref, dx_ref, dw_ref, db_ref = _route_reference(case, relu)
    y = slot(x, relu=relu)
    assert rec.take() == want_fwd
    assert torch.equal(y.cpu(), y_ref)
    if sink:
        with ml.slab_sink() as slabs:
            y.backward(case.dy.to(dev))
    else:
        slabs = {}
        y.backward(case.dy.to(dev))
    called = rec.take()
    route = linear_route(M, K, N, relu, need_dx, need_w)
    z = {"tail wgrad": mt._wgrad_splits(M, N, _cd(K, 32) * 32), "fused": mt._wgrad_splits(M, N, K),
         "two launches": mt._wgrad_splits(M, N, K), "wgrad only": mt._wgrad_splits(M, N, K)}.get(route, 1)
    sunk = sink and z > 1
    assert called == (want_bwd - {"pfrl_splitk_reduce"} if sunk else want_bwd), (route, called)
    if need_dx:
        assert torch.equal(x.grad.cpu(), dx_ref)
    if not need_w:
        assert slot.weight.grad is None and slot.bias.grad is None
    elif sunk:
        assert slot.weight.grad is None and slot.bias.grad is None
        assert set(slabs) == {slot.weight.data_ptr(), slot.bias.data_ptr()}
        for p, ref in ((slot.weight, dw_ref), (slot.bias, db_ref)):
            part, stride, splits = slabs[p.data_ptr()]
            assert splits == z and stride == N * K + N
            total = torch.stack([part[s * stride:s * stride + p.numel()] for s in range(splits)]).sum(0)
            assert torch.equal(total.cpu().view(ref.shape), ref)
    else:
        assert not slabs
        assert torch.equal(slot.weight.grad.cpu(), dw_ref) and torch.equal(slot.bias.grad.cpu(), db_ref)


@gpu
@pytest.mark.parametrize("need_w", [True, False], ids=["trainable", "frozen"])
def test_small_linear_slot_calls_the_narrow_head_entries_and_is_exact(need_w, monkeypatch):
    dev = torch.device("cuda:0")
    case = _case(256, 256, 8, "int")
    rec = _Recorder(_native.lib())
    monkeypatch.setattr(_native, "lib", lambda: rec)
    slot = mt._SmallLinearSlot(_int_layer(case, dev, need_w))
    x = case.x.to(dev).requires_grad_(True)
    assert mt.small_linear_supported(slot, x) and not ml.supported(slot, x)
    with ml.slab_sink() as slabs:
        y = slot(x)
        assert rec.take() == {"pfrl_linear_small_fwd"}
        y.backward(case.dy.to(dev))
        assert rec.take() == {"pfrl_linear_small_bwd"}
    y_ref, dx_ref, dw_ref, db_ref = _route_reference(case, False)
    assert not slabs and torch.equal(y.cpu(), y_ref) and torch.equal(x.grad.cpu(), dx_ref)
    if need_w:
        assert torch.equal(slot.weight.grad.cpu(), dw_ref) and torch.equal(slot.bias.grad.cpu(), db_ref)
    else:
        assert slot.weight.grad is None and slot.bias.grad is None
