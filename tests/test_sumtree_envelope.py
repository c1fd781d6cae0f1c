"""csrc/sumtree.hip driven entry by entry through hand-filled descriptors, against the NumPy
restatement of tests/test_sumtree_envelope_cpu.py (pinned there to the C oracle, its case lists
proven there to reach every route): after every launch all four node arrays are compared WHOLE and
bit for bit -- ring slots outside the frame hold sentinels, nodes off the touched paths must keep
their bits -- the outputs are compared exactly (the weights within 1 ulp of float32: the device's
double pow against NumPy's), and every buffer sits between guard zones of 0xFF bytes.
"""
import ctypes

import numpy as np
import pytest
import torch

from test_sumtree_envelope_cpu import (ABSENT, FAST_CASES, FUSED_CASES, PY, REPAIR_CASES, SAMPLE_CASES,
                                       Layout, apply_repair, build_repair_case, clip_priorities,
                                       fspec, fused_us, initial_trees, repair_route, sampler_route)

pytestmark = pytest.mark.gpu

GUARD = 4096


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from pfrl_amd import _native

    _native.lib()  # fail loudly if the HIP library is missing
    return torch.device("cuda:0")


def _ops():
    from pfrl_amd import ops

    return ops


class Guarded:
    """``n`` elements of ``dtype`` between two guard zones; everything starts as 0xFF bytes."""

    def __init__(self, dev, dtype, n):
        self.nbytes = n * torch.empty(0, dtype=dtype).element_size()
        pad = (-self.nbytes) % 16
        self.buf = torch.full((2 * GUARD + self.nbytes + pad,), 0xFF, dtype=torch.uint8, device=dev)
        self.t = self.buf[GUARD:GUARD + self.nbytes].view(dtype)

    def set(self, a):
        self.t.copy_(torch.from_numpy(np.ascontiguousarray(a)).to(self.t.device))
        return self

    def get(self):
        return self.t.cpu().numpy()

    def guards_ok(self):
        return bool((self.buf[:GUARD] == 255).all()) and bool((self.buf[GUARD + self.nbytes:] == 255).all())

    def untouched(self):
        return bool((self.buf == 255).all())


_pristine = {}      # (frame spec, leaves) -> the four node arrays on the device (2^21 leaves and up)
NAMES = ("sum_val", "sum_tag", "min_val", "min_tag")


class DeviceTrees:
    """The model's trees uploaded into guarded node arrays, the descriptor that points at them,
    and the expected arrays (on the device: the 2^23-leaf frame is 300 MB)."""

    def __init__(self, dev, tr, lay, key=None):
        from pfrl_amd._native import MAX_LEVELS, TreeDesc

        self.dev, self.lay = dev, lay
        big = tr.frame.log2_size >= 21
        if big and key in _pristine:
            flat = _pristine[key]
        else:
            flat = [torch.from_numpy(a).to(dev) for a in lay.flatten(tr)]
            if big:
                _pristine[key] = flat
        self.arr = []
        for a in flat:
            g = Guarded(dev, a.dtype, a.numel())
            g.t.copy_(a)
            self.arr.append(g)
        self.exp = [a.clone() for a in flat]
        self.maxp_v = Guarded(dev, torch.float64, 1).set(np.array([tr.maxp[0]]))
        self.maxp_t = Guarded(dev, torch.uint8, 1).set(np.array([tr.maxp[1]], dtype=np.uint8))
        f = tr.frame
        d = self.desc = TreeDesc()
        d.sum_val, d.sum_tag, d.min_val, d.min_tag = (g.t.data_ptr() for g in self.arr)
        d.maxp_val, d.maxp_tag = self.maxp_v.t.data_ptr(), self.maxp_t.t.data_ptr()
        for l in range(MAX_LEVELS):
            d.level_off[l] = lay.level_off[l]
            d.origin[l] = f.origin[l]
        d.base, d.head, d.length, d.log2_size, d.log2_smax = f.base, f.head, f.length, f.log2_size, lay.log2_smax
        tr.dirty = []

    def check(self, tr, what, min_untouched=False):
        """All four node arrays equal the model's, bit for bit; max_priority; the guard zones."""
        torch.cuda.synchronize()
        f = tr.frame
        if min_untouched:
            assert {w for w, _, _ in tr.dirty} <= {0}, what
        for which in (0, 1):
            nodes = sorted({(l, j) for w, l, j in tr.dirty if w == which})
            if nodes:
                idx = np.array([self.lay.index(f, l, j) for l, j in nodes], dtype=np.int64)
                v = np.array([tr.lv[which][l][0][j] for l, j in nodes], dtype=np.float64)
                t = np.array([tr.lv[which][l][1][j] for l, j in nodes], dtype=np.uint8)
                idx = torch.from_numpy(idx).to(self.dev)
                self.exp[2 * which][idx] = torch.from_numpy(v).to(self.dev)
                self.exp[2 * which + 1][idx] = torch.from_numpy(t).to(self.dev)
        tr.dirty = []
        if self.lay.n_nodes <= 1 << 17:     # the patched arrays ARE the model's trees, whole
            for e, m in zip(self.exp, self.lay.flatten(tr)):
                m = m.view(np.int64) if m.dtype == np.float64 else m
                e = e.cpu().numpy()
                assert np.array_equal(e.view(np.int64) if e.dtype == np.float64 else e, m), what
        for name, g, e in zip(NAMES, self.arr, self.exp):
            got, want = (g.t.view(torch.int64), e.view(torch.int64)) if e.dtype == torch.float64 else (g.t, e)
            if not torch.equal(got, want):
                bad = torch.nonzero(got != want).flatten()[:6].cpu().numpy()
                lev = [int(np.searchsorted(self.lay.level_off[:self.lay.log2_smax + 1], i, "right")) - 1
                       for i in bad]
                raise AssertionError("%s: %s differs at %s (levels %s): got %s, want %s" % (
                    what, name, bad, lev, g.t[bad].cpu().numpy(), e[bad].cpu().numpy()))
            assert g.guards_ok(), "%s: write outside %s" % (what, name)
        assert (float(self.maxp_v.get()[0]), int(self.maxp_t.get()[0])) == tr.maxp, what
        assert self.maxp_v.guards_ok() and self.maxp_t.guards_ok(), what


class SampleOut:
    FIELDS = (("x", torch.int64, 0), ("pri", torch.float64, 0), ("pri_tag", torch.uint8, 0),
              ("prob", torch.float64, 0), ("weight", torch.float32, 0), ("total", torch.float64, 1),
              ("total_tag", torch.uint8, 1), ("min_prob", torch.float64, 1), ("slot", torch.int32, 0))

    def __init__(self, dev, B):
        self.g = {k: Guarded(dev, dt, n or B) for k, dt, n in self.FIELDS}

    def out(self, slot):
        return {k: g.t for k, g in self.g.items() if slot or k != "slot"}

    def untouched(self):
        return all(g.untouched() for g in self.g.values())


def ulp32(a, b):
    ai, bi = (x.view(np.int32).astype(np.int64) for x in (a, b))
    ai, bi = (np.where(x < 0, -(x & 0x7FFFFFFF), x) for x in (ai, bi))
    return np.where(np.isnan(a) & np.isnan(b), 0, np.abs(ai - bi))


MAX_WEIGHT_ULP = [0]


def check_sample(so, want, slot_mod, what):
    torch.cuda.synchronize()
    got = {k: g.get() for k, g in so.g.items()}
    for k in ("x", "pri", "pri_tag"):
        assert np.array_equal(got[k], want[k]), (what, k, got[k], want[k])
    assert (got["total"][0], got["total_tag"][0]) == (want["total"], want["total_tag"]), what
    assert np.array_equal(got["prob"].view(np.int64), want["prob"].view(np.int64)), (what, "prob")
    assert got["min_prob"].view(np.int64)[0] == np.float64(want["min_prob"]).view(np.int64), (what, "min_prob")
    ulp = int(ulp32(got["weight"], want["weight"]).max())
    MAX_WEIGHT_ULP[0] = max(MAX_WEIGHT_ULP[0], ulp)
    print("%s: weights differ by at most %d ulp (running maximum %d)" % (what, ulp, MAX_WEIGHT_ULP[0]))
    assert ulp <= 1, (what, "weight", ulp)
    if slot_mod:
        assert np.array_equal(got["slot"], want["slot"]) and got["slot"].dtype == np.int32, (what, "slot")
    else:
        assert so.g["slot"].untouched(), what
    assert all(g.guards_ok() for g in so.g.values()), "%s: write outside an output" % what


def _dev(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _pow_mode(alpha):
    mode = _ops().powf_host_variant(alpha)
    assert mode is not None, "this host's libm powf is not glibc's"
    return mode


def _err_args(case):
    lo, hi = clip_priorities(case.cfg)
    return (case.cfg.error_min, lo, case.cfg.error_max, hi, case.cfg.eps, case.cfg.alpha)


def launch_repair(dev, case, st, a):
    """The case's launch; returns write_sum's guarded (old_val, old_tag)."""
    ops, d = _ops(), st.desc
    x = _dev(dev, a["x"])
    if case.entry == "write":
        return ops.tree_write(d, x, _dev(dev, a["val"]), _dev(dev, a["tag"]), _dev(dev, a["use_maxp"]))
    if case.entry == "write_sum":
        old = Guarded(dev, torch.float64, case.B), Guarded(dev, torch.uint8, case.B)
        ops.tree_write_sum(d, x, _dev(dev, a["val"]), _dev(dev, np.where(a["tag"] == ABSENT, PY, a["tag"])),
                           old[0].t, old[1].t)
        return old
    if case.entry == "set_priorities":
        return ops.tree_set_priorities(d, x, _dev(dev, a["val"]), _dev(dev, a["tag"]), dedupe=bool(case.dedupe))
    kw = dict(dedupe=bool(case.dedupe), pow_mode=_pow_mode(case.cfg.alpha))
    if case.entry == "update_errors":
        return ops.tree_update_errors_f32(d, x, _dev(dev, a["err"]), *_err_args(case), **kw)
    ops.tree_update_errors_write_f32(d, x, _dev(dev, a["err"]), *_err_args(case), writes=_writes(dev, case, a), **kw)


def _writes(dev, case, a):
    if not case.n:
        return (torch.empty(0, dtype=torch.int64, device=dev), torch.empty(0, dtype=torch.float64, device=dev),
                torch.empty(0, dtype=torch.uint8, device=dev), torch.empty(0, dtype=torch.uint8, device=dev))
    return tuple(_dev(dev, a[k]) for k in ("wx", "wval", "wtag", "wmaxp"))


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SAMPLE_CASES, ids=lambda c: c.name)
def test_sampler(dev, case):
    """pfrl_tree_sample: k_tree_sample_lean2 up to 2^21 leaves, k_tree_sample above."""
    tr = initial_trees(case.frame, case.leaves)
    st = DeviceTrees(dev, tr, Layout(case.frame.smax), (case.frame, case.leaves))
    B = len(case.us)
    so = SampleOut(dev, B)
    _ops().tree_sample(st.desc, _dev(dev, case.us), so.out(case.slot_mod), case.normalize, case.beta,
                       case.slot_mod)
    want = tr.sample(case.us, case.normalize, case.beta, case.slot_mod)
    what = "%s (%s)" % (case.name, sampler_route(case.frame.L))
    check_sample(so, want, case.slot_mod, what)
    st.check(tr, what, min_untouched=True)


@pytest.mark.parametrize("case", REPAIR_CASES, ids=lambda c: c.name)
def test_repair(dev, case):
    """The five repair entries on the route their gates choose."""
    tr, lay, a = build_repair_case(case)
    st = DeviceTrees(dev, tr, lay, (case.frame, case.leaves))
    old = launch_repair(dev, case, st, a)
    want = apply_repair(case, tr, a)
    what = "%s (%s)" % (case.name, repair_route(case.frame.L, case.B + case.n)
                        if case.entry == "update_errors_write" else "levels")
    st.check(tr, what, min_untouched=case.entry == "write_sum")
    if case.entry == "write_sum":
        assert np.array_equal(old[0].get().view(np.int64), want[0].view(np.int64)), what
        assert np.array_equal(old[1].get(), want[1]) and old[0].guards_ok() and old[1].guards_ok(), what


@pytest.mark.parametrize("case", FAST_CASES, ids=lambda c: c.name)
def test_hashed_repair_equals_level_by_level_repair(dev, monkeypatch, case):
    """Every launch repair_paths_hashed admits, again with PFRL_TREE_REPAIR=levels: the node
    arrays of both routes equal the model's, so each other's, bit for bit."""
    runs = []
    for route in ("hashed", "levels"):
        if route == "levels":
            monkeypatch.setenv("PFRL_TREE_REPAIR", "levels")
        else:
            monkeypatch.delenv("PFRL_TREE_REPAIR", raising=False)
        tr, lay, a = build_repair_case(case)
        st = DeviceTrees(dev, tr, lay, (case.frame, case.leaves))
        launch_repair(dev, case, st, a)
        apply_repair(case, tr, a)
        st.check(tr, "%s (%s)" % (case.name, route))
        runs.append(st)
    for g, h in zip(runs[0].arr, runs[1].arr):
        assert torch.equal(g.buf, h.buf), case.name


@pytest.mark.parametrize("case", FUSED_CASES, ids=lambda c: c.name)
def test_fused_launch_equals_the_two_launches(dev, case):
    """pfrl_tree_update_errors_write_sample against pfrl_tree_update_errors_write_f32 followed by
    pfrl_tree_sample, and both against the model."""
    ops = _ops()
    us = fused_us(case)
    runs = []
    for fused in (False, True):
        tr, lay, a = build_repair_case(case)
        st = DeviceTrees(dev, tr, lay)
        so = SampleOut(dev, len(us))
        if fused:
            ops.tree_update_errors_write_sample(
                st.desc, _dev(dev, a["x"]), _dev(dev, a["err"]), *_err_args(case),
                _writes(dev, case, a) if case.n else None, _dev(dev, us), so.out(9973), 1, 0.4, 9973,
                dedupe=bool(case.dedupe), pow_mode=_pow_mode(case.cfg.alpha))
        else:
            launch_repair(dev, case, st, a)
            ops.tree_sample(st.desc, _dev(dev, us), so.out(9973), 1, 0.4, 9973)
        apply_repair(case, tr, a)
        want = tr.sample(us, 1, 0.4, 9973)
        what = "%s (%s)" % (case.name, "fused" if fused else "two launches")
        check_sample(so, want, 9973, what)
        st.check(tr, what)
        runs.append((st, so))
    for g, h in zip(runs[0][0].arr, runs[1][0].arr):
        assert torch.equal(g.buf, h.buf), case.name
    for k in runs[0][1].g:
        assert torch.equal(runs[0][1].g[k].buf, runs[1][1].g[k].buf), (case.name, k)


# ---------------------------------------------------------------------------------------------
def _small_state(dev, L=9):
    spec = fspec(L, 300, 100) if L == 9 else fspec(L, 1)
    tr = initial_trees(spec, "mixed")
    return tr, DeviceTrees(dev, tr, Layout(spec.smax))


def _refused(call):
    with pytest.raises(RuntimeError, match="pfrl_amd"):
        call()


def test_refusals_return_an_error_and_write_nothing(dev):
    from pfrl_amd import _native

    ops, lib = _ops(), _native.lib()
    tr, st = _small_state(dev)
    d, f = st.desc, tr.frame
    x = _dev(dev, f.head + np.arange(1025, dtype=np.int64) % f.length)
    val = torch.ones(1025, dtype=torch.float64, device=dev)
    tag = torch.full((1025,), PY, dtype=torch.uint8, device=dev)
    err = torch.full((1025,), 0.5, dtype=torch.float32, device=dev)
    old = Guarded(dev, torch.float64, 1025), Guarded(dev, torch.uint8, 1025)
    cfg = (0, 0.1, 1, 1.0, 0.01, 0.6)
    w = lambda n: (x[:n].contiguous(), val[:n].contiguous(), tag[:n].contiguous(), tag[:n].contiguous())
    so = SampleOut(dev, 400)
    u = torch.full((400,), 0.5, dtype=torch.float64, device=dev)
    sample = lambda B: lib.pfrl_tree_sample(
        ctypes.byref(d), B, ops._ptr(u), *(ops._ptr(so.g[k].t) for k in
                                          ("x", "pri", "pri_tag", "prob", "weight", "total", "total_tag", "min_prob")),
        1, 0.4, 0, None, ops._stream())
    # n = 1025 on each of the five repair entries
    _refused(lambda: ops.tree_write(d, x, val, tag, tag))
    _refused(lambda: ops.tree_write_sum(d, x, val, tag, old[0].t, old[1].t))
    _refused(lambda: ops.tree_set_priorities(d, x, val, tag))
    _refused(lambda: ops.tree_update_errors_f32(d, x, err, *cfg))
    _refused(lambda: ops.tree_update_errors_write_f32(d, x[:1000].contiguous(), err[:1000].contiguous(), *cfg,
                                                      writes=w(25)))
    # the sampler: B > length, B < 0
    assert sample(f.length + 1) != 0 and sample(-1) != 0
    # the fused entry: Be + n = 65, Be = 0, L = 0, L = 22
    fused = lambda desc, Be, n: ops.tree_update_errors_write_sample(
        desc, x[:Be].contiguous(), err[:Be].contiguous(), *cfg, w(n) if n else None, u[:8].contiguous(),
        so.out(0), 1, 0.4)
    _refused(lambda: fused(d, 40, 25))
    _refused(lambda: fused(d, 0, 3))
    tr0, st0 = _small_state(dev, 0)
    _refused(lambda: fused(st0.desc, 1, 0))
    d.log2_size = 22                    # (refused before anything is read through the descriptor)
    _refused(lambda: fused(d, 8, 8))
    d.log2_size = f.log2_size
    # pow_mode = 3
    _refused(lambda: ops.tree_update_errors_f32(d, x[:8].contiguous(), err[:8].contiguous(), *cfg, pow_mode=3))
    _refused(lambda: ops.tree_update_errors_write_f32(d, x[:8].contiguous(), err[:8].contiguous(), *cfg,
                                                      writes=w(2), pow_mode=3))
    _refused(lambda: ops.tree_update_errors_write_sample(
        d, x[:8].contiguous(), err[:8].contiguous(), *cfg, None, u[:8].contiguous(), so.out(0), 1, 0.4,
        pow_mode=3))
    # a null write list with n > 0
    x8, e8 = x[:8].contiguous(), err[:8].contiguous()
    assert lib.pfrl_tree_update_errors_write_f32(
        ctypes.byref(d), 8, ops._ptr(x8), ops._ptr(e8), 1, 0.0, 0.1, 1, 1.0, 1.0, 0.01, 0.6, 1, 0, 3,
        None, None, None, None, ops._stream()) != 0
    st.check(tr, "after the refusals")
    st0.check(tr0, "after the refusals (L = 0)")
    assert so.untouched() and old[0].untouched() and old[1].untouched()


def test_empty_launches_write_nothing(dev):
    ops = _ops()
    tr, st = _small_state(dev)
    d = st.desc
    e = lambda dt: torch.empty(0, dtype=dt, device=dev)
    x, v, t, err = e(torch.int64), e(torch.float64), e(torch.uint8), e(torch.float32)
    so = SampleOut(dev, 4)
    ops.tree_write(d, x, v, t, t)
    ops.tree_write_sum(d, x, v, t)
    ops.tree_set_priorities(d, x, v, t)
    ops.tree_update_errors_f32(d, x, err, 0, 0.1, 1, 1.0, 0.01, 0.6)
    ops.tree_update_errors_write_f32(d, x, err, 0, 0.1, 1, 1.0, 0.01, 0.6, writes=(x, v, t, t))
    ops.tree_sample(d, v, so.out(5), 1, 0.4, 5)
    st.check(tr, "empty launches")
    assert so.untouched()
