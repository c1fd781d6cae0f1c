"""ops.obs_stats_update (csrc/obsnorm.hip) against the module's update rule restated in NumPy float64.  The yardstick
is the torch float32 module (``PFRL_OBS_STATS_KERNEL=0``) on the same inputs, measured in the same test: the kernel's
largest error against float64 may be at most the module's, no factor granted.  Measured on the MI355X (kernel / module,
largest over the table): mean 3.1e-5 / 1.1e-4 (offset 1 000: half an ulp is 3.1e-5), var 6.0e-8 / 6.6e-6."""
import numpy as np
import pytest
import torch

from pfrl_amd import ops
from pfrl_amd.nn import EmpiricalNormalization

pytestmark = pytest.mark.gpu
GUARD, SENTINEL = 64, 12345.0
# (n, D, count before, data): one slab and its tails (1, 2, 63, 64), two slabs (65), several (257), more rows than
# 64 slabs of 64 (4097); one column group and its tails (1, 3, 64), two (65), six (376), eight (512)
CASES = [(1, 1, 0, "unit"), (2, 3, 1, "unit"), (63, 64, 10 ** 6, "unit"), (64, 65, 0, "offset"),
         (65, 376, 1, "offset"), (257, 512, 10 ** 6, "offset"), (4097, 3, 0, "offset"), (4097, 65, 1, "unit")]


def make(n, D, count, data):
    g = torch.Generator().manual_seed(1000 * n + D)
    x = torch.randn(n, D, generator=g)
    x = 1000.0 + 0.01 * x if data == "offset" else x
    if count == 0:
        return x, torch.zeros(D), torch.ones(D)
    return x, x[0] + 0.1 * torch.randn(D, generator=g), 0.5 + torch.rand(D, generator=g)


def rule64(x, mean, var, count):
    x, m, v = x.double().numpy(), mean.double().numpy(), var.double().numpy()
    mx, r = x.mean(0), x.shape[0] / (count + x.shape[0])
    m1 = m + r * (mx - m)
    return m1, v + r * (x.var(0) - v + (mx - m) * (mx - m1))


def module_with(mean, var, count, until=None):
    n = EmpiricalNormalization(mean.numel(), until=until).cuda()
    n._mean.copy_(mean.view(1, -1))
    n._var.copy_(var.view(1, -1))
    n.count.fill_(count)
    return n


def guarded(t):
    buf = torch.full((t.numel() + 2 * GUARD,), SENTINEL, device="cuda")
    buf[GUARD:-GUARD] = t.cuda()
    return buf[GUARD:-GUARD], buf


@pytest.mark.parametrize("n,D,count,data", CASES)
def test_against_float64_and_the_float32_module(monkeypatch, n, D, count, data):
    x, mean, var = make(n, D, count, data)
    xd, want = x.cuda(), rule64(x, mean, var, count)
    runs = []
    for fill in (0.0, float("nan")):     # two workspace states: the same bits (one order of every sum, no state kept)
        (m, mbuf), (v, vbuf), c = guarded(mean), guarded(var), torch.tensor(count, device="cuda")
        ops.obs_stats_update(xd, m, v, c, workspace=torch.full((128 * D,), fill, dtype=torch.float64, device="cuda"))
        assert int(c) == count + n
        for buf in (mbuf, vbuf):
            assert bool((buf[:GUARD] == SENTINEL).all() and (buf[-GUARD:] == SENTINEL).all())
        runs.append((m, v))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    on = module_with(mean, var, count)      # the module lands on the route ...
    on._cached_std_inverse = "stale"
    on.experience(xd)
    assert torch.equal(on._mean.view(-1), m) and torch.equal(on._var.view(-1), v) and int(on.count) == count + n
    assert on._cached_std_inverse is None
    monkeypatch.setenv("PFRL_OBS_STATS_KERNEL", "0")
    off = module_with(mean, var, count)     # ... and its torch route is the yardstick
    off.experience(xd)
    for name, got, ref, yard in (("mean", m, want[0], off._mean), ("var", v, want[1], off._var)):
        k, t = (float(np.abs(a.double().cpu().numpy().ravel() - ref).max()) for a in (got, yard))
        print("%s n=%d D=%d count=%d %s: kernel %.3e, float32 module %.3e" % (name, n, D, count, data, k, t))
        assert k <= t


def test_until_is_decided_on_the_device_and_an_empty_batch_changes_nothing():
    x, mean, var = make(65, 3, 1, "unit")
    for count, changes in ((99, True), (100, False), (101, False)):
        n = module_with(mean, var, count, until=100)
        before = [t.clone() for t in (n._mean, n._var, n.count)]
        n.experience(x.cuda())
        assert all(torch.equal(a, b) for a, b in zip(before, (n._mean, n._var, n.count))) != changes
        if changes:     # just below: the whole batch is folded in
            assert int(n.count) == count + 65
            np.testing.assert_allclose(n._mean.cpu().numpy().ravel(), rule64(x, mean, var, count)[0], rtol=1e-6)
    n = module_with(mean, var, 5)
    n.experience(x.cuda()[:0])
    assert int(n.count) == 5 and torch.equal(n._mean.cpu().view(-1), mean) and torch.equal(n._var.cpu().view(-1), var)
