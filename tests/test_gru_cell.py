"""pfrl_gru_cell_fwd (csrc/gru.hip) against the float64 formulas.  Yardstick per case: the maximum error of the same formulas in
float32 on the CPU; the kernel may err twice as much (+ 1e-7 where gates saturate and the yardstick can be exactly 0).  The ids name
the edge of the split: MT = 1 / 2 / 4 M-tiles of 16 rows, 64 rows per workgroup, 256 at most, U = 4 units, 16-byte loads iff
I % 4 == H % 4 == 0.  Measured on the MI355X (pytest -s prints every figure): COVERAGE a37."""
import pytest
import torch

from pfrl_amd import _native, ops

pytestmark = pytest.mark.gpu
CASES = {   # id: (N, I, H[, state given, bias, scale of x])
    "one-row-one-unit": (1, 1, 1), "scalar-load-tails": (3, 7, 5), "M-tile-edge-vector-loads": (17, 36, 20),
    "row-block-edge": (65, 16, 16), "envelope-edge": (256, 3, 3), "example-width": (8, 512, 512),
    "no-state": (17, 36, 20, False), "no-bias": (17, 36, 20, True, False), "saturated": (17, 36, 20, True, True, 20)}


def _formulas(x, h0, w_ih, w_hh, b_ih, b_hh):
    H = w_hh.shape[1]
    gi = x @ w_ih.T + (0 if b_ih is None else b_ih)
    gh = (0 if h0 is None else h0 @ w_hh.T) + (x.new_zeros(3 * H) if b_hh is None else b_hh)
    r, z = torch.sigmoid(gi[:, :H] + gh[..., :H]), torch.sigmoid(gi[:, H:2 * H] + gh[..., H:2 * H])
    n = torch.tanh(gi[:, 2 * H:] + r * gh[..., 2 * H:])
    return (1 - z) * n + (0 if h0 is None else z * h0)


def _case(name):   # inputs (f32, CPU), the float64 h1, the yardstick's maximum error
    N, I, H, state, bias, scale = CASES[name] + (True, True, 1)[len(CASES[name]) - 3:]
    g = torch.Generator().manual_seed(sorted(CASES).index(name))
    w_ih, w_hh, b_ih, b_hh = ((torch.rand(s, generator=g) * 2 - 1) / H ** 0.5 for s in ((3 * H, I), (3 * H, H), (3 * H,), (3 * H,)))
    x, h0 = torch.randn((N, I), generator=g) * scale, torch.randn((N, H), generator=g)
    inputs = (x, h0 if state else None, w_ih, w_hh, b_ih if bias else None, b_hh if bias else None)
    want = _formulas(*(None if t is None else t.double() for t in inputs))
    return inputs, want, float((_formulas(*inputs).double() - want).abs().max())


@pytest.mark.parametrize("name", CASES)
def test_kernel_against_float64_twice_and_guarded(name):
    inputs, want, yard = _case(name)
    args = [None if t is None else t.cuda() for t in inputs]
    h1, y = ops.gru_cell_step(*args, want_output=True)
    assert torch.equal(h1, ops.gru_cell_step(*args)), "two launches differ"
    assert torch.equal(h1, y) and h1.data_ptr() != y.data_ptr()            # the output and the state: two buffers, equal contents
    N, H = want.shape
    buf = torch.full((2, N + 2, H + 3), float("nan"), device="cuda")       # sentinel rows round h1 and y
    outs = [b.view(-1)[H:H + N * H] for b in buf]
    ptr = [None if t is None else t.data_ptr() for t in args + outs]
    assert _native.lib().pfrl_gru_cell_fwd(*ptr, N, inputs[0].shape[1], H, ops._stream()) == 0
    assert all(torch.equal(o.view(N, H), h1) for o in outs)
    assert int(torch.isnan(buf).sum()) == buf.numel() - 2 * N * H, "a guard row was written"
    err = float((h1.cpu().double() - want).abs().max())
    print("GRU cell %s f32_formulas_max_err %.3e kernel_max_err %.3e" % (name, yard, err))
    assert err <= 2 * yard + (1e-7 if name == "saturated" else 0), (name, err, yard)


@pytest.mark.parametrize("N,null_weight", [(0, False), (257, False), (4, True)], ids=["N=0", "N=257", "NULL-w_hh"])
def test_refusals_write_nothing(N, null_weight):
    buf = torch.full((4, 2048), float("nan"), device="cuda")
    p = buf.data_ptr()
    rc = _native.lib().pfrl_gru_cell_fwd(p, None, p, None if null_weight else p, None, None, p, p, N, 4, 4, ops._stream())
    assert rc != 0 and bool(torch.isnan(buf).all()) and (null_weight or not ops.gru_cell_supported(N, 4, 4))
