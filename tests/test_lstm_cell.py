"""pfrl_lstm_cell_fwd (csrc/lstm.hip) against the float64 formulas.  Yardstick per case and output: the maximum error of
torch.nn.LSTM in float32 on the CPU against the same float64 result; the kernel may err twice as much (+ 1e-7 where gates
saturate and the yardstick can be exactly 0).  The ids name the edge of the split: MT = 1 / 2 / 4 M-tiles of 16 rows, 64 rows
per workgroup, 256 at most, U = 4 units, 16-byte loads iff I % 4 == H % 4 == 0, 16 waves in trips of 4 blocks (MT = 4: 2)."""
import pytest
import torch

from pfrl_amd import _native, ops

pytestmark = pytest.mark.gpu
CASES = {   # id: (N, I, H[, state given, bias, scale of x])
    "N1-H20": (1, 5, 20), "N15-I3-H3=U-1": (15, 3, 3), "N16-I4-H4=U-vector-loads": (16, 4, 4),
    "N17-MT2-I5-H5=U+1": (17, 5, 5), "N32-MT2-full-H16": (32, 64, 16), "N33-MT4-I1-H1": (33, 1, 1),
    "N64-one-workgroup-I36-vector-tail-H20": (64, 36, 20), "N65-second-grid-row": (65, 7, 6),
    "N256-envelope-maximum": (256, 24, 8), "waves-take-5-or-6-blocks-tail-7-scalar": (17, 1367, 20),
    "waves-take-5-or-6-blocks-vector-MT4": (40, 1376, 32), "no-state-vector": (16, 64, 16, False),
    "no-state-scalar": (17, 5, 5, False), "no-bias": (17, 36, 20, True, False),
    "saturated": (32, 64, 16, True, True, 20), "workload-N32-I3136-H512": (32, 3136, 512)}


def _case(name):   # inputs (f32, CPU), the float64 (h1, c1), the yardstick's maximum errors
    N, I, H, state, bias, scale = CASES[name] + (True, True, 1)[len(CASES[name]) - 3:]
    g = torch.Generator().manual_seed(sorted(CASES).index(name))
    w_ih, w_hh, b_ih, b_hh = ((torch.rand(s, generator=g) * 2 - 1) / H ** 0.5 for s in ((4 * H, I), (4 * H, H), (4 * H,), (4 * H,)))
    x, h0, c0 = (torch.randn(s, generator=g) for s in ((N, I), (N, H), (N, H)))
    x, (h0, c0), (b_ih, b_hh) = x * scale, (h0, c0) if state else (None, None), (b_ih, b_hh) if bias else (None, None)
    d = [None if t is None else t.double() for t in (x, h0, c0, w_ih, w_hh, b_ih, b_hh)]
    gates = d[0] @ d[3].T + (d[1] @ d[4].T if state else 0) + (d[5] + d[6] if bias else 0)
    i, f, gg, o = gates.chunk(4, dim=1)
    c1 = torch.sigmoid(f) * (d[2] if state else 0) + torch.sigmoid(i) * torch.tanh(gg)
    want = (torch.sigmoid(o) * torch.tanh(c1), c1)
    lstm = torch.nn.LSTM(I, H, bias=bias)
    lstm.load_state_dict(dict(zip(lstm.state_dict(), (w_ih, w_hh, b_ih, b_hh))))
    with torch.no_grad():
        _, hc = lstm(x[None], (h0[None], c0[None]) if state else None)
    return (x, h0, c0, w_ih, w_hh, b_ih, b_hh), want, [float((a[0].double() - b).abs().max()) for a, b in zip(hc, want)]


@pytest.mark.parametrize("name", CASES)
def test_kernel_against_float64_twice_and_guarded(name):
    inputs, want, yard = _case(name)
    args = [None if t is None else t.cuda() for t in inputs]
    got = ops.lstm_cell_step(*args)
    assert all(torch.equal(a, b) for a, b in zip(got, ops.lstm_cell_step(*args))), "two launches differ"
    N, H = want[0].shape
    buf = torch.full((3, N + 2, H + 3), float("nan"), device="cuda")     # sentinel rows round h1, c1 and y
    outs = [b.view(-1)[H:H + N * H] for b in buf]
    ptr = [None if t is None else t.data_ptr() for t in args + outs]
    assert _native.lib().pfrl_lstm_cell_fwd(*ptr, N, inputs[0].shape[1], H, ops._stream()) == 0
    assert all(torch.equal(o.view(N, H), g) for o, g in zip(outs, (got[0], got[1], got[0])))
    assert int(torch.isnan(buf).sum()) == buf.numel() - 3 * N * H, "a guard row was written"
    for what, a, b, y in zip(("h1", "c1"), got, want, yard):
        err = float((a.cpu().double() - b).abs().max())
        print("LSTM %s %s torch_f32_max_err %.3e kernel_max_err %.3e" % (name, what, y, err))
        assert err <= 2 * y + (1e-7 if name == "saturated" else 0), (name, what, err, y)


@pytest.mark.parametrize("N,I,H", [(0, 4, 4), (257, 4, 4), (4, 0, 4), (4, 4, 0), (4, 2 ** 15, 2 ** 14)])
def test_refusals(N, I, H):
    buf = torch.full((4, 64), float("nan"), device="cuda")
    p = buf.data_ptr()
    rc = _native.lib().pfrl_lstm_cell_fwd(p, None, None, p, p, None, None, p, p, p, N, I, H, ops._stream())
    assert rc != 0 and not ops.lstm_cell_supported(N, I, H) and bool(torch.isnan(buf).all())
    x, _, _, *w = (t.cuda() for t in _case("N16-I4-H4=U-vector-loads")[0])
    for bad in (x.double(), x.repeat(1, 2)[:, ::2]):     # the front end asserts before it allocates or launches
        with pytest.raises(AssertionError):
            ops.lstm_cell_step(bad, None, None, *w)
