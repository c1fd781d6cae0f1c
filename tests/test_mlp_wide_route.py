"""The wide whole-MLP route (ops.mlp_wide_fwd / mlp_wide_dx) as the agents reach it: ``twin_forward`` on an
``accelerate_mlp``-ed pair of critics and a no-grad ``Sequential``; ``PFRL_MLP_WIDE=0`` is today's launches."""
import copy

import pytest
import torch
from torch import nn

from pfrl_amd import _native
from pfrl_amd.agents import _capture
from pfrl_amd.nn import ConcatObsAndAction, accelerate_mlp
from pfrl_amd.nn.twin_mlp import twin_forward
from tests.test_a2c_agent import _RecordingLib

pytestmark = pytest.mark.gpu
FWD, DX, TWIN = "pfrl_mlp_wide_fwd", "pfrl_mlp_wide_dx", "pfrl_linear_fwd_twin"
TOL = 2e-5          # tests/test_mfma_linear.py::test_twin_q_networks_match_the_two_modules


@pytest.fixture
def recorder(monkeypatch):
    if not _native.available():
        _native.build()
    rec = _RecordingLib(_native.lib())
    monkeypatch.setattr(_native, "_lib", rec)
    return rec


def critics(h1, h2, obs=23, act=6):
    torch.manual_seed(3)
    q = lambda: accelerate_mlp(nn.Sequential(ConcatObsAndAction(), nn.Linear(obs + act, h1), nn.ReLU(), nn.Linear(h1, h2),  # noqa: E731
                                             nn.ReLU(), nn.Linear(h2, 1)).cuda())
    return q(), q(), torch.randn(37, obs, device="cuda"), torch.randn(37, act, device="cuda")


def run(q1, q2, obs, action, monkeypatch, wide, frozen):
    """(values, action gradient, parameter gradients) of (q1 + 2 q2).sum() through ``twin_forward``."""
    monkeypatch.setenv("PFRL_MLP_WIDE", "1" if wide else "0")
    params = list(q1.parameters()) + list(q2.parameters())
    for p in params:
        p.requires_grad_(not frozen)
        p.grad = None
    a = action.clone().requires_grad_()
    ya, yb = twin_forward(q1, q2, (obs, a))
    (ya + 2 * yb).sum().backward()
    return [ya.detach(), yb.detach()], a.grad, [p.grad for p in params]


def close(got, ref):
    return bool(((got - ref).abs() <= TOL * ref.abs().clamp(min=1.0)).all())


@pytest.mark.parametrize("frozen", [False, True])
def test_twin_critics_take_one_launch_and_match_the_per_layer_route(recorder, monkeypatch, frozen):
    q1, q2, obs, action = critics(96, 128)
    ref = run(q1, q2, obs, action, monkeypatch, False, frozen)
    assert recorder.count(TWIN) == 2 and recorder.count(FWD) == recorder.count(DX) == 0
    del recorder.calls[:]
    got = run(q1, q2, obs, action, monkeypatch, True, frozen)
    assert recorder.count(FWD) == 1 and recorder.count(TWIN) == 0 and recorder.count(DX) == (1 if frozen else 0)
    assert not frozen or [c for c in recorder.calls if c.startswith("pfrl_")] == [FWD, DX]
    assert all(close(g, r) for g, r in zip(got[0], ref[0])) and close(got[1], ref[1])
    assert all((g is None and r is None) or close(g, r) for g, r in zip(got[2], ref[2]))


def test_narrow_critics_keep_their_launches(recorder, monkeypatch):
    q1, q2, obs, action = critics(32, 32)
    run(q1, q2, obs, action, monkeypatch, True, True)
    assert recorder.count(FWD) == recorder.count(DX) == 0 and recorder.count(TWIN) == 2


def test_single_network_is_one_launch_without_gradients_only(recorder, monkeypatch):
    monkeypatch.setenv("PFRL_MLP_WIDE", "1")
    torch.manual_seed(5)
    plain = nn.Sequential(nn.Linear(23, 96), nn.ReLU(), nn.Linear(96, 128), nn.ReLU(), nn.Linear(128, 12)).cuda()
    net, x = accelerate_mlp(copy.deepcopy(plain)), torch.randn(37, 23, device="cuda")
    with torch.no_grad():
        y, ref = net(x), plain(x)
    assert recorder.count(FWD) == 1 and [c for c in recorder.calls if c.startswith("pfrl_")] == [FWD]
    assert close(y, ref)
    net(x).sum().backward()
    assert recorder.count(FWD) == 1


def test_captured_twin_forward_replays_the_eager_bits(monkeypatch):
    monkeypatch.setenv("PFRL_MLP_WIDE", "1")
    q1, q2, obs, action = critics(96, 128)
    holder = type("Holder", (), {"pool": None})

    with torch.no_grad():
        eager = twin_forward(q1, q2, (obs, action))
        _capture.warm_up(obs.device, lambda i: twin_forward(q1, q2, (obs, action)))
        g, out = _capture.capture(holder, lambda: twin_forward(q1, q2, (obs, action)))
    for _ in range(2):
        out[0].zero_(), out[1].zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[0], eager[0]) and torch.equal(out[1], eager[1])
