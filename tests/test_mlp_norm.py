"""The normalised-input loaders of the whole-MLP launches (pfrl_mlp_fwd_norm / pfrl_mlp_bwd_norm, csrc/mlp.hip):
``ops.mlp_fused(raw, ..., in_norm=n)`` against ``ops.mlp_fused(n(raw, update=False), ...)`` BIT FOR BIT -- subtract,
multiply and clamp are exact, and the in-kernel scale is shown here to be torch's ``(var + eps) ** -0.5`` on this device
-- then the containers' fall-backs and the agents."""
import numpy as np
import pytest
import torch

from pfrl_amd import ops
from pfrl_amd.nn import EmpiricalNormalization
from pfrl_amd.nn.mfma_linear import _fuse_small_mlps

pytestmark = pytest.mark.gpu
# (M, in_features, [widths per network], activation, clip): every M and K0 edge of the two tile programs and of the
# 64-column chunks once; 1 to 3 layers, one and two networks, both activations, with and without the clamp
TABLE = [(1, 1, [[1]], "tanh", 5), (16, 3, [[16, 6]], "relu", None), (17, 63, [[64, 64, 6], [64, 17, 1]], "tanh", 5),
         (64, 64, [[17, 64, 32]], "relu", 5), (65, 65, [[64, 1], [16, 6]], "tanh", None),
         (513, 130, [[64, 64, 6], [64, 64, 1]], "tanh", 5), (65, 512, [[33]], "relu", 5)]


def normalizer(D, clip, seed, var=None):
    g = torch.Generator().manual_seed(seed)
    n = EmpiricalNormalization(D, clip_threshold=clip).cuda()
    n._mean.copy_(3 * torch.randn(1, D, generator=g))
    n._var.copy_(torch.exp(4 * torch.randn(1, D, generator=g)) if var is None else var.view(1, D))
    return n


def raw_batch(n, M, seed):      # a few deviations round the mean: some beyond the clamp, most inside
    z = torch.randn(M, n._mean.shape[1], generator=torch.Generator().manual_seed(seed)).cuda()
    return (n._mean + 3 * z * n._var.sqrt()).contiguous()


def networks(K0, widths, seed, dtype=torch.float32, device="cuda"):
    g, nets = torch.Generator().manual_seed(seed), []
    for ws in widths:
        shapes = [((w, k), (w,)) for w, k in zip(ws, [K0] + ws[:-1])]
        nets.append([tuple((torch.randn(s, generator=g) / shape[0][1] ** 0.5).to(device, dtype).requires_grad_()
                           for s in shape) for shape in shapes])
    return nets


def test_the_loaders_scale_is_torchs_bit_for_bit():
    """9 x 512 values of var + eps from 1e-2 (var = 0) through 1 to 1e6, seen through identity weights that pick 64
    columns at a time: y is then the normalised tile itself."""
    for i in range(9):
        g = torch.Generator().manual_seed(i)
        var = torch.exp(torch.empty(512).uniform_(np.log(1e-4), np.log(1e6), generator=g))
        if i == 0:
            var[:3] = torch.tensor([0.0, 1.0, 1e6]) - torch.tensor([0.0, 1e-2, 1e-2])
        n = normalizer(512, 5 if i % 2 else None, 100 + i, var=var)
        x = raw_batch(n, 16, 200 + i)
        want = n(x, update=False)
        for j in range(8):
            w = torch.zeros(64, 512, device="cuda")
            w[:, 64 * j:64 * j + 64] = torch.eye(64)
            y = ops.mlp_fused(x, [(w, torch.zeros(64, device="cuda"))], "tanh", in_norm=n)
            assert torch.equal(y, want[:, 64 * j:64 * j + 64]), (i, j)


@pytest.mark.parametrize("small_m", [0, 65536])     # every M on the 64-row program / on the 16-row program
@pytest.mark.parametrize("i", range(len(TABLE)))
def test_forward_saves_and_gradients_bit_for_bit(i, small_m):
    M, K0, widths, act, clip = TABLE[i]
    n, nets = normalizer(K0, clip, 10 + i), networks(K0, widths, 30 + i)
    x = raw_batch(n, M, 20 + i)
    params = [t for net in nets for wb in net for t in wb]
    layers, acts = (nets[0], act) if len(nets) == 1 else (nets, (act,) * len(nets))
    outs = []
    for fused in (True, False):
        y = (ops.mlp_fused(x, layers, acts, small_m, in_norm=n) if fused
             else ops.mlp_fused(n(x, update=False), layers, acts, small_m))
        ys = (y,) if len(nets) == 1 else y
        saves = ys[0].grad_fn.saved_tensors[1 + len(params):]
        g = torch.Generator().manual_seed(40 + i)
        dys = [torch.randn(t.shape, generator=g).cuda() for t in ys]
        outs.append((ys, saves, torch.autograd.grad(ys, params, dys)))
    for kind, a, b in zip(("y", "save", "grad"), *outs):
        assert len(a) == len(b) and len(a) >= (kind != "save")
        assert all(not torch.isnan(u).any() and torch.equal(u, v) for u, v in zip(a, b)), kind
    if i == 5:      # (and y is right, not only equal: the rule of tests/test_mlp_fused.py against float64)
        ref = {}
        for dtype in (torch.float64, torch.float32):
            h = ((x.cpu().to(dtype) - n._mean.cpu().to(dtype)) * (n._var.cpu().to(dtype) + float(n.eps)) ** -0.5
                 ).clamp(-clip, clip)
            for w, b in networks(K0, widths, 30 + i, dtype, "cpu")[0]:
                h = h @ w.t() + b
                h = torch.tanh(h) if w.shape[0] == 64 else h
            ref[dtype] = h.detach().double()
        kernel = (outs[0][0][0].detach().double().cpu() - ref[torch.float64]).abs().max().item()
        torch32 = (ref[torch.float32] - ref[torch.float64]).abs().max().item()
        print("y: kernel %.3e, torch float32 %.3e" % (kernel, torch32))
        assert kernel <= 2 * torch32


@pytest.mark.parametrize("case", ["requires_grad", "float64", "batch_axis", "subclass"])
def test_what_the_loader_refuses_is_normalised_in_front(case):
    D = 11
    seq = torch.nn.Sequential(torch.nn.Linear(D, 64), torch.nn.Tanh(), torch.nn.Linear(64, 3)).cuda()
    layers = [(seq[0].weight, seq[0].bias), (seq[2].weight, seq[2].bias)]
    _fuse_small_mlps(seq)
    n = {"float64": lambda: EmpiricalNormalization(D, dtype=np.float64, clip_threshold=5),
         "batch_axis": lambda: EmpiricalNormalization(D, batch_axis=1),
         "subclass": lambda: type("Sub", (EmpiricalNormalization,), {})(D, clip_threshold=5),
         "requires_grad": lambda: EmpiricalNormalization(D)}[case]().cuda()
    n._mean.add_(0.5)
    x = torch.randn(9, D, device="cuda", requires_grad=case == "requires_grad")
    assert ops.mlp_fused_supported(x, layers, "tanh") and not ops.mlp_fused_supported(x, layers, "tanh", in_norm=n)
    assert ops.mlp_fused_supported(x.detach(), layers, "tanh", in_norm=EmpiricalNormalization(D).cuda())
    if case in ("requires_grad", "subclass"):
        assert torch.equal(seq.forward_normalized(x, n), seq(n(x, update=False)))


def run_agent(kind, monkeypatch):
    """(agent, actions, parameters) after two updates on the synthetic vector env, by the agents' own tests' loops."""
    if kind == "ppo":
        from test_ppo_gaussian import _run_two_rollouts
        ag, actions, _, params, _ = _run_two_rollouts(monkeypatch, switches_off=False)
        return ag, actions, params
    from test_trpo import _device_run, _flat
    ag, actions, _ = _device_run(True, updates=2)
    return ag, actions, np.concatenate([_flat(ag.policy.parameters()), _flat(ag.vf.parameters())])


@pytest.mark.parametrize("kind", ["ppo", "trpo"])
def test_agents_with_the_loader_on_against_off(monkeypatch, kind):
    """The same actions, parameters and statistics, bit for bit; and the loader did run."""
    monkeypatch.setenv("PFRL_OBS_STATS_KERNEL", "0")
    calls, orig, got = [], ops.mlp_fused, {}
    monkeypatch.setattr(ops, "mlp_fused",
                        lambda *a, **kw: (calls.append(kw.get("in_norm") is not None), orig(*a, **kw))[1])
    for switch in ("1", "0"):
        monkeypatch.setenv("PFRL_OBS_NORM_LOADER", switch)
        del calls[:]
        ag, actions, params = run_agent(kind, monkeypatch)
        n = ag.obs_normalizer
        got[switch] = (actions, params, n._mean.cpu().numpy(), n._var.cpu().numpy(), int(n.count))
        assert calls and any(calls) == (switch == "1")
    for a, b in zip(got["1"], got["0"]):
        np.testing.assert_array_equal(a, b)


def test_statistics_overwritten_in_place_are_honoured_by_the_next_acting_step(monkeypatch):
    """The stale-cache case: the captured acting step reads ``_var`` itself, not the module's cached inverse."""
    from pfrl_amd.envs.synthetic import HostSyntheticVectorObsEnv
    from test_ppo_gaussian_cpu import ACT, OBS
    ag, _, _ = run_agent("ppo", monkeypatch)
    n = ag.obs_normalizer
    n(torch.zeros(1, OBS, device="cuda"), update=False)         # (the cache is filled with the old statistics)
    n._var.copy_(4 * n._var + 1)
    obs = HostSyntheticVectorObsEnv(4, obs_dim=OBS, act_dim=ACT, seed=9, p_done=0.02).reset()
    ag.batch_act(obs)
    x = torch.as_tensor(np.asarray(obs, dtype=np.float32)).cuda()
    with torch.no_grad():
        want = ag.model(((x - n._mean) * (n._var + n.eps) ** -0.5).clamp(-5, 5))[1].reshape(-1)
    np.testing.assert_array_equal(ag.value_record.values()[-4:], want.cpu().numpy())
