"""Time of a 64-64 MLP (the policy / value networks of the on-policy continuous-control agents), whole-MLP HIP route
against the per-layer library path, in one process on the same inputs.

The method of tools/gru_time.py: both variants are warmed up, they alternate window by window, a window is a number of calls
between two device events sized from a trial to last at least --window-ms.  One JSON line per shape: mean, minimum and maximum
of the windows in microseconds per call for both variants, and the largest difference of their results.

    python tools/mlp_time.py                     # forward alone (no_grad) and forward + backward
    python tools/mlp_time.py --pair              # policy and value function as a Branched (one launch for both)
    python tools/mlp_time.py --wide              # the wide route (csrc/mlp_wide.hip) against the per-layer launches,
                                                 # PFRL_MLP_WIDE=1 against 0, each as replays of a captured graph
    python tools/mlp_time.py --fvp               # TRPO's Fisher-vector product: ops.gaussian_mlp_fisher (three or four
                                                 # launches) against autograd's double backward, us per product
    python tools/mlp_time.py --norm              # an observation normaliser in front of the policy / value pair:
                                                 # normalised in the launch's loader (PFRL_OBS_NORM_LOADER=1) against
                                                 # the torch expressions in front of it (0, the launches of the parent
                                                 # commit), as replays of a captured graph; then ``experience``,
                                                 # kernel route against module route
"""
import argparse
import copy
import json
import os
import sys

import torch
from torch import nn

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import pfrl_amd  # noqa: E402,F401
from pfrl_amd.nn import Branched, accelerate_mlp  # noqa: E402


def make(obs, out, act, pair):
    net = lambda o: nn.Sequential(nn.Linear(obs, 64), act(), nn.Linear(64, 64), act(), nn.Linear(64, o))  # noqa: E731
    return Branched(net(out), net(1)) if pair else net(out)


def call(model, x, backward):
    if not backward:
        with torch.no_grad():
            return model(x)
    y = model(x)
    y = y if torch.is_tensor(y) else torch.cat(y, dim=1)
    model.zero_grad()
    y.sum().backward()
    return y


def window(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


def wide_cases():
    """(name, rows, fn): fn() runs the pass once; the route is chosen by PFRL_MLP_WIDE when fn is called."""
    from pfrl_amd.nn import ConcatObsAndAction
    from pfrl_amd.nn.twin_mlp import twin_forward

    def mlp(i, h1, h2, o, concat=False):
        head = [ConcatObsAndAction()] if concat else []
        return accelerate_mlp(nn.Sequential(*head, nn.Linear(i, h1), nn.ReLU(), nn.Linear(h1, h2), nn.ReLU(),
                                            nn.Linear(h2, o)).cuda())

    def single(net, x):
        def fn():
            with torch.no_grad():
                return net(x)
        return fn

    def twin(q1, q2, obs, action, frozen):
        for p in list(q1.parameters()) + list(q2.parameters()):
            p.requires_grad_(False)
        a = action.clone().requires_grad_(frozen)

        def fn():
            if not frozen:
                with torch.no_grad():
                    return torch.cat(twin_forward(q1, q2, (obs, a)), 1)
            ya, yb = twin_forward(q1, q2, (obs, a))
            return torch.autograd.grad((ya + yb).sum(), a)[0]
        return fn

    torch.manual_seed(0)
    cases = []
    for rows in (256, 512):
        obs, action = torch.randn(rows, 376, device="cuda"), torch.randn(rows, 17, device="cuda")
        q1, q2 = mlp(393, 256, 256, 1, True), mlp(393, 256, 256, 1, True)
        cases += [("twin 393-256-256-1 forward", rows, twin(q1, q2, obs, action, False)),
                  ("twin 393-256-256-1 forward + frozen backward", rows, twin(q1, q2, obs, action, True))]
    for rows in (64, 256):
        x = torch.randn(rows, 376, device="cuda")
        cases += [("single 376-256-256-34 forward", rows, single(mlp(376, 256, 256, 34), x)),
                  ("single 376-400-300-17 forward", rows, single(mlp(376, 400, 300, 17), x))]
    return cases


def wide_main(args):
    """Route on against route off, each captured once (20 calls a graph) and timed as alternating windows of replays."""
    from pfrl_amd.agents import _capture

    class Holder:
        pool = None

    for name, rows, fn in wide_cases():
        graphs, outs = {}, {}
        for k, env in (("route", "1"), ("per_layer", "0")):
            os.environ["PFRL_MLP_WIDE"] = env
            outs[k] = fn().clone()
            _capture.warm_up("cuda", lambda i: fn())
            graphs[k] = _capture.capture(Holder, lambda: [fn() for _ in range(20)])[0]
        os.environ.pop("PFRL_MLP_WIDE")
        diff = float((outs["route"] - outs["per_layer"]).abs().max())
        fns = {k: g.replay for k, g in graphs.items()}
        for f in fns.values():
            window(f, 20)
        calls = {k: max(5, int(args.window_ms * 1e3 / (20 * window(f, 20)))) for k, f in fns.items()}
        times = {k: [] for k in fns}
        for _ in range(args.windows):
            for k, f in fns.items():
                times[k].append(window(f, calls[k]) / 20)
        rec = dict(case=name, rows=rows, max_abs_diff=diff)
        for k, v in times.items():
            rec[k + "_us"] = dict(mean=sum(v) / len(v), min=min(v), max=max(v))
        print(json.dumps(rec), flush=True)


FVP_SHAPES = [(2048, 11, 3), (5000, 11, 3), (5000, 17, 6), (5000, 376, 17)]      # (rows, obs, A)


def fvp_main(args):
    """One damped product on a 64-64 tanh Gaussian policy (diagonal covariance, as train_trpo.py): the launches of
    ops.gaussian_mlp_fisher against ``_hessian_vector_product`` on a KL graph built once, alternating windows."""
    from pfrl_amd import ops
    from pfrl_amd.agents import trpo

    for rows, obs, A in FVP_SHAPES:
        torch.manual_seed(0)
        head = pfrl_amd.policies.GaussianHeadWithStateIndependentCovariance(
            action_size=A, var_type="diagonal", var_func=lambda v: torch.exp(2 * v), var_param_init=0)
        policy = nn.Sequential(*make(obs, A, nn.Tanh, False), head).cuda()
        params = list(policy.parameters())
        x = torch.randn(rows, obs, device="cuda")
        vec = torch.randn(sum(p.numel() for p in params), device="cuda")
        saved_cap, ops.FISHER_MAX_INPUT = ops.FISHER_MAX_INPUT, 1 << 62       # (time the shapes the cap may refuse too)
        fused = ops.gaussian_mlp_fisher(policy, x, 0.01)
        ops.FISHER_MAX_INPUT = saved_cap
        with torch.no_grad():
            old = policy(x)
        kl = torch.mean(torch.distributions.kl_divergence(old, policy(x)))
        flat = trpo._flat_grads([kl], params, create_graph=True)
        fns = {"route": lambda: fused(vec),
               "double_backward": lambda: trpo._hessian_vector_product(flat, params, vec) + 0.01 * vec}
        outs = {k: f().clone() for k, f in fns.items()}
        diff = float((outs["route"] - outs["double_backward"]).abs().max())
        for f in fns.values():
            window(f, 20)
        calls = {k: max(5, int(args.window_ms * 1e3 / window(f, 20))) for k, f in fns.items()}
        times = {k: [] for k in fns}
        for _ in range(args.windows):
            for k, f in fns.items():
                times[k].append(window(f, calls[k]))
        rec = dict(rows=rows, obs=obs, A=A, max_abs_diff=diff, max_abs=float(outs["double_backward"].abs().max()))
        for k, v in times.items():
            rec[k + "_us"] = dict(mean=sum(v) / len(v), min=min(v), max=max(v))
        print(json.dumps(rec), flush=True)


def alternate(fns, args, per_call=1):
    """{name: mean / min / max us per call} of alternating windows."""
    for f in fns.values():
        window(f, 20)
    calls = {k: max(5, int(args.window_ms * 1e3 / (per_call * window(f, 20)))) for k, f in fns.items()}
    times = {k: [] for k in fns}
    for _ in range(args.windows):
        for k, f in fns.items():
            times[k].append(window(f, calls[k]) / per_call)
    return {k + "_us": dict(mean=sum(v) / len(v), min=min(v), max=max(v)) for k, v in times.items()}


def norm_main(args):
    """The acting step behind the gather (normaliser + policy / value pair, no_grad) as replays of a captured graph of 20
    steps, loader on against off; then ``EmpiricalNormalization.experience`` eagerly, kernel route against module route."""
    from pfrl_amd.agents import _capture
    from pfrl_amd.nn import EmpiricalNormalization
    from pfrl_amd.nn.mfma_linear import _fuse_small_mlps

    class Holder:
        pool = None

    for obs in (11, 376):
        torch.manual_seed(0)
        model = _fuse_small_mlps(make(obs, 6, nn.Tanh, True).cuda())
        n = EmpiricalNormalization(obs, clip_threshold=5).cuda()
        n.experience(3 + 2 * torch.randn(4096, obs, device="cuda"))
        for rows in (1, 64, 2048):
            x = 3 + 2 * torch.randn(rows, obs, device="cuda")

            def fn():
                with torch.no_grad():
                    return torch.cat(model.forward_normalized(x, n), 1)

            graphs, outs = {}, {}
            for k, env in (("loader", "1"), ("in_front", "0")):
                os.environ["PFRL_OBS_NORM_LOADER"] = env
                outs[k] = fn().clone()
                _capture.warm_up("cuda", lambda i: fn())
                graphs[k] = _capture.capture(Holder, lambda: [fn() for _ in range(20)])[0]
            os.environ.pop("PFRL_OBS_NORM_LOADER")
            rec = dict(case="acting step", obs=obs, rows=rows, equal=bool(torch.equal(outs["loader"], outs["in_front"])))
            rec.update(alternate({k: g.replay for k, g in graphs.items()}, args, per_call=20))
            print(json.dumps(rec), flush=True)
    for obs in (11, 376):
        x = 3 + 2 * torch.randn(2048, obs, device="cuda")
        mods = {k: EmpiricalNormalization(obs).cuda() for k in ("kernel", "module")}

        def learn(k):
            os.environ["PFRL_OBS_STATS_KERNEL"] = "1" if k == "kernel" else "0"
            mods[k].experience(x)

        rec = dict(case="experience", obs=obs, rows=2048)
        rec.update(alternate({k: (lambda k=k: learn(k)) for k in mods}, args))
        os.environ.pop("PFRL_OBS_STATS_KERNEL")
        print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1, 64, 2048, 16384])
    ap.add_argument("--obs", type=int, nargs="+", default=[11, 376])
    ap.add_argument("--relu", action="store_true")
    ap.add_argument("--pair", action="store_true")
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--window-ms", type=float, default=20.0)
    ap.add_argument("--wide", action="store_true")
    ap.add_argument("--fvp", action="store_true")
    ap.add_argument("--norm", action="store_true")
    args = ap.parse_args()
    if args.norm:
        return norm_main(args)
    if args.wide:
        return wide_main(args)
    if args.fvp:
        return fvp_main(args)
    act = nn.ReLU if args.relu else nn.Tanh
    for obs in args.obs:
        torch.manual_seed(0)
        base = make(obs, 6, act, args.pair).cuda()
        off = copy.deepcopy(base)                   # (plain containers: the library's launches)
        on = accelerate_mlp(copy.deepcopy(base))
        for rows in args.rows:
            x = torch.randn(rows, obs, device="cuda")
            for backward in (False, True):
                fns = {"route": lambda: call(on, x, backward), "library": lambda: call(off, x, backward)}
                outs = {k: f() for k, f in fns.items()}
                cat = lambda y: y if torch.is_tensor(y) else torch.cat(y, dim=1)     # noqa: E731
                diff = float((cat(outs["route"]) - cat(outs["library"])).abs().max())
                for f in fns.values():
                    window(f, 20)
                calls = {k: max(5, int(args.window_ms * 1e3 / window(f, 20))) for k, f in fns.items()}
                times = {k: [] for k in fns}
                for _ in range(args.windows):
                    for k, f in fns.items():
                        times[k].append(window(f, calls[k]))
                rec = dict(obs=obs, rows=rows, pair=args.pair, backward=backward, max_abs_diff=diff)
                for k, v in times.items():
                    rec[k + "_us"] = dict(mean=sum(v) / len(v), min=min(v), max=max(v))
                print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
