"""Time of IQN's threshold embedding head, HIP route (ops.iqn_embed, csrc/iqn_embed.hip) against the torch statements
it replaces (PFRL_IQN_EMBED=0), in one process on the same inputs.

What is timed is agents.iqn._quantile_head with an identity ``f``: the cosine embedding, its Linear(n, H), the ReLU and the
product with psi_x, for psi_x (B, H) and taus (B, N), n = 64 and H = 3136 as in examples/train_iqn_batch_synthetic.py:
the forward alone (no gradient) at the rows of the target pass at taus~ (32, 32), of the passes at taus / taus' (32, 64)
and of an acting step of 256 envs (256, 32), and forward plus backward at (32, 64), the online pass of an update.

The method of tools/gru_time.py: every shape is warmed up, the two variants alternate window by window, a window is a
number of calls between two device events sized from a trial to last at least --window-ms.  One JSON line per shape:
mean, minimum and maximum of the windows in microseconds per call and the largest difference of the two variants' results.

    python tools/iqn_embed_time.py                      # the table of DESIGN.md section 7
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/iqn_embed_time.py --kernel-only 200
                                                        # launches per evaluation, both variants (200 calls each)
"""
import argparse
import json
import os
import sys

import torch
from torch import nn

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from pfrl_amd.agents import iqn  # noqa: E402

N_BASIS, HIDDEN = 64, 3136
SHAPES = [(32, 64, False), (32, 32, False), (256, 32, False), (32, 64, True)]     # (B, N, backward)


class _Rows(nn.Module):
    """``f``: hands the head's rows back (QuantileDiscreteActionValue only keeps them)."""

    def forward(self, x):
        return x


def run(phi, psi_x, taus, calls, variant, grad):
    os.environ["PFRL_IQN_EMBED"] = variant
    f = _Rows()
    for _ in range(calls):
        with torch.set_grad_enabled(grad):
            out = iqn._quantile_head(psi_x, phi, f)(taus).quantiles
        if grad:
            psi_x.grad = None
            phi.zero_grad(set_to_none=True)
            out.sum().backward()
    lin = phi[0].linear
    return [out.detach()] + ([psi_x.grad, lin.weight.grad, lin.bias.grad] if grad else [])


def window_us(*a):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    run(*a)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / a[3]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--kernel-only", type=int, default=0, metavar="CALLS",
                    help="run CALLS calls of each variant per shape and nothing else (for a kernel trace)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    for B, N, grad in SHAPES:
        torch.manual_seed(0)
        phi = nn.Sequential(iqn.CosineBasisLinear(N_BASIS, HIDDEN), nn.ReLU()).cuda()
        psi_x = torch.randn(B, HIDDEN, device="cuda", requires_grad=grad)
        taus = torch.rand(B, N, device="cuda")
        if args.kernel_only:
            for v in ("1", "0"):
                run(phi, psi_x, taus, args.kernel_only, v, grad)
            torch.cuda.synchronize()
            continue
        line = {"B": B, "N": N, "rows": B * N, "n": N_BASIS, "H": HIDDEN, "backward": grad}
        outs = {v: run(phi, psi_x, taus, 10, v, grad) for v in ("1", "0")}      # warm-up, and the results
        line["max_abs_diff"] = [float((a - b).abs().max()) for a, b in zip(outs["1"], outs["0"])]
        calls = {v: max(10, int(args.window_ms * 1e3 / window_us(phi, psi_x, taus, 20, v, grad))) for v in ("1", "0")}
        times = {"1": [], "0": []}
        for _ in range(args.windows):
            for v in ("1", "0"):
                times[v].append(window_us(phi, psi_x, taus, calls[v], v, grad))
        for v, key in (("1", "hip"), ("0", "composite")):
            t = times[v]
            line[key] = {"mean_us": sum(t) / len(t), "min_us": min(t), "max_us": max(t), "calls_per_window": calls[v]}
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
