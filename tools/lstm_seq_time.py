"""Time of a packed sequence through an nn.LSTM member, forward + backward: the HIP route
(ops.lstm_sequence behind pfrl_amd.nn.recurrent.lstm_sequence_or_none, inside first_order_sequences)
against the library path (PFRL_LSTM_SEQ=0, nn.LSTM on the PackedSequence).  The method of
tools/lstm_step_time.py: both variants run in this process, alternated window by window, on a
RecurrentSequential holding only the LSTM; every shape is warmed up first; a window is a number of
passes between two device events, sized from a trial to last at least --window-ms.  One JSON line
per shape: mean, minimum and maximum of the windows in microseconds per pass, and the largest
difference of the two variants' outputs and input gradients.  The first shape is also timed as a
forward pass without gradients (the DRQN update's two target-side passes).

    python tools/lstm_seq_time.py                     # the table of DESIGN.md section 7
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/lstm_seq_time.py --kernel-only 50
                                                      # per-launch times (k_lstm_seq_step_* rows)
"""
import argparse
import json
import os
import sys

import torch
from torch import nn
from torch.nn.utils.rnn import PackedSequence

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import pfrl_amd  # noqa: E402
from pfrl_amd.nn.recurrent import first_order_sequences  # noqa: E402

RAGGED = [32, 29, 26, 23, 20, 16, 13, 10, 7, 4]
SHAPES = [("drqn", [32] * 10, 3136, 512, True), ("drqn-no-grad", [32] * 10, 3136, 512, False),
          ("ragged", RAGGED, 3136, 512, True), ("ppo-test", [4] * 10, 32, 16, True)]


def run_passes(net, packed, passes, variant, grad):
    os.environ["PFRL_LSTM_SEQ"] = variant
    x = packed.data
    for _ in range(passes):
        with first_order_sequences(), torch.set_grad_enabled(grad):
            y, _ = net(packed, None)
        if grad:
            x.grad = None
            net.zero_grad(set_to_none=True)
            y.data.sum().backward()
    return y.data.detach(), (x.grad if grad else None)


def window_us(net, packed, passes, variant, grad):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    run_passes(net, packed, passes, variant, grad)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / passes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--kernel-only", type=int, default=0, metavar="PASSES",
                    help="run PASSES passes of the HIP route per shape and nothing else (for a kernel trace)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    cases = []
    for name, sizes, I, H, grad in SHAPES:
        torch.manual_seed(0)
        net = pfrl_amd.nn.RecurrentSequential(nn.LSTM(I, H)).cuda()
        packed = PackedSequence(torch.randn(sum(sizes), I, device="cuda", requires_grad=grad), torch.tensor(sizes))
        outs = {v: run_passes(net, packed, 10, v, grad) for v in ("1", "0")}      # warm-up, and the outputs
        cases.append((name, sizes, I, H, grad, net, packed, outs))
    for name, sizes, I, H, grad, net, packed, outs in cases:
        if args.kernel_only:
            run_passes(net, packed, args.kernel_only, "1", grad)
            torch.cuda.synchronize()
            continue
        diff = [float((a - b).abs().max()) for a, b in zip(outs["1"], outs["0"]) if a is not None]
        passes = {v: max(10, int(args.window_ms * 1e3 / window_us(net, packed, 20, v, grad))) for v in ("1", "0")}
        times = {"1": [], "0": []}
        for _ in range(args.windows):
            for v in ("1", "0"):
                times[v].append(window_us(net, packed, passes[v], v, grad))
        line = {"shape": name, "batch_sizes": sizes, "I": I, "H": H, "backward": grad, "max_abs_diff_y_dx": diff}
        for v, key in (("1", "hip"), ("0", "library")):
            t = times[v]
            line[key] = {"mean_us": sum(t) / len(t), "min_us": min(t), "max_us": max(t), "passes_per_window": passes[v]}
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
