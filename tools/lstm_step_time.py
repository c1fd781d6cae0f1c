"""Time of one acting step of an nn.LSTM member: the fused launch (pfrl_lstm_cell_fwd behind
pfrl_amd.nn.recurrent.lstm_cell_step_or_none) against the library path (PFRL_LSTM_CELL=0, nn.LSTM on
a one-step PackedSequence).  Both variants run in this process, alternated window by window, through
``one_step_forward`` on a RecurrentSequential holding only the LSTM: packing and state reshaping are
inside the timed step on both sides.  Every shape is warmed up; a window is STEPS steps between two
device events, sized from a trial to last at least --window-ms; the state is carried from step to
step as the agents carry it.  One JSON line per shape: mean, minimum and maximum of the windows in
microseconds per step, and the largest difference of the two variants' outputs on the timed inputs.

    python tools/lstm_step_time.py                    # the table of DESIGN.md section 7
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/lstm_step_time.py --kernel-only 200
                                                      # the kernel's own time (k_lstm_cell_fwd rows)
"""
import argparse
import json
import os
import sys

import torch
from torch import nn

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import pfrl_amd  # noqa: E402
from pfrl_amd.utils.recurrent import one_step_forward  # noqa: E402

SHAPES = [(32, 3136, 512), (4, 3136, 512), (128, 3136, 512), (4, 32, 16)]     # (N, I, H)
HBM_PEAK = 8e12                                                               # bytes / s, MI355X


def run_steps(net, x, steps, variant):
    os.environ["PFRL_LSTM_CELL"] = variant
    state = None
    with torch.no_grad():
        for _ in range(steps):
            y, state = one_step_forward(net, x, state)
    return y, state


def window_us(net, x, steps, variant):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    run_steps(net, x, steps, variant)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--kernel-only", type=int, default=0, metavar="STEPS",
                    help="run STEPS fused steps per shape and nothing else (for a kernel trace)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    for N, I, H in SHAPES:
        torch.manual_seed(0)
        net = pfrl_amd.nn.RecurrentSequential(nn.LSTM(I, H)).cuda()
        x = torch.randn(N, I, device="cuda")
        if args.kernel_only:
            run_steps(net, x, args.kernel_only, "1")
            torch.cuda.synchronize()
            continue
        outs = {v: run_steps(net, x, 20, v) for v in ("1", "0")}                 # warm-up, and the outputs
        diff = max(float((a - b).abs().max()) for a, b in
                   zip([outs["1"][0], *outs["1"][1][0]], [outs["0"][0], *outs["0"][1][0]]))
        steps = {v: max(20, int(args.window_ms * 1e3 / window_us(net, x, 50, v))) for v in ("1", "0")}
        times = {"1": [], "0": []}
        for _ in range(args.windows):
            for v in ("1", "0"):
                times[v].append(window_us(net, x, steps[v], v))
        line = {"N": N, "I": I, "H": H, "weight_bytes": 16 * H * (I + H), "max_abs_diff_of_outputs": diff}
        for v, name in (("1", "fused"), ("0", "library")):
            t = times[v]
            line[name] = {"mean_us": sum(t) / len(t), "min_us": min(t), "max_us": max(t), "steps_per_window": steps[v]}
        line["weights_at_hbm_peak_us"] = line["weight_bytes"] / HBM_PEAK * 1e6
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
