"""Time of an nn.GRU member of a RecurrentSequential, HIP route against library path, in one process on the same inputs.

  --mode step   one acting step: pfrl_gru_cell_fwd behind nn.recurrent.gru_cell_step_or_none against PFRL_GRU_CELL=0 (nn.GRU
                on a one-step PackedSequence), through ``one_step_forward`` with the state carried from step to step
  --mode seq    a packed sequence, forward + backward (and the first shape again as a no-grad forward): ops.gru_sequence
                behind gru_sequence_or_none inside first_order_sequences against PFRL_GRU_SEQ=0

The method of tools/lstm_step_time.py and tools/lstm_seq_time.py: the container holds only the GRU, every shape is warmed up, the
two variants alternate window by window, a window is a number of calls between two device events sized from a trial to last at
least --window-ms.  One JSON line per shape: mean, minimum and maximum of the windows in microseconds per call and the largest
difference of the two variants' results.

    python tools/gru_time.py --mode step              # the tables of DESIGN.md section 7
    python tools/gru_time.py --mode seq
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/gru_time.py --mode step --kernel-only 200
                                                      # per-launch kernel times (k_gru_* rows)
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
from pfrl_amd.utils.recurrent import one_step_forward  # noqa: E402

STEP_SHAPES = [(8, 512, 512), (32, 512, 512), (128, 512, 512), (4, 32, 16)]     # (N, I, H)
RAGGED = [32, 29, 26, 23, 20, 16, 13, 10, 7, 4]
SEQ_SHAPES = [("example-8", [8] * 10, 512, 512, True), ("example-8-no-grad", [8] * 10, 512, 512, False),
              ("example-32", [32] * 10, 512, 512, True), ("example-32-no-grad", [32] * 10, 512, 512, False),
              ("ragged", RAGGED, 512, 512, True), ("ppo-test", [4] * 10, 32, 16, True)]
HBM_PEAK = 8e12                                                                  # bytes / s, MI355X


def run_steps(net, x, calls, variant, grad=False):
    os.environ["PFRL_GRU_CELL"] = variant
    state = None
    with torch.no_grad():
        for _ in range(calls):
            y, state = one_step_forward(net, x, state)
    return y, state[0]


def run_passes(net, packed, calls, variant, grad):
    os.environ["PFRL_GRU_SEQ"] = variant
    x = packed.data
    for _ in range(calls):
        with first_order_sequences(), torch.set_grad_enabled(grad):
            y, _ = net(packed, None)
        if grad:
            x.grad = None
            net.zero_grad(set_to_none=True)
            y.data.sum().backward()
    return y.data.detach(), (x.grad if grad else None)


def window_us(run, net, inp, calls, variant, grad):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    run(net, inp, calls, variant, grad)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("step", "seq"), required=True)
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--kernel-only", type=int, default=0, metavar="CALLS",
                    help="run CALLS calls of the HIP route per shape and nothing else (for a kernel trace)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    cases = []
    if args.mode == "step":
        for N, I, H in STEP_SHAPES:
            x = torch.randn(N, I, device="cuda")
            cases.append(({"N": N, "I": I, "H": H, "weight_bytes": 12 * H * (I + H),
                           "weights_at_hbm_peak_us": 12 * H * (I + H) / HBM_PEAK * 1e6}, I, H, x, False, run_steps))
    else:
        for name, sizes, I, H, grad in SEQ_SHAPES:
            packed = PackedSequence(torch.randn(sum(sizes), I, device="cuda", requires_grad=grad), torch.tensor(sizes))
            cases.append(({"shape": name, "batch_sizes": sizes, "I": I, "H": H, "backward": grad}, I, H, packed, grad, run_passes))
    for line, I, H, inp, grad, run in cases:
        torch.manual_seed(0)
        net = pfrl_amd.nn.RecurrentSequential(nn.GRU(I, H)).cuda()
        if args.kernel_only:
            run(net, inp, args.kernel_only, "1", grad)
            torch.cuda.synchronize()
            continue
        outs = {v: run(net, inp, 10, v, grad) for v in ("1", "0")}              # warm-up, and the results
        line["max_abs_diff"] = [float((a - b).abs().max()) for a, b in zip(outs["1"], outs["0"]) if a is not None]
        calls = {v: max(10, int(args.window_ms * 1e3 / window_us(run, net, inp, 20, v, grad))) for v in ("1", "0")}
        times = {"1": [], "0": []}
        for _ in range(args.windows):
            for v in ("1", "0"):
                times[v].append(window_us(run, net, inp, calls[v], v, grad))
        for v, key in (("1", "hip"), ("0", "library")):
            t = times[v]
            line[key] = {"mean_us": sum(t) / len(t), "min_us": min(t), "max_us": max(t), "calls_per_window": calls[v]}
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
