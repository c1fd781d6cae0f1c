#!/usr/bin/env python
"""The outside yardstick of profiles/trpo_update.txt: the REFERENCE's TRPO on the host cores, on the
workload of examples/train_trpo_gaussian_synthetic.py (same models, hyper-parameters, synthetic env
and loop -- the example's own functions with ``pfrl`` bound to the reference).  The reference is
taken where tools/reference_cpu_baseline.py takes it: the mounted checkout in the build container,
otherwise ``oracle/_ref/`` (its modules compiled by ``oracle/build_ref.py``, which travel with the
tree).

    python tools/trpo_reference_baseline.py --steps 40000
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_ROOT = os.environ.get(
    "PFRL_REFERENCE",
    "/root/reference" if os.path.isdir("/root/reference/pfrl") else os.path.join(ROOT, "oracle", "_ref"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=8 * 5000)
    ap.add_argument("--update-interval", type=int, default=5000)
    ap.add_argument("--warmup-updates", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "tests", "_gymshim"))
    sys.path.insert(0, REF_ROOT)
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import pfrl                                                     # the reference
    from pfrl import agents
    import train_trpo_gaussian_synthetic as ex

    assert os.path.realpath(os.path.dirname(pfrl.__file__)).startswith(os.path.realpath(REF_ROOT)), \
        "not the reference: %s" % pfrl.__file__
    ex.pfrl, ex.TRPO = pfrl, agents.TRPO
    pfrl.utils.set_random_seed(args.seed)
    env = ex.HostSyntheticVectorObsEnv(1, obs_dim=17, act_dim=6, seed=args.seed)
    agent = ex.make_agent(17, 6, -1, args.update_interval, switches=None)
    agent.n_updates = 0
    update = agent._update

    def counted(dataset):
        update(dataset)
        agent.n_updates += 1

    agent._update = counted
    marks = []
    ex.run(agent, env, args.steps, lambda t: marks.append((t, time.perf_counter())))
    w = args.warmup_updates
    (t0, c0), (t1, c1) = marks[w], marks[-1]
    print("reference TRPO on the host (%s): updates timed %d  env-steps/s %.1f  seconds/update-interval %.4f"
          % (os.path.basename(REF_ROOT.rstrip("/")), len(marks) - 1 - w, (t1 - t0) / (c1 - c0),
             (c1 - c0) / (len(marks) - 1 - w)))


if __name__ == "__main__":
    main()
