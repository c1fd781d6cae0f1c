#!/usr/bin/env python
"""REINFORCE fixtures, recorded by running the REFERENCE (pfnet/pfrl) itself on the CPU.

    python tests/golden/make_reinforce_fixtures.py   (build container only: needs the reference checkout)

api_signatures_reinforce.json
    the signatures of ``pfrl.agents.REINFORCE`` and its public methods (tests/_api_surface.py's format).

agent_trace_reinforce.npz
    the reference's REINFORCE on the scripted env of tests/test_reinforce_cpu.py (observations of 5
    numbers, episodes of 1, 7 and 12 steps in turn) with a 16-unit tanh policy, ``beta = 0.01``,
    ``max_grad_norm = 1.0``, Adam, six updates, in four configurations: {``SoftmaxCategoricalHead`` with
    3 actions, ``GaussianHeadWithStateIndependentCovariance`` with 2 action dimensions} x
    {``batchsize=1``, ``batchsize=3, backward_separately=True``}; the rewards are Python floats except
    in ``sm_b3_``, whose Python ints give an int64 returns column.  Per configuration: the initial
    parameters; per step, in acting order (every step belongs to exactly one update), the network's
    input row, the action and the return (the reference's own cumsum, stored as float64, which holds
    the int64 sums exactly); per ``accumulate_grad`` call its number of rows and its loss (the tensor
    the reference called ``backward`` on), ``update_calls`` calls per update; per update the
    parameters before, the gradient before clipping and the parameters after
    (tests/test_reinforce_cpu.py::update_of slices them).  Recorded under the settings of ``PINNED``
    below (stored in the fixture as ``pinned_env_names`` / ``pinned_env_values``).

    The tolerances that go with the gradient and the parameters are MEASURED, not chosen: every
    update is run twice from the same state, by the agent itself (float32) and by a float64 twin (the
    reference agent on a float64 copy of the model and of Adam's state, teacher-forced with the same
    rows, actions and rewards); ``*_grad_tol`` / ``*_param_tol`` are ten times the largest difference
    between the gradients / the parameters the two leave.  The factor of ten covers another
    implementation rounding in a different order.
"""
import copy
import json
import os
import sys

# One CPU code path on every processor, chosen before torch loads (see make_trpo_fixtures.py).
PINNED = {"ATEN_CPU_CAPABILITY": "default", "MKL_CBWR": "COMPATIBLE", "OMP_NUM_THREADS": "1",
          "MKL_NUM_THREADS": "1"}
os.environ.update(PINNED)

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_golden as mg  # noqa: E402,F401  (puts the reference and the gym shim on sys.path)
import test_reinforce_cpu as shared  # noqa: E402
from _api_surface import API_METHODS, describe_signature  # noqa: E402


def flat(tensors):
    return np.concatenate([t.detach().cpu().numpy().ravel() for t in tensors])


def signatures(pfrl):
    cls = pfrl.agents.REINFORCE
    desc = {"agents.REINFORCE": describe_signature(cls)}
    for meth in API_METHODS:
        if callable(getattr(cls, meth, None)):
            desc["agents.REINFORCE." + meth] = describe_signature(getattr(cls, meth))
    desc["agents.REINFORCE.saved_attributes"] = list(cls.saved_attributes)
    return desc


def double_twin(pfrl, ag, prefix):
    """The agent's learning state in float64: model, Adam state, the same hyperparameters."""
    model = copy.deepcopy(ag.model).double()
    opt = torch.optim.Adam(model.parameters(), lr=shared.LR)
    for p32, p64 in zip(ag.model.parameters(), model.parameters()):
        st = ag.optimizer.state.get(p32)
        if st:
            opt.state[p64] = {k: (v.clone().double() if torch.is_tensor(v) and v.dim() > 0
                                  else copy.deepcopy(v)) for k, v in st.items()}
    _, batchsize, separately, _ = shared.CONFIGS[prefix]
    return pfrl.agents.REINFORCE(model, opt, gpu=-1, batchsize=batchsize,
                                 backward_separately=separately, **shared.HYPER)


class capture_backward:
    """While the reference accumulates: the value of every tensor ``backward`` is called on."""

    def __enter__(self):
        self.values = []
        self.saved = torch.Tensor.backward
        values, saved = self.values, self.saved

        def backward(tensor, *args, **kwargs):
            values.append(tensor.detach().clone())
            return saved(tensor, *args, **kwargs)

        torch.Tensor.backward = backward
        return self

    def __exit__(self, *exc):
        torch.Tensor.backward = self.saved
        return False


def trace(pfrl, prefix, out):
    import pfrl.agents.reinforce as ref_module

    head, batchsize, separately, ints = shared.CONFIGS[prefix]
    torch.manual_seed(1357)         # (the initial parameters; recorded below)
    model = shared.make_model(pfrl, head)
    ag = shared.make_agent(pfrl, prefix, model, gpu=-1)
    out[prefix + "init_params"] = flat(model.parameters())
    out[prefix + "int_rewards"] = np.asarray(ints)
    pending = {"rows": [], "actions": []}      # steps acted since the last accumulate_grad
    upd = {}                                   # the update being recorded
    count = [0]
    records, acted, seen = {}, [], [0]
    worst = {"grad": 0.0, "param": 0.0}

    orig_batch_states = ag.batch_states

    def spy_batch_states(states, device, phi):
        batch = orig_batch_states(states, device, phi)
        if ag.training:
            pending["rows"].append(batch.numpy()[0].copy())
        return batch

    orig_accumulate = ag.accumulate_grad

    def spy_accumulate():
        if ag.n_backward == 0:
            upd.clear()
            upd.update(before=flat(model.parameters()), rows=[], actions=[], returns=[], call_rows=[],
                       loss=[], twin=double_twin(pfrl, ag, prefix))
        twin = upd["twin"]
        rows, actions = np.stack(pending["rows"]), np.stack(pending["actions"])
        pending["rows"], pending["actions"] = [], []
        returns = [np.cumsum(list(reversed(r_seq[1:])))[::-1] for r_seq in ag.reward_sequences]
        assert sum(len(R) for R in returns) == len(rows)
        assert all(R.dtype == (np.int64 if ints else np.float64) for R in returns)
        # the twin: the reference's own accumulate_grad on float64 graphs of the same steps
        twin.reward_sequences = copy.deepcopy(ag.reward_sequences)
        twin.log_prob_sequences, twin.entropy_sequences = [], []
        at = 0
        for R in returns:
            lps, ents = [], []
            for i in range(at, at + len(R)):
                distrib = twin.model(torch.from_numpy(rows[i:i + 1]).double())
                a = torch.from_numpy(actions[i:i + 1])
                lps.append(distrib.log_prob(a.double() if a.dtype == torch.float32 else a))
                ents.append(distrib.entropy())
            at += len(R)
            twin.log_prob_sequences.append(lps)
            twin.entropy_sequences.append(ents)
        twin.accumulate_grad()
        with capture_backward() as cap:
            orig_accumulate()
        assert len(cap.values) == 1
        upd["rows"].append(rows)
        upd["actions"].append(actions)
        upd["returns"].append(np.concatenate(returns).astype(np.float64))
        upd["call_rows"].append(len(rows))
        upd["loss"].append(float(cap.values[0]))

    orig_clip = ref_module.clip_l2_grad_norm_

    def spy_clip(parameters, max_norm):
        parameters = list(parameters)
        if parameters[0] is next(iter(model.parameters())):
            upd["grad"] = flat(p.grad for p in parameters)
            grad64 = flat(p.grad for p in upd["twin"].model.parameters())
            worst["grad"] = max(worst["grad"], float(np.abs(upd["grad"] - grad64).max()))
        return orig_clip(parameters, max_norm)

    def finished():
        twin = upd["twin"]
        assert twin.n_backward == batchsize
        twin.update_with_accumulated_grad()
        after = flat(model.parameters())
        worst["param"] = max(worst["param"], float(np.abs(after - flat(twin.model.parameters())).max()))
        rec = dict(params_before=upd["before"], rows=np.concatenate(upd["rows"]),
                   returns=np.concatenate(upd["returns"]), grad=upd["grad"], params_after=after,
                   call_rows=np.asarray(upd["call_rows"], dtype=np.int64),
                   loss=np.asarray(upd["loss"], dtype=np.float32))
        assert np.array_equal(np.concatenate(upd["actions"]), np.asarray(acted[seen[0]:seen[0] + len(rec["rows"])]))
        seen[0] += len(rec["rows"])
        for name, value in rec.items():
            records.setdefault(name, []).append(value)
        count[0] += 1

    orig_step = ag.optimizer.step

    def spy_step(*a, **k):
        res = orig_step(*a, **k)
        finished()
        return res

    ag.batch_states = spy_batch_states
    ag.accumulate_grad = spy_accumulate
    ref_module.clip_l2_grad_norm_ = spy_clip
    ag.optimizer.step = spy_step
    orig_act = ag.act

    def spy_act(obs):
        a = orig_act(obs)
        pending["actions"].append(np.asarray(a).copy())
        acted.append(np.asarray(a).copy())
        return a

    ag.act = spy_act
    try:
        actions, after = shared.run_loop(ag, prefix)
    finally:
        ref_module.clip_l2_grad_norm_ = orig_clip
    assert count[0] == shared.UPDATES == len(after)
    assert seen[0] == len(actions)       # every step belongs to one update, in acting order
    for name in ("params_before", "grad", "params_after"):
        out[prefix + name] = np.stack(records[name])
    for name in ("rows", "returns", "call_rows", "loss"):
        out[prefix + name] = np.concatenate(records[name])
    out[prefix + "update_calls"] = np.asarray([len(c) for c in records["call_rows"]], dtype=np.int64)
    assert all(np.array_equal(a, b) for a, b in zip(after, records["params_after"]))
    out[prefix + "actions"] = actions
    out[prefix + "average_entropy"] = np.asarray(ag.average_entropy)
    out[prefix + "f32_f64_grad_diff"] = np.asarray(worst["grad"])
    out[prefix + "f32_f64_param_diff"] = np.asarray(worst["param"])
    out[prefix + "grad_tol"] = np.asarray(10.0 * worst["grad"])
    out[prefix + "param_tol"] = np.asarray(10.0 * worst["param"])
    print(prefix, "steps", len(actions), "f32-f64 gradient difference", worst["grad"],
          "parameter difference", worst["param"])


def main():
    import pfrl

    with open(os.path.join(HERE, "api_signatures_reinforce.json"), "w") as f:
        json.dump(signatures(pfrl), f, indent=1, sort_keys=True)
        f.write("\n")
    out = {}
    for prefix in shared.CONFIGS:
        trace(pfrl, prefix, out)
    assert torch.backends.cpu.get_cpu_capability() == "DEFAULT" and torch.get_num_threads() == 1
    out["pinned_env_names"] = np.asarray(sorted(PINNED))
    out["pinned_env_values"] = np.asarray([PINNED[k] for k in sorted(PINNED)])
    out["hyper_names"] = np.asarray(sorted(shared.HYPER) + ["lr"])
    out["hyper_values"] = np.asarray([float(shared.HYPER[k]) for k in sorted(shared.HYPER)] + [shared.LR])
    path = os.path.join(HERE, "agent_trace_reinforce.npz")
    np.savez_compressed(path, **out)
    print("agent_trace_reinforce", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
