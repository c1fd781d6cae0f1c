"""Trust Region Policy Optimization.

Mirrors ``pfrl.agents.trpo.TRPO`` (/root/reference/pfrl/agents/trpo.py): constructor (:166-195),
``batch_act`` / ``batch_observe`` (:701-835), the update (:318-324: normaliser statistics, policy by
conjugate gradient + line search, value function by SGD) and the statistics (:837-844).

Created without a GPU (``gpu=None / -1``), or with ``recurrent=True`` on any device, the agent runs
the reference's algorithm on lists of transition dicts (``ppo_host.HostRollouts`` and its dataset
helpers), with stock torch ops.

With a GPU and a feed-forward model it keeps the rollout where PPO keeps it (``agents/ppo.py``: HBM
columns, captured acting step, value pass, ``pfrl_gae_scan``) and runs the policy update without the
host reads the reference ends every small step with:

  gain / KL / entropy   pfrl_trpo_gaussian_eval behind the head-less policy (``_policy_split``), once
                        with the gradient of the gain and once per line-search trial; any other
                        policy keeps the torch.distributions expressions
  Fisher-vector product the reference's double backward through autograd, unchanged
  conjugate gradient    pfrl_cg_init / pfrl_cg_step: ``conjugate_gradient_max_iter`` unconditional
                        steps, the scalars and the convergence flag in a device state block
  KL-scaled step        pfrl_trpo_scale_step
  line search           pfrl_params_axpy writes the trial parameters; ONE device-to-host copy per
                        trial brings the trial's gain and KL, the reference's tests run on those
  value function        minibatch positions from PPO's walk of the ``random`` stream, one captured
                        graph per minibatch step

Out of scope: recurrent TRPO on the device rollout, a fused Fisher-vector product, the CG loop as
one captured graph.
"""
import collections
import random
from logging import getLogger

import numpy as np
import torch
import torch.nn.functional as F

from pfrl_amd import ops
from pfrl_amd.agents.dqn import _mean_or_nan
from pfrl_amd.agents import _policy_split
from pfrl_amd.agents.ppo import PPO, _iter_minibatch_positions
from pfrl_amd.agents.ppo_host import (HostRollouts, _actions, _states, _yield_minibatches,
                                      _yield_subset_of_sequences_with_fixed_number_of_items)
from pfrl_amd.utils.batch_states import batch_states
from pfrl_amd.utils.clip_l2_grad_norm import clip_grad_norm_device_, clip_l2_grad_norm_
from pfrl_amd.utils.conjugate_gradient import conjugate_gradient
from pfrl_amd.utils.contexts import evaluating
from pfrl_amd.utils.recurrent import (concatenate_recurrent_states, flatten_sequences_time_first,
                                      pack_and_forward)


# ---- the reference's module-level helpers (its tests and users call them) ---------------------------
def _flatten_and_concat_variables(vs):
    """One flat vector out of a list of tensors (reference :32-34)."""
    return torch.cat([torch.flatten(v) for v in vs], dim=0)


def _split_and_reshape_to_ndarrays(flat_v, sizes, shapes):
    """The inverse: pieces of ``sizes`` reshaped to ``shapes`` (reference :45-48)."""
    return [v.reshape(shape) for v, shape in zip(torch.split(flat_v, sizes), shapes)]


def _replace_params_data(params, new_params_data):
    """Overwrite parameters in place (reference :51-56)."""
    for param, new in zip(params, new_params_data):
        assert param.shape == new.shape
        assert isinstance(param, torch.nn.Parameter)
        param.data.copy_(new)


def _hessian_vector_product(flat_grads, params, vec):
    """H vec by one more backward through the gradient graph (reference :59-68)."""
    grads = torch.autograd.grad([torch.sum(flat_grads * vec.detach())], params, retain_graph=True)
    assert all(g is not None for g in grads), "The Hessian-vector product contains None."
    return _flatten_and_concat_variables(grads)


def _flat_grads(ys, params, grad_outputs=None, create_graph=False):
    grads = torch.autograd.grad(ys, params, grad_outputs=grad_outputs, create_graph=create_graph,
                                retain_graph=True)
    assert all(g is not None for g in grads), \
        "The gradient contains None. The policy may have unused parameters."
    return _flatten_and_concat_variables(grads)


def _clip_l2_grad_norm_host_(parameters, max_norm):
    """Gradient clipping of the value-function fit on the CPU with the reference's arithmetic there
    (pfrl/utils/clip_l2_grad_norm.py:29-37): NumPy's norm of the per-tensor NumPy norms, a Python
    float coefficient.  ``clip_l2_grad_norm_`` takes torch's function on every device; the two agree
    to rounding only, and the host route follows the reference to the bit."""
    grads = [p.grad.detach() for p in parameters if p.grad is not None]
    if not grads or grads[0].is_cuda:
        return clip_l2_grad_norm_(parameters, max_norm)
    total_norm = np.linalg.norm([np.linalg.norm(g.numpy()) for g in grads])
    coef = float(max_norm) / (total_norm + 1e-6)
    if coef < 1:
        for g in grads:
            g.mul_(coef)
    return total_norm


class _HostTRPO(HostRollouts):
    """The list-of-dicts rollout of ``ppo_host`` with TRPO's update (reference :318-334)."""

    def _normaliser_learns(self, transitions):
        a = self.agent
        if a.obs_normalizer:
            a.obs_normalizer.experience(batch_states([tr["state"] for tr in transitions], a.device,
                                                     a.phi))

    def _update(self, dataset):
        a = self.agent
        self._normaliser_learns(dataset)
        states = _states(dataset, "state", a.batch_states, a.device, a.phi, a.obs_normalizer)
        a._update_policy(lambda: a.policy(states), dataset)
        for batch in _yield_minibatches(dataset, minibatch_size=a.vf_batch_size,
                                        num_epochs=a.vf_epochs):
            vs_pred = a.vf(_states(batch, "state", a.batch_states, a.device, a.phi, a.obs_normalizer))
            self._vf_step(vs_pred, batch, column=True)
        a.n_updates += 1

    def _update_recurrent(self, dataset):
        a = self.agent
        self._normaliser_learns(flatten_sequences_time_first(dataset))
        ordered = sorted(dataset, key=len, reverse=True)        # longest first, for pack_sequence
        seqs = [_states(ep, "state", a.batch_states, a.device, a.phi, a.obs_normalizer)
                for ep in ordered]
        with torch.no_grad():
            rs = concatenate_recurrent_states([
                ep[0]["recurrent_state"][0] if ep[0]["recurrent_state"] is not None else None
                for ep in ordered])
        a._update_policy(lambda: pack_and_forward(a.policy, seqs, rs)[0],
                         flatten_sequences_time_first(ordered))
        for _ in range(a.vf_epochs):
            random.shuffle(dataset)
            for episodes in _yield_subset_of_sequences_with_fixed_number_of_items(
                    dataset, a.vf_batch_size):
                episodes = sorted(episodes, key=len, reverse=True)
                seqs = [_states(ep, "state", a.batch_states, a.device, a.phi, a.obs_normalizer)
                        for ep in episodes]
                with torch.no_grad():
                    rs = concatenate_recurrent_states([
                        ep[0]["recurrent_state"][1] if ep[0]["recurrent_state"] is not None else None
                        for ep in episodes])
                vs_pred, _ = pack_and_forward(a.vf, seqs, rs)
                self._vf_step(vs_pred, flatten_sequences_time_first(episodes), column=True)
        a.n_updates += 1

    def _vf_step(self, vs_pred, transitions, column):
        a = self.agent
        loss = F.mse_loss(vs_pred, self._column(transitions, "v_teacher", column=column))
        a.vf.zero_grad()
        loss.backward()
        if a.max_grad_norm is not None:
            _clip_l2_grad_norm_host_(list(a.vf.parameters()), a.max_grad_norm)
        a.vf_optimizer.step()


class TRPO(PPO):
    """Trust Region Policy Optimization (arguments as in the reference, then this package's
    switches).  ``policy`` and ``vf`` are separate models: the policy moves by conjugate gradient and
    a line search, the value function by ``vf_optimizer``.

    ``fused_gaussian_eval`` / ``device_cg`` / ``fused_param_step`` / ``capture_vf_step`` (device
    route only): False keeps the corresponding part of the update as eager torch on the device."""

    saved_attributes = ("policy", "vf", "vf_optimizer", "obs_normalizer")

    def __init__(self, policy, vf, vf_optimizer, obs_normalizer=None, gpu=None, gamma=0.99, lambd=0.95,
                 phi=lambda x: x, entropy_coef=0.01, update_interval=2048, max_kl=0.01, vf_epochs=3,
                 vf_batch_size=64, standardize_advantages=True, batch_states=batch_states,
                 recurrent=False, max_recurrent_sequence_len=None, line_search_max_backtrack=10,
                 conjugate_gradient_max_iter=10, conjugate_gradient_damping=1e-2,
                 act_deterministically=False, max_grad_norm=None, value_stats_window=1000,
                 entropy_stats_window=1000, kl_stats_window=100, policy_step_size_stats_window=100,
                 logger=getLogger(__name__), fused_gaussian_eval=True, device_cg=True,
                 fused_param_step=True, capture_vf_step=True, value_pass_chunk=16384):
        from pfrl_amd.nn import Branched, RecurrentBranched

        self.policy = policy
        self.vf = vf
        self.vf_optimizer = vf_optimizer
        self.obs_normalizer = obs_normalizer
        on_gpu = gpu is not None and gpu >= 0
        if on_gpu:
            assert torch.cuda.is_available()
            self.device = torch.device("cuda:{}".format(gpu))
            self.policy.to(self.device)
            self.vf.to(self.device)
            if self.obs_normalizer is not None:
                self.obs_normalizer.to(self.device)
        else:
            self.device = torch.device("cpu")
        self.recurrent = bool(recurrent)
        self.model = RecurrentBranched(policy, vf) if recurrent else Branched(policy, vf)
        self.gamma = gamma
        self.lambd = lambd
        self.phi = phi
        self.entropy_coef = entropy_coef
        self.update_interval = update_interval
        self.max_kl = max_kl
        self.vf_epochs = vf_epochs
        self.vf_batch_size = vf_batch_size
        self.standardize_advantages = standardize_advantages
        self.batch_states = batch_states
        self.max_recurrent_sequence_len = max_recurrent_sequence_len
        self.line_search_max_backtrack = line_search_max_backtrack
        self.conjugate_gradient_max_iter = conjugate_gradient_max_iter
        self.conjugate_gradient_damping = conjugate_gradient_damping
        self.act_deterministically = act_deterministically
        self.max_grad_norm = max_grad_norm
        self.logger = logger
        self.fused_gaussian_eval = bool(fused_gaussian_eval)
        self.device_cg = bool(device_cg)
        self.fused_param_step = bool(fused_param_step)
        self.capture_vf_step = bool(capture_vf_step)

        self.kl_record = collections.deque(maxlen=kl_stats_window)
        self.policy_step_size_record = collections.deque(maxlen=policy_step_size_stats_window)
        # what the rollout machinery of agents/ppo.py reads (n_updates: completed updates, policy
        # step + value-function fit)
        self._init_rollout_state(value_stats_window, entropy_stats_window, value_pass_chunk,
                                 reuse_next_values=False, device_actions=False)
        self._vf_graph = None
        self._vf_cols = None
        if on_gpu and not self.recurrent:
            from pfrl_amd import _native
            from pfrl_amd.staging import StagingRing

            _native.lib()          # no CPU fallback on this route: a missing library raises
            self._stage = StagingRing(self.device,
                                      slot_bytes=max(1 << 22, 96 * int(update_interval)), n_slots=8)
        else:
            self._host = _HostTRPO(self)

    # -- the policy update ---------------------------------------------------------------------
    def _compute_gain(self, log_prob, log_prob_old, entropy, advs):
        """The surrogate objective to maximise (reference :415-420)."""
        prob_ratio = torch.exp(log_prob - log_prob_old)
        return torch.mean(prob_ratio * advs) + self.entropy_coef * torch.mean(entropy)

    def _standardized(self, advs):
        if not self.standardize_advantages:
            return advs
        std, mean = torch.std_mean(advs, unbiased=False)
        return (advs - mean) / (std + 1e-8)

    def _update_policy(self, evaluate, transitions):
        """Reference :422-477 / :479-555 on a flat list of transitions whose fresh action
        distribution ``evaluate()`` returns (in the transitions' order)."""
        actions = _actions(transitions, self.device)
        advs = self._standardized(torch.as_tensor([tr["adv"] for tr in transitions],
                                                  device=self.device, dtype=torch.float))
        log_prob_old = torch.as_tensor([tr["log_prob"] for tr in transitions], device=self.device,
                                       dtype=torch.float)
        self._policy_step_by_distributions(evaluate, actions, advs, log_prob_old)

    def _policy_step_by_distributions(self, evaluate, actions, advs, log_prob_old):
        """One TRPO step with gain, KL and entropy as torch.distributions expressions -- the
        reference's update, on whatever device the tensors live.  On the device route the
        conjugate gradient and the parameter writes still take the kernels (``device_cg``,
        ``fused_param_step``), and a trial's gain and KL come to the host in one copy."""
        params = list(self.policy.parameters())
        on_dev = self._host is None
        distrib = evaluate()
        gain = self._compute_gain(distrib.log_prob(actions), log_prob_old, distrib.entropy(), advs)
        with torch.no_grad():
            distrib_old = evaluate()       # (distributions cannot be deep-copied)
        kl = torch.mean(torch.distributions.kl_divergence(distrib_old, distrib))
        full_step = self._kl_constrained_step(params, kl, _flat_grads([gain], params).detach())

        def trial():
            with torch.no_grad(), evaluating(self.policy):
                new = evaluate()
                new_gain = self._compute_gain(new.log_prob(actions), log_prob_old, new.entropy(), advs)
                new_kl = torch.mean(torch.distributions.kl_divergence(distrib_old, new))
            if on_dev:
                return torch.stack([new_gain, new_kl, gain.detach()])
            return float(new_gain), float(new_kl), float(gain.detach())

        self._line_search(params, full_step, trial)

    def _kl_constrained_step(self, params, kl, flat_gain_grads):
        """Reference :557-598: the step direction F^-1 g by conjugate gradient around Fisher-vector
        products (a double backward through ``kl``), scaled to the KL bound."""
        flat_kl_grads = _flat_grads([kl], params, create_graph=True)
        assert flat_kl_grads.requires_grad
        damping = self.conjugate_gradient_damping

        def fisher_vector_product(vec):
            vec = torch.as_tensor(vec)
            return _hessian_vector_product(flat_kl_grads, params, vec) + damping * vec

        on_dev = self._host is None
        if on_dev and self.device_cg:
            direction = ops.conjugate_gradient_device(fisher_vector_product, flat_gain_grads,
                                                      max_iter=self.conjugate_gradient_max_iter)
            full_step, _ = ops.trpo_scale_step(direction, fisher_vector_product(direction), self.max_kl)
            return full_step
        direction = conjugate_gradient(fisher_vector_product, flat_gain_grads,
                                       max_iter=self.conjugate_gradient_max_iter)
        dId = float(direction.dot(fisher_vector_product(direction)))
        return (2.0 * self.max_kl / (dId + 1e-8)) ** 0.5 * direction

    def _line_search(self, params, full_step, trial):
        """Reference :600-699.  ``trial()`` evaluates the policy as it stands and returns (gain,
        KL, gain before the step) as three floats or as one device tensor of three."""
        sizes = [p.numel() for p in params]
        shapes = [p.shape for p in params]
        flat_params = _flatten_and_concat_variables(params).detach()
        fused = self._host is None and self.fused_param_step and all(
            p.is_contiguous() and p.dtype == torch.float32 for p in params)

        def write(step_size):
            if fused:
                ops.params_axpy(params, flat_params, full_step, step_size)
            else:
                new = flat_params + step_size * full_step if step_size else flat_params
                _replace_params_data(params, _split_and_reshape_to_ndarrays(new, sizes, shapes))

        step_size = 1.0
        for i in range(self.line_search_max_backtrack + 1):
            self.logger.info("Line search iteration: %s step size: %s", i, step_size)
            write(step_size)
            out = trial()
            new_gain, new_kl, gain = out.tolist() if isinstance(out, torch.Tensor) else out
            improve = new_gain - gain
            self.logger.info("Surrogate objective improve: %s", improve)
            self.logger.info("KL divergence: %s", new_kl)
            if not np.isfinite(new_gain):
                self.logger.info("Surrogate objective is not finite. Backtracking...")
            elif not np.isfinite(new_kl):
                self.logger.info("KL divergence is not finite. Backtracking...")
            elif improve < 0:
                self.logger.info("Surrogate objective didn't improve. Backtracking...")
            elif new_kl > self.max_kl:
                self.logger.info("KL divergence exceeds max_kl. Backtracking...")
            else:
                self.kl_record.append(new_kl)
                self.policy_step_size_record.append(step_size)
                return
            step_size *= 0.5
        self.logger.info("Line search couldn't find a good step size. The policy was not updated.")
        self.policy_step_size_record.append(0.0)
        write(0.0)

    # -- the device route ---------------------------------------------------------------------------
    def _gaussian_found(self):
        """``_policy_split.gaussian_actor_critic`` of ``Branched(policy, vf)`` when gain / KL / entropy
        can run as pfrl_trpo_gaussian_eval: the policy ends in ``Linear(., A <= 32)`` + a Gaussian
        head whose scale does not depend on the state."""
        if not self.fused_gaussian_eval or self.device.type != "cuda":
            return None
        hit = self.__dict__.get("_policy_split_cache")
        if hit is None or hit[0] is not self.model:
            hit = self._policy_split_cache = (
                self.model, _policy_split.gaussian_actor_critic(self.model, self.device))
        return hit[1]

    def _gaussian_policy_split(self):
        """(head-less policy, head) of ``_gaussian_found()``, or None."""
        found = self._gaussian_found()
        return None if found is None else (found.view.child_modules[0], found.head)

    def _policy_step_fused(self, found, states, actions, advs, log_prob_old):
        """The same step with the Gaussian row arithmetic in pfrl_trpo_gaussian_eval: once with the
        gradient of the gain (backpropagated through the head-less policy by autograd), once per
        line-search trial without.  The KL whose double backward is the Fisher-vector product is
        the reference's expression on the head's own distribution."""
        body, head, scale_of = found.view.child_modules[0], found.head, found.scale
        params = list(self.policy.parameters())
        mean = body(states)
        scale = scale_of()
        mean_old, scale_old = mean.detach(), scale.detach().contiguous()
        out0, dmean, dscale = ops.trpo_gaussian_eval(mean, scale, mean_old, scale_old, actions, advs,
                                                     log_prob_old, self.entropy_coef, want_grad=True)
        if scale.requires_grad:
            flat_gain_grads = _flat_grads([mean, scale], params, grad_outputs=[dmean, dscale])
        else:       # (a constant scale)
            flat_gain_grads = _flat_grads([mean], params, grad_outputs=[dmean])
        with torch.no_grad():
            distrib_old = head(mean_old)
        kl = torch.mean(torch.distributions.kl_divergence(distrib_old, head(mean)))
        full_step = self._kl_constrained_step(params, kl, flat_gain_grads.detach())

        def trial():
            with torch.no_grad(), evaluating(self.policy):
                out = ops.trpo_gaussian_eval(body(states), scale_of(), mean_old, scale_old, actions,
                                             advs, log_prob_old, self.entropy_coef)
                return torch.stack([out[0], out[1], out0[0]])

        self._line_search(params, full_step, trial)

    def _update_policy_device(self, states, actions, advs, log_prob_old):
        found = (self._gaussian_found()
                 if actions.dtype == torch.float32 and actions.dim() == 2 else None)
        if found is not None:
            self._policy_step_fused(found, states, actions, advs, log_prob_old)
        else:
            self._policy_step_by_distributions(lambda: self.policy(states), actions, advs,
                                               log_prob_old)

    def _update(self):
        """Reference :265-306 + :318-324 on the rollout's columns."""
        ro = self.rollout
        T, N, k = ro.T, ro.N, ro.k
        order = ro.dataset_order()
        n = len(order)
        assert n == T * N
        self._check_frames_alive(ro)
        up = self._stage.upload([
            ro.h_state[:T].reshape(T * N, k), ro.h_next[:T].reshape(T * N, k),
            ro.h_action[:T].reshape((T * N,) + ro.h_action.shape[2:]),
            ro.h_reward[:T].reshape(-1), ro.h_nonterm[:T].reshape(-1),
            self._cut_with_rollout_end(ro, T).reshape(-1), order])
        # (staging views are recycled when the ring wraps: private device copies)
        s_refs, n_refs, actions, reward, nonterm, cut, order_dev = [t.clone() for t in up]
        log_probs, v_pred = self._value_pass(s_refs, actions)
        next_v = self._next_values(ro, T, N, v_pred, n_refs)
        adv, v_teacher = ops.gae_scan(reward.view(T, N), v_pred.view(T, N), next_v.view(T, N),
                                      nonterm.view(T, N), cut.view(T, N), self.gamma, self.lambd,
                                      self._reward_mode)
        adv, v_teacher = adv.view(-1), v_teacher.view(-1)
        if self.obs_normalizer is not None:
            with torch.no_grad():
                self.obs_normalizer.experience(self._gather(s_refs))
        # the full batch in the reference's dataset order (finished fragments first)
        advs = adv[order_dev]
        if self.standardize_advantages:
            mean_std = ops.adv_stats(adv)
            advs = (advs - mean_std[0]) / (mean_std[1] + 1e-8)
        with torch.no_grad():
            states = self._features(s_refs[order_dev])
        self._update_policy_device(states, actions[order_dev], advs, log_probs[order_dev])
        self._fit_vf(s_refs, v_teacher, order)
        with torch.no_grad():
            vart = torch.var(v_teacher, unbiased=False)
            ev = 1 - torch.var(v_teacher - v_pred, unbiased=False) / vart
            self.explained_variance = float("nan") if float(vart) == 0 else float(ev)
        self.n_updates += 1

    # -- the value function fit (reference :387-413) ---------------------------------------------------
    def _fit_vf(self, s_refs, v_teacher, order):
        src = dict(s_refs=s_refs, v_teacher=v_teacher)
        capture = self.capture_vf_step and self.device.type == "cuda"
        if capture:
            cols = self._vf_cols
            if cols is None or any(cols[name].shape != v.shape for name, v in src.items()):
                cols = self._vf_cols = {name: torch.empty_like(v) for name, v in src.items()}
                cols["idx"] = torch.empty(self.vf_batch_size, dtype=torch.int64, device=self.device)
                self._vf_graph = None
            for name, v in src.items():
                cols[name].copy_(v)
            if self._vf_graph is None:
                from pfrl_amd.agents.graphed_update import CapturedStep

                self._vf_graph = CapturedStep(self._vf_step, [self.vf], [self.vf_optimizer],
                                              self.device, lr_on_device=True)
        for pos in _iter_minibatch_positions(len(order), self.vf_batch_size, self.vf_epochs):
            (idx,) = self._stage.upload([order[pos]])
            if capture:
                cols["idx"].copy_(idx)
                self._vf_graph.run({"idx": cols["idx"]},
                                   baked=(None if self.max_grad_norm is None
                                          else float(self.max_grad_norm), id(self.vf)))
            else:
                self._vf_step({"idx": idx}, src)

    def _vf_step(self, batch, cols=None):
        c = self._vf_cols if cols is None else cols
        idx = batch["idx"]
        with torch.no_grad():
            states = self._features(c["s_refs"][idx])
        loss = F.mse_loss(self.vf(states), c["v_teacher"][idx][..., None])
        self.vf_optimizer.zero_grad(set_to_none=True)
        loss.backward()
        if self.max_grad_norm is not None:
            clip_grad_norm_device_(self.vf.parameters(), self.max_grad_norm)
        self.vf_optimizer.step()
        return {"loss": loss.detach()}

    def get_statistics(self):
        return [
            ("average_value", _mean_or_nan(self.value_record.values())),
            ("average_entropy", _mean_or_nan(self.entropy_record.values())),
            ("average_kl", _mean_or_nan(self.kl_record)),
            ("average_policy_step_size", _mean_or_nan(self.policy_step_size_record)),
            ("explained_variance", self.explained_variance),
        ]
