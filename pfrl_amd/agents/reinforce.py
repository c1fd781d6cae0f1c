"""Williams's episodic REINFORCE.

Mirrors ``pfrl.agents.reinforce.REINFORCE`` (/root/reference/pfrl/agents/reinforce.py): constructor
(:44-90), ``act`` / ``observe`` (:92-174), ``accumulate_grad`` / ``batch_update`` /
``update_with_accumulated_grad`` (:176-214) and the statistics (:216-219), quirks included: on
``done`` the last reward is appended a second time (:143), and the returns are
``np.cumsum(list(reversed(r_seq[1:])))[::-1]`` (:186), which drops the first reward and counts the
last twice.

Created without a GPU (``gpu=None / -1``), with ``recurrent=True``, or with
``recompute_forward=False``, the agent runs the reference's algorithm statement for statement: the
autograd graph of every acting step is kept for ``batchsize`` episodes, the update stacks one scalar
loss per step and runs backward through all of those batch-1 graphs.

With a GPU, a feed-forward model and ``recompute_forward=True`` (the default) acting runs under
``torch.no_grad()`` and stores the network's input row and the action of every step in device buffers.
The parameters do not change between the first acting step of a batch of episodes and its update, so
the update gets the same gradient from ONE forward over the M stored rows, one loss launch
(``pfrl_reinforce_loss`` behind a ``SoftmaxCategoricalHead``, ``pfrl_reinforce_gaussian_loss`` behind a
Gaussian head whose scale does not depend on the state; any other distribution keeps the torch
expression on the batched forward) and one backward.  This assumes a model that is deterministic in
train mode: with dropout or similar layers the recomputed forward is not the one that chose the
actions, and ``recompute_forward=False`` is the setting to use.

Out of scope: recurrent models on the device route, a captured acting graph, a batched REINFORCE
(the reference has none).
"""
import warnings
from logging import getLogger

import numpy as np
import torch

from pfrl_amd import agent, ops
from pfrl_amd.agents import _policy_split
from pfrl_amd.agents.trpo import _clip_l2_grad_norm_host_
from pfrl_amd.utils.batch_states import batch_states
from pfrl_amd.utils.mode_of_distribution import mode_of_distribution
from pfrl_amd.utils.recurrent import one_step_forward


def returns_of(r_seq):
    """The reference's returns of one finished episode (:186), float64 or int64 as NumPy accumulates
    them: ``r_seq`` holds the rewards with the last one twice, one entry more than the episode has
    steps."""
    return np.cumsum(list(reversed(r_seq[1:])))[::-1]


def _head_split(model, device):
    """How the loss of the stored rows runs behind ``model`` (``_policy_split.softmax_policy`` /
    ``gaussian_policy``):

      ("softmax", logits_fn, None)     ``Sequential(body..., Linear(K, A <= 31), SoftmaxCategoricalHead())``
      ("gaussian", mean_fn, scale_fn)  ``Sequential(..., Linear(., A <= 32), head)`` with a
                                       state-independent or fixed covariance
      None                             anything else: torch.distributions on the batched forward"""
    found = _policy_split.softmax_policy(model)
    if found is not None:
        body, pol = found
        return "softmax", (lambda x: pol(body(x))), None
    found = _policy_split.gaussian_policy(model, device)
    if found is not None:
        return "gaussian", found.view, found.scale
    return None


class REINFORCE(agent.AttributeSavingMixin, agent.Agent):
    """Williams's episodic REINFORCE.

    Args:
        model (Policy): Model to train. It must be a callable that accepts
            observations as input and return action distributions
            (Distribution).
        optimizer (torch.optim.Optimizer): optimizer used to train the model
        gpu (int): GPU device id if not None nor negative
        beta (float): Weight coefficient for the entropy regularizaiton term.
        phi (callable): Feature extractor function
        act_deterministically (bool): If set true, choose most probable actions
            in act method.
        batchsize (int): Number of episodes used for each update
        backward_separately (bool): If set true, call backward separately for
            each episode and accumulate only gradients.
        average_entropy_decay (float): Decay rate of average entropy. Used only
            to record statistics.
        batch_states (callable): Method which makes a batch of observations.
            default is `pfrl_amd.utils.batch_states`
        recurrent (bool): If set to True, `model` is assumed to implement
            `pfrl_amd.nn.Recurrent` and update in a recurrent
            manner.
        max_grad_norm (float or None): Maximum L2 norm of the gradient used for
            gradient clipping. If set to None, the gradient is not clipped.
        logger (logging.Logger): Logger to be used.
        recompute_forward (bool, keyword only): on a GPU with a feed-forward model, act without
            autograd graphs, keep every step's input row and action on the device and obtain the
            gradient of an update from one batched forward, one fused loss launch and one backward.
            Assumes a model that is deterministic in train mode; set it to False for models with
            dropout and similar layers.
    """

    saved_attributes = ("model", "optimizer")

    def __init__(
        self,
        model,
        optimizer,
        gpu=None,
        beta=0,
        phi=lambda x: x,
        batchsize=1,
        act_deterministically=False,
        average_entropy_decay=0.999,
        backward_separately=False,
        batch_states=batch_states,
        recurrent=False,
        max_grad_norm=None,
        logger=None,
        *,
        recompute_forward=True,
    ):
        self.model = model
        if gpu is not None and gpu >= 0:
            assert torch.cuda.is_available()
            self.device = torch.device("cuda:{}".format(gpu))
            self.model.to(self.device)
        else:
            self.device = torch.device("cpu")
        self.optimizer = optimizer
        self.beta = beta
        self.phi = phi
        self.batchsize = batchsize
        self.backward_separately = backward_separately
        self.act_deterministically = act_deterministically
        self.average_entropy_decay = average_entropy_decay
        self.batch_states = batch_states
        self.recurrent = recurrent
        self.max_grad_norm = max_grad_norm
        self.logger = logger or getLogger(__name__)
        self.recompute_forward = bool(recompute_forward)

        # Recurrent states of the model
        self.train_recurrent_states = None
        self.test_recurrent_states = None

        # Statistics
        self.average_entropy = 0

        self.t = 0
        self.reward_sequences = [[]]
        self.log_prob_sequences = [[]]
        self.entropy_sequences = [[]]
        self.n_backward = 0

        # the device route: input rows and actions of the pending episodes, in acting order
        self.device_route = (self.device.type == "cuda" and not self.recurrent
                             and self.recompute_forward)
        self._rows = None
        self._acts = None
        self._n_rows = 0            # rows stored, the episode in progress included
        self._episode_rows = 0      # of those, the episode in progress
        self._split = None
        self.last_loss = None       # the total loss of the latest accumulate_grad (0-dim tensor)
        if self.device_route:
            from pfrl_amd import _native

            _native.lib()          # no CPU fallback on this route: a missing library raises

    def act(self, obs):
        if self.training:
            return self._act_train(obs)
        else:
            return self._act_eval(obs)

    def observe(self, obs, reward, done, reset):
        if self.training:
            self._observe_train(obs, reward, done, reset)
        else:
            self._observe_eval(obs, reward, done, reset)

    def _act_train(self, obs):
        if self.device_route:
            return self._act_train_device(obs)
        batch_obs = self.batch_states([obs], self.device, self.phi)
        if self.recurrent:
            action_distrib, self.train_recurrent_states = one_step_forward(
                self.model, batch_obs, self.train_recurrent_states
            )
        else:
            action_distrib = self.model(batch_obs)
        batch_action = action_distrib.sample()

        # Save values used to compute losses
        self.log_prob_sequences[-1].append(action_distrib.log_prob(batch_action))
        self.entropy_sequences[-1].append(action_distrib.entropy())

        action = batch_action.cpu().numpy()[0]

        self.logger.debug("t:%s a:%s", self.t, action)

        # Update stats
        self.average_entropy += (1 - self.average_entropy_decay) * (
            float(action_distrib.entropy()) - self.average_entropy
        )

        return action

    def _act_train_device(self, obs):
        with torch.no_grad():
            batch_obs = self.batch_states([obs], self.device, self.phi)
            if not isinstance(batch_obs, torch.Tensor):
                raise TypeError("pfrl_amd REINFORCE: recompute_forward=True stores the network's input "
                                "as one tensor row per step; tuple observations need "
                                "recompute_forward=False")
            action_distrib = self.model(batch_obs)
            batch_action = action_distrib.sample()
            self._store(batch_obs, batch_action)
            entropy = float(action_distrib.entropy())
        action = batch_action.cpu().numpy()[0]

        self.logger.debug("t:%s a:%s", self.t, action)

        self.average_entropy += (1 - self.average_entropy_decay) * (entropy - self.average_entropy)

        return action

    def _store(self, batch_obs, batch_action, initial_capacity=64):
        """Row ``_n_rows`` of the buffers; they grow by doubling, earlier rows are copied once."""
        n = self._n_rows
        if self._rows is None:
            self._rows = torch.empty((initial_capacity,) + tuple(batch_obs.shape[1:]),
                                     dtype=batch_obs.dtype, device=self.device)
            self._acts = torch.empty((initial_capacity,) + tuple(batch_action.shape[1:]),
                                     dtype=batch_action.dtype, device=self.device)
        if n == self._rows.shape[0]:
            for name in ("_rows", "_acts"):
                old = getattr(self, name)
                new = torch.empty((2 * n,) + tuple(old.shape[1:]), dtype=old.dtype, device=self.device)
                new[:n].copy_(old)
                setattr(self, name, new)
        self._rows[n].copy_(batch_obs[0])
        self._acts[n].copy_(batch_action[0])
        self._n_rows = n + 1
        self._episode_rows += 1

    def _observe_train(self, obs, reward, done, reset):
        self.reward_sequences[-1].append(reward)
        self.t += 1

        if done or reset:
            if not done:
                warnings.warn(
                    "Since REINFORCE supports episodic environments only, "
                    "reset=True with done=False will throw away the last episode."
                )
                self.reward_sequences[-1] = []
                self.log_prob_sequences[-1] = []
                self.entropy_sequences[-1] = []
                self._n_rows -= self._episode_rows
                self._episode_rows = 0
            elif done:
                self.reward_sequences[-1].append(reward)
                self._episode_rows = 0
                if self.backward_separately:
                    self.accumulate_grad()
                    if self.n_backward == self.batchsize:
                        self.update_with_accumulated_grad()
                else:
                    if len(self.reward_sequences) == self.batchsize:
                        self.batch_update()
                    else:
                        # Prepare for the next episode
                        self.reward_sequences.append([])
                        self.log_prob_sequences.append([])
                        self.entropy_sequences.append([])
            self.train_recurrent_states = None

    def _act_eval(self, obs):
        with torch.no_grad():
            batch_obs = self.batch_states([obs], self.device, self.phi)
            if self.recurrent:
                action_distrib, self.test_recurrent_states = one_step_forward(
                    self.model, batch_obs, self.test_recurrent_states
                )
            else:
                action_distrib = self.model(batch_obs)
            if self.act_deterministically:
                return mode_of_distribution(action_distrib).cpu().numpy()[0]
            else:
                return action_distrib.sample().cpu().numpy()[0]

    def _observe_eval(self, obs, reward, done, reset):
        if done or reset:
            self.test_recurrent_states = None

    def accumulate_grad(self):
        if self.n_backward == 0:
            self.optimizer.zero_grad()
        if self.device_route:
            self._accumulate_grad_device()
        else:
            # Compute losses
            losses = []
            for r_seq, log_prob_seq, ent_seq in zip(
                self.reward_sequences, self.log_prob_sequences, self.entropy_sequences
            ):
                assert len(r_seq) - 1 == len(log_prob_seq) == len(ent_seq)
                # Convert rewards into returns (=sum of future rewards)
                R_seq = returns_of(r_seq)
                for R, log_prob, entropy in zip(R_seq, log_prob_seq, ent_seq):
                    loss = -R * log_prob - self.beta * entropy
                    losses.append(loss)
            total_loss = torch.stack(losses).sum() / self.batchsize
            total_loss.backward()
            self.last_loss = total_loss.detach()
        self.reward_sequences = [[]]
        self.log_prob_sequences = [[]]
        self.entropy_sequences = [[]]
        self.n_backward += 1

    def _return_column(self):
        """The returns of the pending episodes as ONE float32 column: ``-R * log_prob`` in the
        reference is a float32 product with ``R`` as a scalar, so each return is cast once."""
        R = np.concatenate([np.asarray(returns_of(r_seq)).astype(np.float32)
                            for r_seq in self.reward_sequences])
        return torch.from_numpy(R).to(self.device)

    def _accumulate_grad_device(self):
        M = self._n_rows
        assert self._episode_rows == 0
        assert sum(len(r_seq) - 1 for r_seq in self.reward_sequences) == M
        self.last_loss = self.loss_and_backward(self._rows[:M], self._acts[:M], self._return_column())
        self._n_rows = 0

    def loss_and_backward(self, rows, actions, ret):
        """One forward over ``rows`` [M, ...], the loss of ``actions`` weighted by the float32 return
        column ``ret`` [M], and backward into ``.grad`` (accumulating, as ``total_loss.backward()``
        does).  Returns the total loss, a 0-dim device tensor."""
        if self._split is None or self._split[0] is not self.model:
            self._split = (self.model, _head_split(self.model, self.device))
        split = self._split[1]
        inv_b = 1.0 / self.batchsize
        if split is None:
            distrib = self.model(rows)
            total_loss = (-ret * distrib.log_prob(actions) - self.beta * distrib.entropy()).sum() \
                / self.batchsize
            total_loss.backward()
            return total_loss.detach()
        kind, body, scale_of = split
        if kind == "softmax":
            logits = body(rows)
            out2, dlogits = ops.reinforce_loss(logits, actions, ret, inv_b, self.beta)
            logits.backward(dlogits)
            return out2[0]
        mean = body(rows)
        scale = scale_of()
        out2, dmean, dscale = ops.reinforce_gaussian_loss(mean, scale, actions, ret, inv_b, self.beta,
                                                         want_dscale=scale.requires_grad)
        if scale.requires_grad:
            torch.autograd.backward([mean, scale], [dmean, dscale])
        else:       # (a constant scale)
            mean.backward(dmean)
        return out2[0]

    def batch_update(self):
        assert len(self.reward_sequences) == self.batchsize
        assert len(self.log_prob_sequences) == self.batchsize
        assert len(self.entropy_sequences) == self.batchsize
        # Update the model
        assert self.n_backward == 0
        self.accumulate_grad()
        if self.max_grad_norm is not None:
            _clip_l2_grad_norm_host_(list(self.model.parameters()), self.max_grad_norm)
        self.optimizer.step()
        self.n_backward = 0

    def update_with_accumulated_grad(self):
        assert self.n_backward == self.batchsize
        if self.max_grad_norm is not None:
            _clip_l2_grad_norm_host_(list(self.model.parameters()), self.max_grad_norm)
        self.optimizer.step()
        self.n_backward = 0

    def get_statistics(self):
        return [
            ("average_entropy", self.average_entropy),
        ]
