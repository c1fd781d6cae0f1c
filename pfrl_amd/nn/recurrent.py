"""Recurrent containers (reference pfrl/nn/recurrent.py:1-30, recurrent_sequential.py:12-62,
recurrent_branched.py:6-26).

The calling convention is ``torch.nn.LSTM``'s with packed input:
``module(packed_sequences, recurrent_state) -> (packed_output, new_recurrent_state)``, where a
``None`` state means "start of sequence"."""
import contextlib
import os
import threading

import torch
from torch import nn
from torch.nn.utils.rnn import PackedSequence

from pfrl_amd import _native, ops
from pfrl_amd.utils.recurrent import (get_packed_sequence_info, is_recurrent,
                                      unwrap_packed_sequences_recursive,
                                      wrap_packed_sequences_recursive)


class Recurrent(object):
    """Marker + interface of a stateful module."""

    def forward(self, packed_input, recurrent_state):
        raise NotImplementedError


def _kernel_member_and_input(member, cls, packed):
    """What the four routes below ask of the member and its input alike: a plain one-layer,
    one-direction ``cls`` in f32 on the device of a ``PackedSequence`` without ``sorted_indices``."""
    if (type(member) is not cls or member.num_layers != 1 or member.bidirectional
            or member.proj_size != 0):
        return False
    if not isinstance(packed, PackedSequence) or packed.sorted_indices is not None:
        return False
    x, w_ih = packed.data, member.weight_ih_l0
    return (x.is_cuda and x.dtype == torch.float32 and w_ih.dtype == torch.float32
            and w_ih.device == x.device and _native.available())


def lstm_cell_step_or_none(member, packed, state):
    """One acting step of an ``nn.LSTM`` member as one launch (``ops.lstm_cell_step``), or None where
    the member, the input or the mode is not the kernel's: the caller then runs the member itself.
    Returns what ``nn.LSTM`` returns for a one-step packed input: the ``PackedSequence`` over h1 and
    the state ``(h1[None], c1[None])`` of shape (1, N, H), output and state in separate buffers (an
    in-place member behind the LSTM must not reach the carried state).  Training passes (gradients enabled) and
    whole sequences are :func:`lstm_sequence_or_none`'s, or the library's."""
    if os.environ.get("PFRL_LSTM_CELL", "1") == "0" or torch.is_grad_enabled():
        return None
    if not _kernel_member_and_input(member, nn.LSTM, packed) or packed.batch_sizes.numel() != 1:
        return None
    x, w_ih = packed.data, member.weight_ih_l0
    N, H = x.shape[0], member.hidden_size
    if not ops.lstm_cell_supported(N, x.shape[1], H):
        return None
    h0, c0 = (None, None) if state is None else (state[0][0].contiguous(), state[1][0].contiguous())
    b_ih, b_hh = (member.bias_ih_l0, member.bias_hh_l0) if member.bias else (None, None)
    h1, c1, y = ops.lstm_cell_step(x.contiguous(), h0, c0, w_ih.contiguous(),
                                   member.weight_hh_l0.contiguous(), b_ih, b_hh, want_output=True)
    return PackedSequence(y, packed.batch_sizes, None, None), (h1[None], c1[None])


_route = threading.local()


@contextlib.contextmanager
def first_order_sequences():
    """Inside this block (per thread) a container may take an ``nn.LSTM`` or ``nn.GRU`` member's whole
    packed sequence, training passes included, to ``ops.lstm_sequence`` / ``ops.gru_sequence``.  The
    caller vouches that it differentiates the result at most once and does not hold it to ``nn.LSTM``'s bits: the DQN family's
    and PPO's recurrent updates enter it; TRPO (a Fisher-vector product differentiates twice),
    REINFORCE and bare container calls do not, and keep ``nn.LSTM``."""
    before, _route.sequences = getattr(_route, "sequences", False), True
    try:
        yield
    finally:
        _route.sequences = before


def lstm_sequence_or_none(member, packed, state):
    """A packed sequence through an ``nn.LSTM`` member as ``ops.lstm_sequence`` (one library GEMM for
    the input projection, one launch of csrc/lstm_seq.hip per time step, forward and backward), or
    None: outside :func:`first_order_sequences`, with ``PFRL_LSTM_SEQ=0``, or where the member, the
    input or the shape is not the kernels'.  Returns what ``nn.LSTM`` returns."""
    if not getattr(_route, "sequences", False) or os.environ.get("PFRL_LSTM_SEQ", "1") == "0":
        return None
    if not _kernel_member_and_input(member, nn.LSTM, packed):
        return None
    x, w_ih = packed.data, member.weight_ih_l0
    sizes = packed.batch_sizes.tolist()          # (a CPU tensor: no synchronisation)
    if not ops.lstm_sequence_supported(sizes, x.shape[1], member.hidden_size):
        return None
    h0, c0 = (None, None) if state is None else (state[0][0], state[1][0])
    b_ih, b_hh = (member.bias_ih_l0, member.bias_hh_l0) if member.bias else (None, None)
    y, hn, cn = ops.lstm_sequence(x, sizes, h0, c0, w_ih, member.weight_hh_l0, b_ih, b_hh)
    return PackedSequence(y, packed.batch_sizes, None, None), (hn[None], cn[None])


def gru_cell_step_or_none(member, packed, state):
    """:func:`lstm_cell_step_or_none` for an ``nn.GRU`` member (``ops.gru_cell_step``, csrc/gru.hip;
    ``PFRL_GRU_CELL=0`` keeps the library).  The state is ``nn.GRU``'s: one tensor ``h1[None]`` of
    shape (1, N, H), in a buffer of its own next to the output."""
    if os.environ.get("PFRL_GRU_CELL", "1") == "0" or torch.is_grad_enabled():
        return None
    if not _kernel_member_and_input(member, nn.GRU, packed) or packed.batch_sizes.numel() != 1:
        return None
    x = packed.data
    if not ops.gru_cell_supported(x.shape[0], x.shape[1], member.hidden_size):
        return None
    b_ih, b_hh = (member.bias_ih_l0, member.bias_hh_l0) if member.bias else (None, None)
    h1, y = ops.gru_cell_step(x.contiguous(), None if state is None else state[0].contiguous(),
                              member.weight_ih_l0.contiguous(), member.weight_hh_l0.contiguous(), b_ih, b_hh,
                              want_output=True)
    return PackedSequence(y, packed.batch_sizes, None, None), h1[None]


def gru_sequence_or_none(member, packed, state):
    """:func:`lstm_sequence_or_none` for an ``nn.GRU`` member (``ops.gru_sequence``, csrc/gru_seq.hip;
    ``PFRL_GRU_SEQ=0`` keeps the library): only inside :func:`first_order_sequences`."""
    if not getattr(_route, "sequences", False) or os.environ.get("PFRL_GRU_SEQ", "1") == "0":
        return None
    if not _kernel_member_and_input(member, nn.GRU, packed):
        return None
    x = packed.data
    sizes = packed.batch_sizes.tolist()          # (a CPU tensor: no synchronisation)
    if not ops.gru_sequence_supported(sizes, x.shape[1], member.hidden_size):
        return None
    b_ih, b_hh = (member.bias_ih_l0, member.bias_hh_l0) if member.bias else (None, None)
    y, hn = ops.gru_sequence(x, sizes, None if state is None else state[0], member.weight_ih_l0,
                             member.weight_hh_l0, b_ih, b_hh)
    return PackedSequence(y, packed.batch_sizes, None, None), hn[None]


class RecurrentSequential(Recurrent, nn.Sequential):
    """``nn.Sequential`` whose recurrent members (LSTM / GRU / RNN / ``Recurrent``) each own one
    slot of the tuple state.  Stateless members run once on the flat time-major tensor under the
    ``PackedSequence`` -- all time steps of all sequences in one launch -- and the packing is
    re-applied only where a recurrent member needs it."""

    @property
    def recurrent_children(self):
        return tuple(m for m in self if is_recurrent(m))

    def forward(self, sequences, recurrent_state):
        n_slots = len(self.recurrent_children)
        if recurrent_state is None:
            recurrent_state = (None,) * n_slots
        assert len(recurrent_state) == n_slots
        packing = get_packed_sequence_info(sequences)
        h, packed = sequences, True
        slot, new_state = 0, []
        for member in self:
            if is_recurrent(member):
                if not packed:
                    h, packed = wrap_packed_sequences_recursive(h, *packing), True
                h, s = (lstm_cell_step_or_none(member, h, recurrent_state[slot])
                        or lstm_sequence_or_none(member, h, recurrent_state[slot])
                        or gru_cell_step_or_none(member, h, recurrent_state[slot])
                        or gru_sequence_or_none(member, h, recurrent_state[slot])
                        or member(h, recurrent_state[slot]))
                new_state.append(s)
                slot += 1
            else:
                if packed:
                    h, packed = unwrap_packed_sequences_recursive(h), False
                h = member(h)
        if not packed:
            h = wrap_packed_sequences_recursive(h, *packing)
        assert slot == n_slots
        return h, tuple(new_state)


class RecurrentBranched(Recurrent, nn.ModuleList):
    """Feeds the same packed input to every branch; outputs and states are tuples in branch order."""

    def __init__(self, *modules):
        super().__init__(modules)

    def forward(self, sequences, recurrent_state):
        if recurrent_state is None:
            recurrent_state = (None,) * len(self)
        outs, states = [], []
        for branch, s in zip(self, recurrent_state):
            y, s = branch(sequences, s)
            outs.append(y)
            states.append(s)
        return tuple(outs), tuple(states)
