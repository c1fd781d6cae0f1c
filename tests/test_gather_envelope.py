"""csrc/frames.hip, csrc/replay.hip and csrc/nhwc.h -- the gather and scatter kernels every minibatch
passes through -- over every path their launchers select and every tail their loops have, through
``pfrl_amd.ops``, against plain NumPy.

Everything here is integer movement, a correctly rounded division or an f64 sum in a fixed order, so
every comparison is bit for bit (``assert_array_equal`` on integers and on the uint32 / uint64 view
of floats); there is no tolerance in this file.

References (NumPy only, none taken from another kernel; tests/test_gather_envelope_cpu.py pins them to
the C oracle on a machine without a GPU):

* u8 conversion    ``frames[refs].astype(float32) / float32(d)`` -- IEEE division, as ``__fdiv_rn``
* channels-last    the same values transposed to [M, H, W, 4]
* raw nhwc4        ``np.stack`` of the four u8 frames on the last axis
* n-step scalars   reward = the sequential f64 sum acc = acc + gp[i] * r[t_i] cast to f32, discount
                   = float32(gp[len]), terminal = any, action and state from the first transition,
                   next state from transition len - 1
* synthetic frames the generator of ``k_frames_synth`` in ``np.uint64`` arithmetic: ``mix64`` is the
                   splitmix64 finaliser, key = mix64(seed ^ mix64((env_id0 + f) * GOLDEN + step)),
                   word i of the frame = mix64(key + i * STRIDE), little endian, 4-byte tail = the low
                   half of word frame_bytes // 8

Guards: every output is a slice of a larger buffer with 4 KiB before and after it, filled (payload
included, so that an element the kernel leaves unwritten shows) with a byte pattern no kernel here
produces -- 0xA5 bytes for u8 / int outputs, the NaN 0x7FA5A5A5 for f32 -- and the guard zones must
hold that pattern after the launch.  Stores updated in place (frame stores, table columns) are
compared WHOLE with the NumPy result, which shows untouched slots and rows unchanged.

The cases are the smallest shapes that reach each branch: the one-dword-per-lane boundary (1024 B)
and the one-trip boundary (kThreads * kUnroll = 2048 dwords = 8192 B) of ``convert_frame`` /
``move_frame``, the 1024-pixel tile of nhwc.h, the 256-row scalar workgroup, the 2048-workgroup cap
of ``pfrl_batch_states_f32``, ``kNtMinBytes`` = 32 MiB from both sides, the switch to
``k_batch_experiences_f32_small`` (f32, frame_bytes % 16 == 0, <= 8192 B, 2 B k >= 4096), and the
table limits PFRL_MAX_STACK = 8 and PFRL_MAX_NSTEP = 16.
"""
import itertools
import random
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 4096                       # bytes on each side of every output
NAN_BITS = 0x7FA5A5A5              # f32 guard / fill pattern (a NaN)
U8, I32, I64, F32, F64 = "u8", "i32", "i64", "f32", "f64"
_NP = {U8: np.uint8, I32: np.int32, I64: np.int64, F32: np.float32, F64: np.float64}
_TORCH = {U8: torch.uint8, I32: torch.int32, I64: torch.int64, F32: torch.float32,
          F64: torch.float64}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from pfrl_amd import _native

    _native.lib()  # fail loudly if the HIP library is missing
    return torch.device("cuda:0")


def _ops():
    from pfrl_amd import ops

    return ops


# ---------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------
def ref_states_u8(frames2d, refs, divisor):
    """frames2d u8 [F, fb], refs [M, k] -> f32 [M, k, fb]."""
    return frames2d[refs].astype(np.float32) / np.float32(divisor)


def ref_states_f32(frames2d, refs):
    return frames2d[refs]


def ref_states_nhwc4(frames2d, refs, divisor, hw):
    """refs [M, 4] -> f32 [M, H, W, 4]."""
    M = refs.shape[0]
    return np.ascontiguousarray(ref_states_u8(frames2d, refs, divisor).transpose(0, 2, 1)).reshape(
        M, hw[0], hw[1], 4)


def ref_raw_nhwc4(frames2d, refs, hw):
    """refs [M, 4] -> u8 [M, H, W, 4]."""
    M = refs.shape[0]
    return np.stack([frames2d[refs[:, c]] for c in range(4)], axis=-1).reshape(M, hw[0], hw[1], 4)


def gamma_pow(gamma, n):
    return [gamma ** i for i in range(n + 1)]


def ref_nstep(e_tids, e_len, slots, t_reward, t_term, gp):
    """The n-step collapse of the sampled entries ``slots``: dict of reward / is_state_terminal /
    discount (f32) and the first / last transition id of every entry."""
    gp = np.asarray(gp, dtype=np.float64)
    tids = e_tids[slots].astype(np.int64)
    lens = e_len[slots].astype(np.int64)
    B, n = tids.shape
    acc = np.zeros(B, dtype=np.float64)
    any_t = np.zeros(B, dtype=bool)
    for i in range(n):
        live = i < lens
        t = np.where(live, tids[:, i], 0)
        term = gp[i] * t_reward[t]              # one rounding
        acc = np.where(live, acc + term, acc)   # one rounding, in transition order
        any_t |= live & (t_term[t] != 0)
    rows = np.arange(B)
    return dict(reward=acc.astype(np.float32), is_state_terminal=any_t.astype(np.float32),
                discount=gp[lens].astype(np.float32), first=tids[:, 0], last=tids[rows, lens - 1])


_M64 = (1 << 64) - 1
_MIX_A, _MIX_B = np.uint64(0xbf58476d1ce4e5b9), np.uint64(0x94d049bb133111eb)
_GOLDEN, _STRIDE = 0x9e3779b97f4a7c15, np.uint64(0xd1342543de82ef95)


def mix64(z):
    """The splitmix64 finaliser on a uint64 array (array arithmetic wraps modulo 2^64)."""
    z = np.atleast_1d(np.asarray(z, dtype=np.uint64))
    z = (z ^ (z >> np.uint64(30))) * _MIX_A
    z = (z ^ (z >> np.uint64(27))) * _MIX_B
    return z ^ (z >> np.uint64(31))


def ref_synth_frame(frame_bytes, seed, env_id, step):
    """One synthetic frame (u8 [frame_bytes]) of env ``env_id`` at ``step``."""
    inner = ((env_id & _M64) * _GOLDEN + (step & _M64)) & _M64
    key = mix64(np.uint64(seed & _M64) ^ mix64(np.uint64(inner)))
    words = (frame_bytes + 7) // 8                  # a 4-byte tail takes the low half of one more
    r = mix64(key + np.arange(words, dtype=np.uint64) * _STRIDE)
    return r.astype("<u8").view(np.uint8)[:frame_bytes].copy()


def ref_synth(store, slots, seed, env_id0, step):
    """``store`` u8 [F, fb] with frame f of the batch written to slots[f], in launch order."""
    out = store.copy()
    for f, s in enumerate(slots):
        out[int(s)] = ref_synth_frame(store.shape[1], seed, env_id0 + f, step)
    return out


# ---------------------------------------------------------------------------
# guarded buffers
# ---------------------------------------------------------------------------
def _bits(a):
    """Floats as the unsigned integers of their bit patterns; integers as they are."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.float32:
        return a.view(np.uint32)
    if a.dtype == np.float64:
        return a.view(np.uint64)
    return a


def assert_bits_equal(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype,
                                                                 got.shape, want.shape)
    np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=what)


def fill_pattern(kind, shape):
    """What a guarded buffer of this type holds before a launch, as a NumPy array."""
    if kind == F32:
        return np.full(shape, NAN_BITS, dtype=np.uint32).view(np.float32)
    n = int(np.prod(shape, dtype=np.int64)) * np.dtype(_NP[kind]).itemsize
    return np.full(n, 0xA5, dtype=np.uint8).view(_NP[kind]).reshape(shape)


class Guarded:
    """``shape`` elements of ``kind`` inside a larger device buffer: GUARD bytes of fill pattern on
    both sides, the payload 16-byte aligned and holding the fill pattern too (or ``init``)."""

    def __init__(self, dev, kind, shape, init=None):
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        self.kind, self.shape = kind, shape
        self.nbytes = int(np.prod(shape, dtype=np.int64)) * np.dtype(_NP[kind]).itemsize
        total = GUARD + (self.nbytes + 15) // 16 * 16 + GUARD
        if kind == F32:
            self.buf = torch.full((total // 4,), NAN_BITS, dtype=torch.int32,
                                  device=dev).view(torch.uint8)
        else:
            self.buf = torch.full((total,), 0xA5, dtype=torch.uint8, device=dev)
        self.pristine = self.buf.cpu().numpy().copy()
        self.t = self.buf[GUARD:GUARD + self.nbytes].view(_TORCH[kind]).view(shape)
        assert self.t.data_ptr() % 16 == 0 and self.t.is_contiguous()
        if init is not None:
            init = np.ascontiguousarray(init, dtype=_NP[kind]).reshape(shape)
            self.t.copy_(torch.from_numpy(init.copy()).to(dev))

    def channels_last(self):
        """The payload [M, H, W, 4] seen as the [M, 4, H, W] channels_last tensor."""
        return self.t.permute(0, 3, 1, 2)

    def check(self, want=None, what=""):
        """Guards intact; payload == ``want`` bit for bit (when given).  Returns the payload."""
        torch.cuda.synchronize()
        now = self.buf.cpu().numpy()
        end = GUARD + self.nbytes
        np.testing.assert_array_equal(now[:GUARD], self.pristine[:GUARD],
                                      err_msg="%s: write BEFORE the output" % what)
        np.testing.assert_array_equal(now[end:], self.pristine[end:],
                                      err_msg="%s: write PAST the output" % what)
        got = now[GUARD:end].view(_NP[self.kind]).reshape(self.shape)
        if want is not None:
            assert_bits_equal(got, np.asarray(want, dtype=_NP[self.kind]).reshape(self.shape), what)
        return got


def _T(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def distinct_frames(rs, F, fb):
    """u8 [F, fb]: (slot * 37 + pixel * 11 + noise[pixel]) & 0xff -- any two of the (fewer than 256)
    slots differ in EVERY pixel, so a swapped channel or shift cannot cancel out."""
    assert F < 256
    noise = rs.randint(0, 256, size=fb)
    slot = np.arange(F)[:, None]
    pix = np.arange(fb)[None, :]
    return ((slot * 37 + pix * 11 + noise[None, :]) & 0xff).astype(np.uint8)


def random_f32_bits(rs, shape):
    """f32 with arbitrary bit patterns (NaNs and denormals included): a copy must keep them."""
    return rs.randint(0, 1 << 32, size=shape, dtype=np.uint64).astype(np.uint32).view(np.float32)


def edge_refs(rs, F, M, k):
    """int32 [M, k] into F slots with slot 0, the last slot and a repeat among them."""
    refs = rs.randint(0, F, size=M * k).astype(np.int32)
    refs[-1] = F - 1
    if M * k >= 2:
        refs[0] = 0
    if M * k >= 4:
        refs[2] = refs[1]
    return refs.reshape(M, k)


# ---------------------------------------------------------------------------
# 1. batch_states, u8 planar
# ---------------------------------------------------------------------------
U8_FRAME_BYTES = [4, 8, 1020, 1024, 1028, 8188, 8192, 8196, 9216, 16388]
REF_SHAPES = [(1, 1), (255, 1), (64, 4), (257, 1)]          # M * k = 1, 255, 256, 257


@pytest.mark.parametrize("divisor", [255.0, 1.0])
@pytest.mark.parametrize("fb", U8_FRAME_BYTES)
def test_batch_states_u8(dev, fb, divisor):
    rs = np.random.RandomState(fb)
    F = 9
    frames = rs.randint(0, 256, size=(F, fb)).astype(np.uint8)
    d_frames = _T(dev, frames)
    for M, k in REF_SHAPES:
        refs = edge_refs(rs, F, M, k)
        out = Guarded(dev, F32, (M, k, fb))
        _ops().batch_states(d_frames, _T(dev, refs), divisor, out=out.t)
        out.check(ref_states_u8(frames, refs, divisor), "fb=%d M=%d k=%d" % (fb, M, k))


@pytest.mark.parametrize("divisor", [255.0, 1.0])
@pytest.mark.parametrize("n_refs", [910, 911])
def test_batch_states_u8_nontemporal_threshold(dev, n_refs, divisor):
    """9216-byte frames: 910 refs write 33 546 240 B (below kNtMinBytes = 33 554 432), 911 write
    33 583 104 B (the non-temporal instantiation)."""
    fb = 9216
    assert (910 * fb * 4 < 32 << 20) and (911 * fb * 4 >= 32 << 20)
    rs = np.random.RandomState(n_refs)
    F = 7
    frames = rs.randint(0, 256, size=(F, fb)).astype(np.uint8)
    refs = edge_refs(rs, F, n_refs, 1)
    out = Guarded(dev, F32, (n_refs, 1, fb))
    _ops().batch_states(_T(dev, frames), _T(dev, refs), divisor, out=out.t)
    out.check(ref_states_u8(frames, refs, divisor), "n_refs=%d" % n_refs)


# ---------------------------------------------------------------------------
# 2. batch_states, f32
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("fe,shapes", [
    (1, [(1, 1), (85, 3)]), (3, [(1, 1), (85, 3)]), (4, [(1, 1), (85, 3)]), (5, [(1, 1), (85, 3)]),
    (1023, [(1, 1), (85, 3)]), (1024, [(1, 1), (85, 3)]), (1025, [(1, 1), (85, 3)]),
    # the 2048-workgroup cap: 524 544 uint4 items / 524 800 dword items > 2048 * 256 = 524 288, so
    # the grid-stride loop takes a second trip
    (1024, [(2049, 1)]), (1025, [(512, 1)])])
def test_batch_states_f32(dev, fe, shapes):
    rs = np.random.RandomState(fe)
    F = 9
    frames = random_f32_bits(rs, (F, fe))
    d_frames = _T(dev, frames)
    for M, k in shapes:
        refs = edge_refs(rs, F, M, k)
        out = Guarded(dev, F32, (M, k, fe))
        _ops().batch_states(d_frames, _T(dev, refs), out=out.t)
        out.check(ref_states_f32(frames, refs), "fe=%d M=%d k=%d" % (fe, M, k))


# ---------------------------------------------------------------------------
# 3. batch_states channels-last (k = 4) and batch_states_raw_nhwc4
# ---------------------------------------------------------------------------
# frame bytes -> frame shape ((H, W) or (1, H, W): what ops._spatial_hw admits): fewer pixels than one
# 1024-pixel tile, exactly one, one plus a single dword, two, a ragged last tile, nine
NHWC_SHAPES = {4: (2, 2), 16: (4, 4), 1020: (30, 34), 1024: (32, 32), 1028: (4, 257),
               2048: (1, 32, 64), 7056: (1, 84, 84), 9216: (96, 96)}


def _nhwc_case(rs, fb, n_obs):
    fshape = NHWC_SHAPES[fb]
    assert int(np.prod(fshape)) == fb
    F = 11
    frames = distinct_frames(rs, F, fb)
    refs = edge_refs(rs, F, n_obs, 4)
    refs[0] = [0, 3, 7, F - 1]                 # four different frames: slot 0 and the last slot
    if n_obs >= 2:
        refs[1, :] = 5                         # one observation whose four refs are the same frame
    if n_obs >= 3:
        refs[2] = [9, 2, 4, 2]                 # a repeat two channels apart
    return fshape, fshape[-2:], frames, refs


@pytest.mark.parametrize("divisor", [255.0, 1.0])
@pytest.mark.parametrize("n_obs", [1, 3])
@pytest.mark.parametrize("fb", sorted(NHWC_SHAPES))
def test_batch_states_nhwc4(dev, fb, n_obs, divisor):
    ops = _ops()
    rs = np.random.RandomState(fb + n_obs)
    fshape, hw, frames, refs = _nhwc_case(rs, fb, n_obs)
    d_frames = _T(dev, frames.reshape((-1,) + fshape))
    assert ops.channels_last_supported(d_frames, 4)
    out = Guarded(dev, F32, (n_obs, hw[0], hw[1], 4))
    got = ops.batch_states_nhwc4(d_frames, _T(dev, refs), divisor, out=out.channels_last())
    assert got.shape == (n_obs, 4) + hw
    out.check(ref_states_nhwc4(frames, refs, divisor, hw), "fb=%d n_obs=%d" % (fb, n_obs))


@pytest.mark.parametrize("n_obs", [1, 3])
@pytest.mark.parametrize("fb", sorted(NHWC_SHAPES))
def test_batch_states_raw_nhwc4(dev, fb, n_obs):
    ops = _ops()
    rs = np.random.RandomState(fb + n_obs)
    fshape, hw, frames, refs = _nhwc_case(rs, fb, n_obs)
    d_frames = _T(dev, frames.reshape((-1,) + fshape))
    out = Guarded(dev, U8, (n_obs, hw[0], hw[1], 4))
    px = ops.batch_states_raw_nhwc4(d_frames, _T(dev, refs), 255.0, out=out.t)
    assert px.data.data_ptr() == out.t.data_ptr() and px.divisor == 255.0
    out.check(ref_raw_nhwc4(frames, refs, hw), "fb=%d n_obs=%d" % (fb, n_obs))


@pytest.mark.parametrize("divisor", [255.0, 1.0])
@pytest.mark.parametrize("n_obs", [227, 228])
def test_batch_states_nhwc4_nontemporal_threshold(dev, n_obs, divisor):
    """9216-byte frames: 227 observations write 33 472 512 B, 228 write 33 619 968 B >= 32 MiB."""
    ops = _ops()
    fb, hw = 9216, (96, 96)
    assert (227 * 16 * fb < 32 << 20) and (228 * 16 * fb >= 32 << 20)
    rs = np.random.RandomState(n_obs)
    F = 11
    frames = distinct_frames(rs, F, fb)
    refs = edge_refs(rs, F, n_obs, 4)
    d_frames, d_refs = _T(dev, frames.reshape((F,) + hw)), _T(dev, refs)
    out = Guarded(dev, F32, (n_obs, hw[0], hw[1], 4))
    ops.batch_states_nhwc4(d_frames, d_refs, divisor, out=out.channels_last())
    out.check(ref_states_nhwc4(frames, refs, divisor, hw), "float n_obs=%d" % n_obs)
    raw = Guarded(dev, U8, (n_obs, hw[0], hw[1], 4))
    ops.batch_states_raw_nhwc4(d_frames, d_refs, divisor, out=raw.t)
    raw.check(ref_raw_nhwc4(frames, refs, hw), "raw n_obs=%d" % n_obs)


# ---------------------------------------------------------------------------
# the transition table and the entry ring
# ---------------------------------------------------------------------------
SPARE = 5         # table rows / entry slots that are never appended and must stay as they were
LENS_MODES, TERM_MODES, REWARD_MODES = ["one", "full", "mixed"], ["first", "last", "none"], \
    ["cancel", "gamma099", "gamma1"]


def big_actions(rs, shape):
    """int64 actions, every second one above 2^31 (up to 2^62), some negative."""
    a = rs.randint(0, 1 << 62, size=shape, dtype=np.int64)
    a[..., ::2] |= np.int64(1) << 31
    a[..., 1::5] *= -1
    return a


def awkward_rewards(rs, n):
    """f64 rewards no f32 holds: random mantissas over 40 binades, 1 / 3, 1e16 + 2, a denormal."""
    r = rs.randn(n) * np.exp2(rs.randint(-20, 20, size=n).astype(np.float64))
    r[::7] = 1.0 / 3.0
    r[3::11] = 1e16 + 2.0
    r[5::13] = 5e-324
    assert (r.astype(np.float32).astype(np.float64) != r).mean() > 0.8
    return r


class Table:
    """Host truth and guarded device columns of one transition table + entry ring.

    ``E`` entries of ``n`` slots each own ``n`` table rows of their own (entry e, step i -> logical
    row e * n + i), so length, terminal position and rewards are set per entry; logical rows and
    entries are placed at permuted slots of columns that are SPARE longer than needed."""

    def __init__(self, dev, rs, E, F, k, n, act_dim, lens="mixed", term="mixed", reward="gamma099",
                 ring=False):
        self.dev, self.E, self.F, self.k, self.n, self.act_dim = dev, E, F, k, n, act_dim
        R = E * n
        self.R, self.Rcap, self.Ecap = R, R + SPARE, E if ring else E + SPARE
        self.gamma = 0.99 if reward == "gamma099" else 1.0
        self.gp = gamma_pow(self.gamma, n)
        # --- what is appended, in logical order
        if lens == "one":
            e_len = np.ones(E, dtype=np.int32)
        elif lens == "full":
            e_len = np.full(E, n, dtype=np.int32)
        else:
            e_len = rs.randint(1, n + 1, size=E).astype(np.int32)
            e_len[0], e_len[-1] = n, 1
        state_ref = rs.randint(0, F, size=(R, k)).astype(np.int32)
        next_ref = rs.randint(0, F, size=(R, k)).astype(np.int32)
        state_ref[0, 0], next_ref[0, 0] = 0, F - 1
        action = (big_actions(rs, R) if act_dim == 0
                  else rs.randn(R, act_dim).astype(np.float32))
        rew = awkward_rewards(rs, R)
        if reward == "cancel" and n >= 3:
            # 1e16 + 1.0 rounds back to 1e16 in f64, so the sum in transition order is 0.0; adding
            # the two large terms first gives 1.0
            for e in range(0, E, 3):
                if e_len[e] >= 3:
                    rew[e * n:e * n + e_len[e]] = 0.0
                    rew[e * n:e * n + 3] = [1e16, 1.0, -1e16]
        term_col = np.zeros(R, dtype=np.uint8)
        for e in range(E):
            if term == "first":
                term_col[e * n] = 1
            elif term == "last":
                term_col[e * n + e_len[e] - 1] = 1
            elif term == "mixed":
                term_col[e * n:(e + 1) * n] = rs.rand(n) < 0.15
        if term in ("first", "last"):
            term_col[::4] *= np.uint8(2)          # any non-zero byte is a terminal
        # --- where it goes
        self.row_slot = rs.permutation(self.Rcap)[:R].astype(np.int32)     # logical row -> slot
        # logical entry -> slot (ring: the entry ring of batch_episodes, entry e at position e)
        self.ent_slot = (np.arange(E, dtype=np.int32) if ring
                         else rs.permutation(self.Ecap)[:E].astype(np.int32))
        tids = -np.ones((E, n), dtype=np.int32)
        for e in range(E):
            tids[e, :e_len[e]] = self.row_slot[e * n:e * n + e_len[e]]
        self.app = dict(state_ref=state_ref, next_ref=next_ref, action=action, reward=rew,
                        terminal=term_col, tids=tids, lens=e_len)
        # --- the columns: the fill pattern where nothing is appended
        ashape = (self.Rcap,) if act_dim == 0 else (self.Rcap, act_dim)
        self.akind = I64 if act_dim == 0 else F32
        self.kinds = dict(t_state_ref=(I32, (self.Rcap, k)), t_next_ref=(I32, (self.Rcap, k)),
                          t_action=(self.akind, ashape), t_reward=(F64, (self.Rcap,)),
                          t_terminal=(U8, (self.Rcap,)), e_tids=(I32, (self.Ecap, n)),
                          e_len=(I32, (self.Ecap,)))
        self.host = {c: fill_pattern(kd, sh).copy() for c, (kd, sh) in self.kinds.items()}
        self.cols = {c: Guarded(dev, kd, sh) for c, (kd, sh) in self.kinds.items()}
        self.desc = _ops().make_table_desc(*[self.cols[c].t for c in (
            "t_state_ref", "t_next_ref", "t_action", "t_reward", "t_terminal", "e_tids", "e_len")],
            k, n, act_dim)

    def append(self, chunks=1):
        """Through ``table_append`` / ``entries_append``, in ``chunks`` launches; the host truth
        follows."""
        ops, a, dev = _ops(), self.app, self.dev
        for part in np.array_split(np.arange(self.R), chunks):
            s = self.row_slot[part]
            ops.table_append(self.desc, _T(dev, s), _T(dev, a["state_ref"][part]),
                             _T(dev, a["next_ref"][part]), _T(dev, a["action"][part]),
                             _T(dev, a["reward"][part]), _T(dev, a["terminal"][part]))
            self.host["t_state_ref"][s] = a["state_ref"][part]
            self.host["t_next_ref"][s] = a["next_ref"][part]
            self.host["t_action"][s] = a["action"][part]
            self.host["t_reward"][s] = a["reward"][part]
            self.host["t_terminal"][s] = a["terminal"][part]
        for part in np.array_split(np.arange(self.E), chunks):
            s = self.ent_slot[part]
            ops.entries_append(self.desc, _T(dev, s), _T(dev, a["tids"][part]),
                               _T(dev, a["lens"][part]))
            self.host["e_tids"][s] = a["tids"][part]
            self.host["e_len"][s] = a["lens"][part]

    def check_columns(self, what=""):
        """Every column WHOLE (rows and entries never appended still hold the fill pattern) and its
        guards."""
        for c in self.cols:
            self.cols[c].check(self.host[c], "%s column %s" % (what, c))

    def outputs(self, rows, state_kind_shape):
        """Guarded output dict of batch_experiences / batch_episodes for ``rows`` rows."""
        ashape = (rows,) if self.act_dim == 0 else (rows, self.act_dim)
        return dict(state=Guarded(self.dev, F32, state_kind_shape),
                    next_state=Guarded(self.dev, F32, state_kind_shape),
                    action=Guarded(self.dev, self.akind, ashape),
                    reward=Guarded(self.dev, F32, (rows,)),
                    is_state_terminal=Guarded(self.dev, F32, (rows,)),
                    discount=Guarded(self.dev, F32, (rows,)))


# ---------------------------------------------------------------------------
# 4. table_append / entries_append
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("k,n,act_dim", [(1, 1, 0), (4, 3, 1), (8, 16, 3), (4, 16, 17), (8, 1, 0),
                                         (1, 3, 17)])
@pytest.mark.parametrize("rows", [1, 255, 256, 257])
def test_table_and_entries_append(dev, rows, k, n, act_dim):
    """``rows`` table rows in ONE table_append launch and ``rows`` entries in ONE entries_append
    launch, at permuted slots; every column compared whole and bit for bit (f64 rewards no f32
    holds, int64 actions above 2^31, strided float action rows)."""
    rs = np.random.RandomState(rows * 100 + k * 10 + n)
    ops = _ops()
    # (rows entries bring rows * n table rows; this test appends the first `rows` of them)
    tab = Table(dev, rs, E=rows, F=50, k=k, n=n, act_dim=act_dim)
    a = tab.app
    # --- `rows` rows of the row columns in one launch (the first `rows` logical rows)
    part = np.arange(rows)
    s = tab.row_slot[part]
    ops.table_append(tab.desc, _T(dev, s), _T(dev, a["state_ref"][part]),
                     _T(dev, a["next_ref"][part]), _T(dev, a["action"][part]),
                     _T(dev, a["reward"][part]), _T(dev, a["terminal"][part]))
    for c, key in (("t_state_ref", "state_ref"), ("t_next_ref", "next_ref"), ("t_action", "action"),
                   ("t_reward", "reward"), ("t_terminal", "terminal")):
        tab.host[c][s] = a[key][part]
    # --- `rows` entries in one launch
    ops.entries_append(tab.desc, _T(dev, tab.ent_slot), _T(dev, a["tids"]), _T(dev, a["lens"]))
    tab.host["e_tids"][tab.ent_slot] = a["tids"]
    tab.host["e_len"][tab.ent_slot] = a["lens"]
    tab.check_columns("rows=%d k=%d n=%d act_dim=%d" % (rows, k, n, act_dim))
    if act_dim == 0:
        assert (np.abs(tab.host["t_action"][s]) > 1 << 31).any()


# ---------------------------------------------------------------------------
# 5. - 7. batch_experiences
# ---------------------------------------------------------------------------
def pairwise_cover(factors, ok, seed=0):
    """A selection of the product of ``factors`` (dict name -> levels) restricted to ``ok(case)`` in
    which every pair of levels that some admissible case combines occurs together at least once
    (greedy, deterministic)."""
    names = list(factors)
    every = [dict(zip(names, c)) for c in itertools.product(*[factors[m] for m in names])]
    every = [c for c in every if ok(c)]
    pairs = lambda c: {((a, c[a]), (b, c[b])) for a, b in itertools.combinations(names, 2)}  # noqa: E731
    todo = set().union(*[pairs(c) for c in every])
    rng = random.Random(seed)
    chosen = []
    while todo:
        cand = rng.sample(every, min(len(every), 300))
        best = max(cand, key=lambda c: len(pairs(c) & todo))
        if not pairs(best) & todo:
            best = next(c for c in every if pairs(c) & todo)
        chosen.append(best)
        todo -= pairs(best)
    return chosen, every


def case_id(c):
    return "-".join("x".join(str(x) for x in v) if isinstance(v, tuple) else str(v)
                    for v in c.values())


def case_seed(c):
    return zlib.crc32(case_id(c).encode())


# frame: ("u8", bytes) or ("f32", elements)
BE_FACTORS = dict(
    mode=["u8/255", "u8/1", "f32"], act_dim=[0, 1, 3, 17], kn=[(1, 1), (4, 3), (8, 16), (2, 16)],
    B=[1, 255, 256, 257],
    frame=[("u8", 1024), ("u8", 7056), ("u8", 9216), ("f32", 5), ("f32", 17), ("f32", 24),
           ("f32", 376)],
    lens=LENS_MODES, term=TERM_MODES, reward=REWARD_MODES)


def _be_ok(c):
    if (c["mode"] == "f32") != (c["frame"][0] == "f32"):
        return False
    out_bytes = c["B"] * c["kn"][0] * c["frame"][1] * 4
    return out_bytes <= 34 << 20                    # one output tensor: as large as the NT cases


BE_CASES, _BE_EVERY = pairwise_cover(BE_FACTORS, _be_ok)


def _divisor(mode):
    return {"u8/255": 255.0, "u8/1": 1.0, "f32": 255.0}[mode]       # (f32 frames ignore it)


def run_batch_experiences(dev, rs, mode, act_dim, k, n, B, frame, lens, term, reward, E=40, F=23,
                          hw=None):
    """One launch on a fresh table; everything it writes against NumPy.  ``hw`` (u8, k == 4): the
    channels-last form, out[B][H][W][4]."""
    ops = _ops()
    u8 = frame[0] == "u8"
    fe = frame[1]
    frames = distinct_frames(rs, F, fe) if u8 else random_f32_bits(rs, (F, fe))
    tab = Table(dev, rs, E, F, k, n, act_dim, lens, term, reward)
    tab.append(chunks=2)
    tab.check_columns("append")
    # sampled entries: logical 0 (the full / cancelling one) and E - 1 among them, with repeats
    pick = rs.randint(0, E, size=B)
    pick[0] = 0
    pick[-1:] = E - 1 if B > 1 else 0
    slots = tab.ent_slot[pick].astype(np.int32)
    sshape = (B, hw[0], hw[1], 4) if hw else (B, k, fe)
    out = tab.outputs(B, sshape)
    d_frames = _T(dev, frames.reshape((F,) + tuple(hw)) if hw else frames)
    tensors = {key: (g.channels_last() if hw and key in ("state", "next_state") else g.t)
               for key, g in out.items()}
    ops.batch_experiences(tab.desc, d_frames, _divisor(mode), _T(dev, slots), tab.gp, tensors)
    h = tab.host
    want = ref_nstep(h["e_tids"], h["e_len"], slots, h["t_reward"], h["t_terminal"], tab.gp)
    out["reward"].check(want["reward"], "reward")
    out["is_state_terminal"].check(want["is_state_terminal"], "is_state_terminal")
    out["discount"].check(want["discount"], "discount")
    out["action"].check(h["t_action"][want["first"]], "action")
    srefs, nrefs = h["t_state_ref"][want["first"]], h["t_next_ref"][want["last"]]
    if hw:
        ws = ref_states_nhwc4(frames, srefs, _divisor(mode), hw)
        wn = ref_states_nhwc4(frames, nrefs, _divisor(mode), hw)
    elif u8:
        ws, wn = ref_states_u8(frames, srefs, _divisor(mode)), ref_states_u8(frames, nrefs,
                                                                             _divisor(mode))
    else:
        ws, wn = ref_states_f32(frames, srefs), ref_states_f32(frames, nrefs)
    out["state"].check(ws, "state")
    out["next_state"].check(wn, "next_state")
    tab.check_columns("after the gather")           # a gather writes nothing into the table
    return tab, want


@pytest.mark.parametrize("c", BE_CASES, ids=case_id)
def test_batch_experiences_planar(dev, c):
    rs = np.random.RandomState(case_seed(c))
    tab, want = run_batch_experiences(dev, rs, c["mode"], c["act_dim"], c["kn"][0], c["kn"][1],
                                      c["B"], c["frame"], c["lens"], c["term"], c["reward"])
    if c["reward"] == "cancel" and c["kn"][1] >= 3 and c["lens"] != "one":
        assert want["reward"][0] == 0.0              # the 1e16, 1.0, -1e16 entry is in the batch


# (B, elements): k = 1, n = 3, mixed lengths
F32_SMALL = [(2048, 4),      # nv = 1
             (2047, 4),      # 2 B k = 4094: just below the switch, the generic kernel
             (2049, 376),    # nv = 94; 4098 frames: two idle waves in the last workgroup; 9 scalar
                             # workgroups
             (2048, 512),    # nv = 128
             (2048, 516),    # nv = 129: a second trip with one live lane
             (2048, 2048),   # 8192 B, the upper bound
             (2048, 2052)]   # 8208 B: back to the generic kernel


@pytest.mark.parametrize("act_dim", [0, 17])
@pytest.mark.parametrize("B,fe,k", [(b, e, 1) for b, e in F32_SMALL] + [(513, 24, 4)])
def test_batch_experiences_f32_small(dev, B, fe, k, act_dim):
    """Both sides of every condition that selects ``k_batch_experiences_f32_small`` and every trip
    and tail inside it; (513, 24, k = 4): 2 B k = 4104."""
    rs = np.random.RandomState(B + fe)
    run_batch_experiences(dev, rs, "f32", act_dim, k, 3, B, ("f32", fe), "mixed", "mixed",
                          "gamma099", E=300, F=37)


BE_NHWC_FACTORS = dict(mode=["u8/255", "u8/1"], act_dim=[0, 1, 3, 17], n=[1, 3, 16], B=[1, 257],
                       frame=[("u8", 1020), ("u8", 1028), ("u8", 7056)], lens=LENS_MODES,
                       term=TERM_MODES, reward=REWARD_MODES)
BE_NHWC_CASES, _BE_NHWC_EVERY = pairwise_cover(BE_NHWC_FACTORS, lambda c: True, seed=1)


@pytest.mark.parametrize("c", BE_NHWC_CASES, ids=case_id)
def test_batch_experiences_nhwc4(dev, c):
    """The channels-last launch (scalar workgroups first, 1024-pixel tiles) against NumPy."""
    rs = np.random.RandomState(case_seed(c))
    hw = NHWC_SHAPES[c["frame"][1]][-2:]
    run_batch_experiences(dev, rs, c["mode"], c["act_dim"], 4, c["n"], c["B"], c["frame"],
                          c["lens"], c["term"], c["reward"], hw=hw)


# ---------------------------------------------------------------------------
# 8. batch_episodes, called directly
# ---------------------------------------------------------------------------
def _episode_sets():
    rs = np.random.RandomState(40)
    twenty = np.sort(rs.randint(1, 41, size=20))[::-1].copy()
    twenty[0] = 40
    assert twenty.sum() > 256
    return {"5-3-3-1": [5, 3, 3, 1], "single": [1], "twenty": [int(x) for x in twenty]}


EPISODE_SETS = _episode_sets()


@pytest.mark.parametrize("k", [1, 4])
@pytest.mark.parametrize("act_dim", [0, 3])
@pytest.mark.parametrize("mode", ["u8/255", "u8/1", "f32"])
@pytest.mark.parametrize("lens_id", sorted(EPISODE_SETS))
def test_batch_episodes(dev, lens_id, mode, act_dim, k):
    """Windows sorted by descending length over a ring of E one-transition entries, the first two
    placed at the end of the ring so that ``ep_first + step`` wraps past E: episode-major states,
    time-major packed scalars, discount == float32(gamma)."""
    ops = _ops()
    rs = np.random.RandomState(len(lens_id) * 7 + k)
    lens = np.array(EPISODE_SETS[lens_id], dtype=np.int64)
    E, F, gamma = 64, 19, 0.97
    u8 = mode != "f32"
    fe = 1028 if u8 else (5 if k == 1 else 24)           # f32: the dword and the uint4 copy
    frames = distinct_frames(rs, F, fe) if u8 else random_f32_bits(rs, (F, fe))
    n = 1 if k == 1 else 3                                # (only an entry's first id is read)
    tab = Table(dev, rs, E, F, k, n, act_dim, "one", "mixed", ring=True)
    tab.append()
    tab.check_columns("append")
    n_eps = len(lens)
    first = rs.randint(0, E, size=n_eps)
    first[0] = E - 2 if lens[0] > 1 else E - 1            # steps 2.. of the longest window wrap
    if n_eps > 1:
        first[1] = E - 1
    # as DeviceReplay.fetch_episodes builds them
    rows, T = int(lens.sum()), int(lens[0])
    ep_first = (first % E).astype(np.int32)
    ep_row0 = np.zeros(n_eps + 1, dtype=np.int32)
    ep_row0[1:] = np.cumsum(lens)
    row_start = np.minimum(lens[None, :], np.arange(T + 1)[:, None]).sum(axis=1).astype(np.int32)
    assert row_start[T] == rows
    out = tab.outputs(rows, (rows, k, fe))
    ops.batch_episodes(tab.desc, _T(dev, frames), _divisor(mode), _T(dev, ep_first),
                       _T(dev, ep_row0), _T(dev, row_start), n_eps, T, rows, E, gamma,
                       {key: g.t for key, g in out.items()})
    h = tab.host
    # episode-major: episode by episode, step by step
    em = np.array([h["e_tids"][(ep_first[e] + i) % E, 0] for e in range(n_eps)
                   for i in range(lens[e])], dtype=np.int64)
    # time-major packed: step by step, every episode that is long enough, longest first
    tm = np.array([h["e_tids"][(ep_first[e] + t) % E, 0] for t in range(T) for e in range(n_eps)
                   if lens[e] > t], dtype=np.int64)
    assert len(em) == len(tm) == rows
    srefs, nrefs = h["t_state_ref"][em], h["t_next_ref"][em]
    if u8:
        ws, wn = ref_states_u8(frames, srefs, _divisor(mode)), ref_states_u8(frames, nrefs,
                                                                             _divisor(mode))
    else:
        ws, wn = ref_states_f32(frames, srefs), ref_states_f32(frames, nrefs)
    out["state"].check(ws, "state")
    out["next_state"].check(wn, "next_state")
    out["action"].check(h["t_action"][tm], "action")
    out["reward"].check(h["t_reward"][tm].astype(np.float32), "reward")
    out["is_state_terminal"].check((h["t_terminal"][tm] != 0).astype(np.float32), "terminal")
    out["discount"].check(np.full(rows, np.float32(gamma), dtype=np.float32), "discount")
    tab.check_columns("after the gather")


# ---------------------------------------------------------------------------
# 9. frames_scatter
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 8])
@pytest.mark.parametrize("fb", [4, 1020, 1024, 1028, 7056])
def test_frames_scatter(dev, fb, n):
    rs = np.random.RandomState(fb + n)
    F = 11
    store = rs.randint(0, 256, size=(F, fb)).astype(np.uint8)
    src = rs.randint(0, 256, size=(n, fb)).astype(np.uint8)
    slots = np.array([F - 1, 0, 3, 7, 4, 9, 2, 6][:n], dtype=np.int32)
    g = Guarded(dev, U8, (F, fb), init=store)
    _ops().frames_scatter(g.t, _T(dev, src), _T(dev, slots))
    want = store.copy()
    want[slots] = src
    g.check(want, "fb=%d n=%d" % (fb, n))


# ---------------------------------------------------------------------------
# 10. frames_synth_u8 and frames_synth_u8_ring against the NumPy generator
# ---------------------------------------------------------------------------
SYNTH_BYTES = [8, 12, 1028, 7056]            # 12 and 1028 have the 4-byte tail
SEED, ENV0, STEP = 0x9E3779B97F4A7C15 ^ 12345, 1000003, 77


@pytest.mark.parametrize("fb", SYNTH_BYTES)
def test_frames_synth_slot_list(dev, fb):
    """Odd slots (with a 12-byte frame: 8-byte stores at addresses 4 mod 8), slot 0 and the last;
    the whole store against the generator."""
    rs = np.random.RandomState(fb)
    F = 12
    store = rs.randint(0, 256, size=(F, fb)).astype(np.uint8)
    slots = np.array([1, 3, 11, 0, 7, 5], dtype=np.int32)
    g = Guarded(dev, U8, (F, fb), init=store)
    _ops().frames_synth_u8(g.t, _T(dev, slots), SEED, ENV0, STEP)
    g.check(ref_synth(store, slots, SEED, ENV0, STEP), "fb=%d" % fb)


@pytest.mark.parametrize("seq0,n", [(0, 12), (9, 7), (5, 1), (2 ** 40 + 3, 5), (2 ** 40 + 3, 12)],
                         ids=["all_slots", "wrap", "one", "seq_2^40", "seq_2^40_all"])
@pytest.mark.parametrize("fb", SYNTH_BYTES)
def test_frames_synth_ring(dev, fb, seq0, n):
    """n == n_slots, seq0 + n > n_slots, a sequence number above 2^40; and the ring form equals
    the slot-list form for the same (seed, env_id0, step)."""
    ops = _ops()
    rs = np.random.RandomState(fb + n)
    F = 12
    store = rs.randint(0, 256, size=(F, fb)).astype(np.uint8)
    slots = np.array([(seq0 + f) % F for f in range(n)], dtype=np.int32)
    want = ref_synth(store, slots, SEED, ENV0, STEP)
    ring = Guarded(dev, U8, (F, fb), init=store)
    ops.frames_synth_u8_ring(ring.t, seq0, n, SEED, ENV0, STEP)
    got_ring = ring.check(want, "ring fb=%d seq0=%d n=%d" % (fb, seq0, n))
    lst = Guarded(dev, U8, (F, fb), init=store)
    ops.frames_synth_u8(lst.t, _T(dev, slots), SEED, ENV0, STEP)
    np.testing.assert_array_equal(lst.check(want, "list"), got_ring)


# ---------------------------------------------------------------------------
# 11. select_actions
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("greedy_kind", [I32, I64])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_select_actions(dev, n, greedy_kind):
    rs = np.random.RandomState(n)
    if greedy_kind == I64:
        greedy = rs.randint(0, 18, size=n).astype(np.int64)
        greedy[::3] = 2 ** 40
        greedy[1::7] = -(2 ** 40) - 1
    else:
        greedy = rs.randint(1, 18, size=n).astype(np.int32)
        greedy[::3] = 2 ** 31 - 2
    choice = rs.choice(np.array([-1, -1, 0, 5, 2 ** 31 - 1], dtype=np.int64), size=n).astype(np.int32)
    if n >= 256:
        choice[254], choice[255] = -1, 2 ** 31 - 1        # the last lanes of the first workgroup
    choice[0] = -1
    choice[n // 2] = 0                                    # 0 is a chosen action, not "greedy"
    want = np.where(choice >= 0, choice.astype(np.int64), greedy.astype(np.int64))
    out = Guarded(dev, I64, (n,))
    got = _ops().select_actions(_T(dev, greedy), _T(dev, choice), out=out.t)
    assert got.data_ptr() == out.t.data_ptr()
    out.check(want, "n=%d" % n)
    assert want[n // 2] == 0 and (want[choice == 0] == 0).all() and (n == 1 or want[0] == greedy[0])
