"""The NumPy references of tests/test_gather_envelope.py against the committed C oracle
(oracle/pfrl_oracle.c), and the arithmetic its case lists rest on: no GPU needed."""
import os
import re

import numpy as np
import pytest

import oracle
from test_gather_envelope import (BE_CASES, BE_FACTORS, BE_NHWC_CASES, BE_NHWC_FACTORS, F32,
                                  F32_SMALL, NHWC_SHAPES, _BE_EVERY, _BE_NHWC_EVERY, _be_ok,
                                  awkward_rewards, distinct_frames, fill_pattern, gamma_pow, mix64,
                                  ref_nstep, ref_raw_nhwc4, ref_states_f32, ref_states_nhwc4,
                                  ref_states_u8, ref_synth_frame)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same_bits(a, b):
    assert a.dtype == b.dtype == np.float32 and a.shape == b.shape
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("divisor", [255.0, 1.0, 3.0])
@pytest.mark.parametrize("F,fb,M,k", [(1, 4, 1, 1), (256, 256, 256, 1), (9, 1028, 5, 4),
                                      (7, 7056, 3, 4), (5, 8196, 2, 8)])
def test_u8_reference_is_the_oracle(F, fb, M, k, divisor):
    rs = np.random.RandomState(fb)
    frames = rs.randint(0, 256, size=(F, fb)).astype(np.uint8)
    if F == 256:
        frames[:, 0] = np.arange(256)                 # every byte value
    refs = rs.randint(0, F, size=(M, k)).astype(np.int32)
    if F == 256:
        refs[:, 0] = np.arange(256)
    _same_bits(ref_states_u8(frames, refs, divisor), oracle.batch_states_u8(frames, refs, divisor))


@pytest.mark.parametrize("fb,n_obs", [(4, 1), (1028, 3), (7056, 2)])
def test_channels_last_references_are_the_oracle_transposed(fb, n_obs):
    rs = np.random.RandomState(fb)
    hw = NHWC_SHAPES[fb][-2:]
    frames = distinct_frames(rs, 11, fb)
    refs = rs.randint(0, 11, size=(n_obs, 4)).astype(np.int32)
    planar = oracle.batch_states_u8(frames, refs, 255.0)                  # [M, 4, fb]
    got = ref_states_nhwc4(frames, refs, 255.0, hw)
    assert got.shape == (n_obs,) + hw + (4,)
    raw = ref_raw_nhwc4(frames, refs, hw)
    assert raw.dtype == np.uint8 and raw.shape == got.shape
    for c in range(4):
        _same_bits(np.ascontiguousarray(got[..., c].reshape(n_obs, fb)),
                   np.ascontiguousarray(planar[:, c]))
        np.testing.assert_array_equal(raw[..., c].reshape(n_obs, fb), frames[refs[:, c]])
    # any two slots differ in every pixel
    assert all((frames[a] != frames[b]).all() for a in range(11) for b in range(a))


@pytest.mark.parametrize("fe,M,k", [(1, 1, 1), (5, 7, 3), (1025, 4, 2)])
def test_f32_reference_is_the_oracle(fe, M, k):
    rs = np.random.RandomState(fe)
    frames = rs.randn(9, fe).astype(np.float32)
    refs = rs.randint(0, 9, size=(M, k)).astype(np.int32)
    _same_bits(np.ascontiguousarray(ref_states_f32(frames, refs)),
               oracle.batch_states_f32(frames, refs))


@pytest.mark.parametrize("gamma", [0.99, 1.0])
@pytest.mark.parametrize("n", [1, 3, 16])
def test_nstep_reference_is_the_oracle(n, gamma):
    rs = np.random.RandomState(n)
    R, E, B = 400, 60, 300
    rewards = awkward_rewards(rs, R)
    term = (rs.rand(R) < 0.1).astype(np.uint8) * np.uint8(3)
    e_len = rs.randint(1, n + 1, size=E).astype(np.int32)
    e_len[0], e_len[1] = n, 1
    e_tids = -np.ones((E, n), dtype=np.int32)
    for e in range(E):
        e_tids[e, :e_len[e]] = rs.randint(0, R, size=e_len[e])
    if n >= 3:
        rewards[:3] = [1e16, 1.0, -1e16]
        e_tids[0, :3], e_len[0] = [0, 1, 2], 3
    slots = rs.randint(0, E, size=B).astype(np.int32)
    slots[0] = 0
    got = ref_nstep(e_tids, e_len, slots, rewards, term, gamma_pow(gamma, n))
    want = oracle.batch_experiences_scalars([list(e_tids[s, :e_len[s]]) for s in slots], rewards,
                                            term, gamma, n)
    for key in ("reward", "is_state_terminal", "discount"):
        _same_bits(got[key], want[key])
    np.testing.assert_array_equal(got["first"], want["first"])
    np.testing.assert_array_equal(got["last"], want["last"])
    if n >= 3 and gamma == 1.0:
        assert got["reward"][0] == 0.0 and (1e16 + -1e16) + 1.0 == 1.0      # order matters


def test_mix64_is_the_splitmix64_finaliser():
    # splitmix64 seeded with 0: state += 0x9e3779b97f4a7c15, output = finaliser(state); the first
    # three outputs of the published generator
    want = [0xe220a8397b1dcdaf, 0x6e789e6aa1b965f4, 0x06c45d188009454f]
    state = np.uint64(0x9e3779b97f4a7c15) * np.arange(1, 4, dtype=np.uint64)
    assert [int(x) for x in mix64(state)] == want


def test_synthetic_frame_layout():
    a16, a12, a8 = (ref_synth_frame(fb, 7, 3, 5) for fb in (16, 12, 8))
    np.testing.assert_array_equal(a12, a16[:12])           # the tail = low half of the next word
    np.testing.assert_array_equal(a8, a16[:8])
    assert a12.dtype == np.uint8 and len(a12) == 12
    assert not np.array_equal(ref_synth_frame(16, 7, 4, 5), a16)      # env
    assert not np.array_equal(ref_synth_frame(16, 7, 3, 6), a16)      # step
    assert not np.array_equal(ref_synth_frame(16, 8, 3, 5), a16)      # seed
    big = ref_synth_frame(7056, 7, 3, 5)
    assert len(np.unique(big)) == 256 and 120 < big.mean() < 135


def test_fill_pattern_is_a_nan_no_conversion_produces():
    assert np.isnan(fill_pattern(F32, (3,))).all()
    assert (fill_pattern("i32", (2,)).view(np.uint8) == 0xA5).all()


def _pairs(c):
    names = list(c)
    return {((a, c[a]), (b, c[b])) for i, a in enumerate(names) for b in names[i + 1:]}


@pytest.mark.parametrize("cases,every,factors", [(BE_CASES, _BE_EVERY, BE_FACTORS),
                                                 (BE_NHWC_CASES, _BE_NHWC_EVERY, BE_NHWC_FACTORS)],
                         ids=["planar", "nhwc4"])
def test_batch_experiences_selection_is_pairwise_covering(cases, every, factors):
    """Every pair of levels that some admissible case combines occurs in the selection, and every
    level of every factor occurs."""
    need = set().union(*[_pairs(c) for c in every])
    have = set().union(*[_pairs(c) for c in cases])
    assert need <= have
    for name, levels in factors.items():
        assert {c[name] for c in cases} == set(levels)
    assert all(c in every for c in cases) and len(cases) < len(every) // 50


def test_case_arithmetic():
    """The sizes the case lists claim to cross."""
    assert all(_be_ok(c) for c in BE_CASES)
    assert 1024 // 4 * 2049 == 524544 > 2048 * 256 and 1025 * 512 == 524800 > 2048 * 256
    assert 910 * 9216 * 4 == 33546240 < 32 << 20 <= 911 * 9216 * 4 == 33583104
    assert 227 * 16 * 9216 < 32 << 20 <= 228 * 16 * 9216
    assert all(int(np.prod(s)) == fb for fb, s in NHWC_SHAPES.items())
    switch = [(b, e) for b, e in F32_SMALL if e * 4 % 16 == 0 and e * 4 <= 8192 and 2 * b >= 4096]
    assert switch == [(2048, 4), (2049, 376), (2048, 512), (2048, 516), (2048, 2048)]
    hdr = open(os.path.join(ROOT, "include", "pfrl_amd.h")).read()
    assert int(re.search(r"#define PFRL_MAX_STACK (\d+)", hdr).group(1)) == 8 == max(
        k for k, _ in BE_FACTORS["kn"])
    assert int(re.search(r"#define PFRL_MAX_NSTEP (\d+)", hdr).group(1)) == 16 == max(
        n for _, n in BE_FACTORS["kn"])
