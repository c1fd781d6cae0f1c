"""The prioritized-replay trees restated in NumPy, pinned to the committed C oracle, and the case
lists of tests/test_sumtree_envelope.py with the proof that they reach what they claim: no GPU.

The restatement follows the reference's semantics (pfrl/collections/prioritized.py:135-323): a node
is a pure function of its two children -- the sum ``((0 + left) + right)`` over the children
present, the min ``left unless right < left`` -- on NEP-50 typed scalars (Python float, np.float32,
np.float64, absent).  Every claim about which route of csrc/sumtree.hip a case takes is computed
from this model and from host restatements of the kernels' GATES (the constants below and
``path_hash``); none comes from running a kernel.
"""
import collections
import copy
import functools

import numpy as np
import pytest

import oracle
from pfrl_amd.collections.tree_frame import TreeFrame

ABSENT, PY, F32, F64 = 0, 1, 2, 3
MAX_LEVELS = 40

# the gates of csrc/sumtree.hip
K_BOT_LEVELS = 9        # kBotLevels: level of the bottom subtrees' roots
K_MAX_TOP_LOG2 = 13     # kMaxTopLog2: the LDS top heap holds at most 13 levels
K_FAST_THREADS = 128    # kFastThreads: largest launch of the hashed repair
K_FAST_LEVELS = 22      # kFastLevels: largest frame of the hashed repair
K_MAX_BATCH = 1024      # kMaxBatch

SENT_V, SENT_T = -7.25, 0x5A    # ring slots outside the frame
SHIFT = 1 << 40                 # translation of a frame: a multiple of every ring length


# ---------------------------------------------------------------------------------------------
# typed scalars
# ---------------------------------------------------------------------------------------------
def s_add(a, b):
    t = max(a[1], b[1])
    if t == F32:
        return float(np.float32(a[0]) + np.float32(b[0])), t
    return float(np.float64(a[0]) + np.float64(b[0])), t


def s_sub(a, b):
    t = max(a[1], b[1])
    if t == F32:
        return float(np.float32(a[0]) - np.float32(b[0])), t
    return float(np.float64(a[0]) - np.float64(b[0])), t


def s_div(a, b):
    t = max(a[1], b[1])
    with np.errstate(all="ignore"):
        if t == F32:
            return float(np.float32(a[0]) / np.float32(b[0])), t
        return float(np.float64(a[0]) / np.float64(b[0])), t


def s_lt(a, b):
    if max(a[1], b[1]) == F32:
        return bool(np.float32(a[0]) < np.float32(b[0]))
    return bool(a[0] < b[0])


ZERO = (0.0, PY)            # the int 0 of sum(), the 0.0 of an absent left child and of _write(ix, 0.0)
NONE = (0.0, ABSENT)


def reduce_sum(a, b):
    """_reduce with op=sum: ((0 + left) + right) over the children present."""
    if a[1] == ABSENT and b[1] == ABSENT:
        return NONE
    acc = ZERO
    if a[1] != ABSENT:
        acc = s_add(acc, a)
    if b[1] != ABSENT:
        acc = s_add(acc, b)
    return acc


def reduce_min(a, b):
    """_reduce with op=min: the first of the smallest."""
    if a[1] == ABSENT:
        return b if b[1] != ABSENT else NONE
    if b[1] == ABSENT:
        return a
    return b if s_lt(b, a) else a


def v_add(av, at, bv, bt):
    t = np.maximum(at, bt)
    r32 = (av.astype(np.float32) + bv.astype(np.float32)).astype(np.float64)
    return np.where(t == F32, r32, av + bv), t


def v_lt(av, at, bv, bt):
    return np.where(np.maximum(at, bt) == F32, av.astype(np.float32) < bv.astype(np.float32), av < bv)


def build_levels(v, t, which):
    """Every level of one tree from its leaves, bottom-up and vectorised: [(values, tags)] with
    level l at index l, nodes in frame order; an absent node is (0.0, ABSENT)."""
    v = np.where(t == ABSENT, 0.0, np.asarray(v, dtype=np.float64))
    t = np.asarray(t, dtype=np.uint8)
    levels = [(v, t)]
    while len(v) > 1:
        lv, lt, rv, rt = v[0::2], t[0::2], v[1::2], t[1::2]
        lp, rp = lt != ABSENT, rt != ABSENT
        if which == 0:
            zv, zt = np.zeros_like(lv), np.full_like(lt, PY)
            av, at = v_add(zv, zt, lv, lt)                 # 0 + left
            bv, bt = v_add(av, at, rv, rt)                 # (0 + left) + right
            cv, ct = v_add(zv, zt, rv, rt)                 # 0 + right
        else:
            av, at, cv, ct = lv, lt, rv, rt
            right = v_lt(rv, rt, lv, lt)
            bv, bt = np.where(right, rv, lv), np.where(right, rt, lt)
        v = np.where(lp & rp, bv, np.where(lp, av, np.where(rp, cv, 0.0)))
        t = np.where(lp & rp, bt, np.where(lp, at, np.where(rp, ct, ABSENT))).astype(np.uint8)
        levels.append((v, t))
    return levels


# ---------------------------------------------------------------------------------------------
# the two trees over one frame
# ---------------------------------------------------------------------------------------------
Step = collections.namedtuple("Step", "level pt lt lt_kids tie right")   # one level of _find


class Trees:
    """Sum tree (which = 0) and min tree (which = 1) over ``frame``, every level in frame order,
    ``max_priority`` beside them.  ``dirty`` logs every node store as (which, level, node)."""

    def __init__(self, frame, sum_leaves=None, min_leaves=None, maxp=(1.0, PY)):
        self.frame = frame
        self.maxp = maxp
        self.dirty = []
        if sum_leaves is None:
            self.lv = [[[np.zeros(1), np.zeros(1, np.uint8)]] for _ in range(2)]
        else:
            min_leaves = sum_leaves if min_leaves is None else min_leaves
            self.lv = [[[v.copy(), t.copy()] for v, t in build_levels(*leaves, which)]
                       for which, leaves in enumerate((sum_leaves, min_leaves))]

    @property
    def L(self):
        return self.frame.log2_size

    def node(self, which, l, j):
        v, t = self.lv[which][l]
        return float(v[j]), int(t[j])

    def _store(self, which, l, j, val):
        v, t = self.lv[which][l]
        v[j], t[j] = val
        self.dirty.append((which, l, j))

    def root(self, which):
        return self.node(which, self.L, 0)

    # -- TreeQueue._write ----------------------------------------------------------------------
    def write(self, which, j, val):
        """_write(ix, value) on one tree (``val`` NONE deletes the leaf); returns the old leaf."""
        old = self.node(which, 0, j)
        self._store(which, 0, j, val if val[1] != ABSENT else NONE)
        red = reduce_min if which else reduce_sum
        for l in range(1, self.L + 1):
            j >>= 1
            self._store(which, l, j, red(self.node(which, l - 1, 2 * j), self.node(which, l - 1, 2 * j + 1)))
        return old

    # -- frame changes (prioritized.py:207-242), for the pin to the oracle ------------------------
    def append(self, val):
        f = self.frame
        if f.length == 0:
            self.lv = [[[np.zeros(1), np.zeros(1, np.uint8)]] for _ in range(2)]
        elif f.next_x == f.base + f.size:
            for tree in self.lv:
                top = [tree[-1][0].copy(), tree[-1][1].copy()]     # [self.root, [], root_value]
                for lev in tree:
                    lev[0] = np.concatenate([lev[0], np.zeros_like(lev[0])])
                    lev[1] = np.concatenate([lev[1], np.zeros_like(lev[1])])
                tree.append(top)
        x = f.append()
        for which in (0, 1):
            self.write(which, x - f.base, val)
        return x

    def popleft(self):
        f = self.frame
        for which in (0, 1):
            self.write(which, f.head - f.base, NONE)
        L = f.log2_size
        f.popleft()
        if f.length and f.log2_size < L:
            for tree in self.lv:
                tree.pop()
                for lev in tree:
                    half = len(lev[0]) // 2
                    lev[0], lev[1] = lev[0][half:].copy(), lev[1][half:].copy()

    # -- SumTreeQueue.prioritized_sample ---------------------------------------------------------
    def find(self, u):
        """_find from the root with np.random.uniform(0.0, root) = 0.0 + (root - 0.0) * u.
        Returns (leaf, [Step])."""
        root = self.root(0)
        pos = (float(np.float64(0.0) + np.float64(root[0]) * np.float64(u)), PY)
        j, steps = 0, []
        tags = [lev[1] for lev in self.lv[0]]
        for l in range(self.L, 0, -1):
            left = self.node(0, l - 1, 2 * j)
            kids = (int(tags[l - 2][4 * j]), int(tags[l - 2][4 * j + 2])) if l >= 2 else None
            lval = left if left[1] != ABSENT else ZERO
            cmp32 = max(pos[1], lval[1]) == F32
            tie = (np.float32(pos[0]) == np.float32(lval[0])) if cmp32 else (pos[0] == lval[0])
            if s_lt(pos, lval):
                steps.append(Step(l, pos[1], left[1], kids, bool(tie), False))
                j = 2 * j
            else:
                steps.append(Step(l, pos[1], left[1], kids, bool(tie), True))
                pos = s_sub(pos, lval)
                j = 2 * j + 1
        return j, steps

    def sibling_tags(self, j):
        """Tags of the siblings of leaf j's path, level 0 .. L - 1."""
        return [int(self.lv[0][c][1][(j >> c) ^ 1]) for c in range(self.L)]

    def draw(self, u):
        j, steps = self.find(u)
        sibs = self.sibling_tags(j)
        old = self.write(0, j, ZERO)
        assert old[1] != ABSENT, "the reference asserts here: a draw reached an absent leaf"
        return j, old, steps, sibs

    def sample(self, us, normalize, beta, slot_mod=0):
        """PrioritizedBuffer.sample with uniform_ratio = 0 and the weights of
        PriorityWeightError.weights_from_probabilities; ``trace`` holds what each draw met."""
        f = self.frame
        total, minv = self.root(0), self.root(1)
        xs, pri, trace = [], [], []
        for u in us:
            j, old, steps, sibs = self.draw(u)
            xs.append(f.base + j)
            pri.append(old)
            trace.append((j, steps, sibs))
        prob = np.array([s_add(ZERO, s_div(p, total))[0] for p in pri], dtype=np.float64)
        min_prob = s_div(minv, total)[0]
        with np.errstate(all="ignore"):
            if normalize == 0:
                w = np.power(np.float64(f.length) * prob, -np.float64(beta))
            else:
                den = np.min(prob) if normalize == 1 else np.float64(min_prob)
                w = np.power(prob / den, -np.float64(beta))
        xs = np.array(xs, dtype=np.int64)
        return dict(x=xs, pri=np.array([p[0] for p in pri], dtype=np.float64),
                    pri_tag=np.array([p[1] for p in pri], dtype=np.uint8), prob=prob,
                    weight=w.astype(np.float32), total=total[0], total_tag=total[1], min_prob=min_prob,
                    slot=(xs % slot_mod).astype(np.int32) if slot_mod else None, trace=trace)

    # -- the writes --------------------------------------------------------------------------------
    def set_last_priority(self, xs, vals, tags):
        """prioritized.py:107-116: sequential, so the last occurrence of a leaf wins; max_priority
        moves only for a strictly larger (typed) priority."""
        for x, v, t in zip(xs, vals, tags):
            p = (float(v), int(t))
            for which in (0, 1):
                self.write(which, int(x) - self.frame.base, p)
            if s_lt(self.maxp, p):
                self.maxp = p

    def write_leaves(self, xs, vals, tags, use_maxp):
        """The leaf writes of append (at max_priority when ``use_maxp``) and popleft (ABSENT)."""
        for x, v, t, m in zip(xs, vals, tags, use_maxp):
            p = self.maxp if m else (float(v), int(t))
            for which in (0, 1):
                self.write(which, int(x) - self.frame.base, p)

    def write_sum(self, xs, vals=None, tags=None):
        """uniform_sample's _write on the sum tree only (0.0 when no values); the old leaves."""
        old = []
        for i, x in enumerate(xs):
            p = ZERO if vals is None else (float(vals[i]), int(tags[i]))
            old.append(self.write(0, int(x) - self.frame.base, p))
        return (np.array([o[0] for o in old], dtype=np.float64),
                np.array([o[1] for o in old], dtype=np.uint8))

    def update_errors(self, xs, errs, cfg):
        v, t = priorities_of_errors(errs, cfg)
        self.set_last_priority(xs, v, t)


ErrCfg = collections.namedtuple("ErrCfg", "error_min error_max eps alpha")


def priorities_of_errors(errs, cfg):
    """priority_from_errors stays the oracle's."""
    v, t = oracle.priority_from_errors_f32(np.asarray(errs, dtype=np.float32), cfg.error_min,
                                           cfg.error_max, cfg.eps, cfg.alpha)
    return v, t.astype(np.uint8)


def clip_priorities(cfg):
    """(pri_at_min, pri_at_max): what the clipped branches give, Python floats."""
    lo = None if cfg.error_min is None else float(cfg.error_min + cfg.eps) ** cfg.alpha
    hi = None if cfg.error_max is None else float(cfg.error_max + cfg.eps) ** cfg.alpha
    return lo, hi


# ---------------------------------------------------------------------------------------------
# frames and the ring layout
# ---------------------------------------------------------------------------------------------
FrameSpec = collections.namedtuple("FrameSpec", "L length head_off rebased start shift smax")


def fspec(L, length, head_off=0, rebased=False, start=0, shift=0, smax=None):
    return FrameSpec(L, length, head_off, rebased, start, shift, L + 1 if smax is None else smax)


_grown = {}     # L -> untouched frame (base 0) at the append that made it 2^L wide


def _grow(L):
    if L not in _grown:
        have = [k for k in _grown if k < L]
        f = copy.deepcopy(_grown[max(have)]) if have else TreeFrame()
        while f.length == 0 or f.log2_size < L:
            f.append()
            if f.log2_size not in _grown:
                _grown[f.log2_size] = copy.deepcopy(f)
    return copy.deepcopy(_grown[L])


@functools.lru_cache(maxsize=None)
def _build_frame(spec):
    L = spec.L
    if spec.start == 0 and not spec.rebased:
        f = _grow(L)
    else:
        f = TreeFrame()
        for _ in range(spec.start):         # a buffer that ran empty: the next frame starts here
            f.append()
            f.popleft()
        while f.length == 0 or f.log2_size < L + int(spec.rebased):
            f.append()
        while f.log2_size > L:              # pop until the frame halves: base moves to the middle
            f.popleft()
    while f.next_x < f.base + spec.head_off + spec.length:
        f.append()
    while f.head < f.base + spec.head_off:
        f.popleft()
    assert (f.log2_size, f.length, f.head - f.base) == (L, spec.length, spec.head_off), spec
    if spec.shift:
        f.base += spec.shift
        f.head += spec.shift
        f.next_x += spec.shift
        for l in range(1, MAX_LEVELS):
            f.origin[l] += spec.shift
    return f


def build_frame(spec):
    return copy.deepcopy(_build_frame(spec))


class Layout:
    """Where PrioritizedBuffer.__init__ puts the per-level rings, and the slot of a frame node."""

    def __init__(self, log2_smax):
        self.log2_smax = log2_smax
        self.level_off = [0] * MAX_LEVELS
        off = 0
        for l in range(MAX_LEVELS):
            self.level_off[l] = off
            off += max((1 << log2_smax) >> l, 1) if l <= log2_smax else 0
        self.n_nodes = off

    def ring(self, l):
        return max((1 << self.log2_smax) >> l, 1)

    def index(self, frame, l, j):
        """Flat index of node j (frame order; an int or an array) of level l."""
        q = ((frame.base - frame.origin[l]) >> l) + j
        return self.level_off[l] + (q & (self.ring(l) - 1))

    def flatten(self, trees):
        """The four node arrays as the device holds them; slots outside the frame are sentinels."""
        out = []
        for which in (0, 1):
            v = np.full(self.n_nodes, SENT_V, dtype=np.float64)
            t = np.full(self.n_nodes, SENT_T, dtype=np.uint8)
            for l, (lv, lt) in enumerate(trees.lv[which]):
                idx = self.index(trees.frame, l, np.arange(len(lv), dtype=np.int64))
                v[idx], t[idx] = lv, lt
            out += [v, t]
        return out


# ---------------------------------------------------------------------------------------------
# leaves
# ---------------------------------------------------------------------------------------------
def make_leaves(spec, kind, seed=0):
    """(values, tags) of the 2^L leaves; present on [head_off, head_off + length)."""
    rs = np.random.RandomState(seed + 1000 * spec.L)
    n = 1 << spec.L
    lo, hi = spec.head_off, spec.head_off + spec.length
    v = rs.rand(n) * 2.0 + 0.01
    if kind == "mixed":
        t = rs.choice([PY, F32, F64], size=n, p=[0.3, 0.5, 0.2]).astype(np.uint8)
    elif kind == "f32":
        t = np.full(n, F32, np.uint8)
    elif kind == "py":
        t = np.full(n, PY, np.uint8)
    elif kind == "ones32":
        v, t = np.ones(n), np.full(n, F32, np.uint8)
    elif kind == "ones_py":
        v, t = np.ones(n), np.full(n, PY, np.uint8)
    elif kind[0] == "planted":          # ~99 % of the mass in one leaf
        t = np.full(n, F32, np.uint8)
        v[kind[1]] = 99.0 * v[lo:hi].sum()
    elif kind[0] == "ranges":           # ("ranges", [(lo, hi, tag)], heavy leaf): PY elsewhere
        t = np.full(n, PY, np.uint8)
        for a, b, tag in kind[1]:
            t[a:b] = tag
        v[kind[2]] = 1000.0
    else:
        raise ValueError(kind)
    v = np.where(t == F32, v.astype(np.float32).astype(np.float64), v)
    t[:lo] = ABSENT
    t[hi:] = ABSENT
    return np.where(t == ABSENT, 0.0, v), t


# ---------------------------------------------------------------------------------------------
# host restatements of the gates
# ---------------------------------------------------------------------------------------------
def sampler_route(L):
    r = min(L, K_BOT_LEVELS)
    return "lean2" if L - r + 1 <= K_MAX_TOP_LOG2 else "one_wave"


def repair_route(L, n, env_levels=False):
    if not env_levels and n <= K_FAST_THREADS and 1 <= L <= K_FAST_LEVELS:
        return "hashed64" if n <= 64 else "hashed128"
    return "levels"


def fused_admits(L, Be, n):
    r = min(L, K_BOT_LEVELS)
    return Be >= 1 and Be + n <= 64 and 1 <= L <= K_FAST_LEVELS and L - r + 1 <= K_MAX_TOP_LOG2


def path_hash(key, slots):
    return (((int(key) & 0xFFFFFFFF) * 2654435761 & 0xFFFFFFFF) >> 20) & (slots - 1)


def step_kind(pt, lt):
    """Which arithmetic one level of _find is, by the NEP-50 types of position and left child."""
    if pt == F64 or lt == F64:
        return "f64"
    if pt == PY and lt == ABSENT:
        return "absent_left"
    if pt == PY and lt == PY:
        return "py_py"
    return "f32"


def pair_steps(L, steps):
    """How many pairs of levels take find_down's all-np.float32 step: the position np.float32 and
    none of the three left children it looks at np.float64.  The top heap pairs the levels from
    the root, the bottom heap from level r."""
    r = min(L, K_BOT_LEVELS)
    n = 0
    for first, count in ((0, L - r), (L - r, r)):
        for d in range(0, count - 1, 2):
            s = steps[first + d]
            if s.pt == F32 and s.lt != F64 and F64 not in s.lt_kids:
                n += 1
    return n


def chain_shape(L, sibs):
    """(l2, l3) of a draw's repair chain -- the first sibling that is np.float32 or wider, the
    first that is np.float64 -- and which of the three runs meet an absent / a Python-float
    sibling."""
    l2 = next((c for c, t in enumerate(sibs) if t >= F32), L)
    l3 = next((c for c, t in enumerate(sibs) if t == F64), L)
    run = lambda c: 0 if c < l2 else (1 if c < l3 else 2)
    absent = {run(c) for c, t in enumerate(sibs) if t == ABSENT}
    py = {run(c) for c, t in enumerate(sibs) if t == PY}
    return l2, l3, absent, py


def shape_name(L, l2, l3):
    if l2 == l3 == L:
        return "none_wide"
    if l2 == l3 == 0:
        return "f64_at_leaf"
    if 0 < l2 < l3 < L:
        return "three_runs"
    if l2 < l3 == L:
        return "f32_to_root"
    return "other"


# ---------------------------------------------------------------------------------------------
# sampler cases
# ---------------------------------------------------------------------------------------------
SampleCase = collections.namedtuple("SampleCase", "name frame leaves us normalize beta slot_mod")
U_LAST = 1.0 - 2.0 ** -53


def _us(seed, B, first=()):
    u = np.random.RandomState(seed).random_sample(B)
    u[:len(first)] = first
    return u


def _planted_us():
    """Draw 0 removes the leaf holding 99 % of the mass; u1 is chosen so that draw 1's level-r node
    differs between the root before draw 0 and the root after it."""
    spec = PLANTED_FRAME
    tr = Trees(build_frame(spec), make_leaves(spec, PLANTED_LEAVES))
    u0 = 0.5
    for u1 in np.random.RandomState(7).random_sample(400):
        before = tr.find(u1)[0] >> K_BOT_LEVELS
        t2 = copy.deepcopy(tr)
        t2.draw(u0)
        after = t2.find(u1)[0] >> K_BOT_LEVELS
        if before != after:
            return np.array([u0, u1, 0.3, 0.9])
    raise AssertionError("no planted miss found")


def _tie_us(spec, kind, ks):
    """u_i with root_i * u_i == k_i exactly, on integer-valued leaves."""
    tr = Trees(build_frame(spec), make_leaves(spec, kind))
    us = []
    for k in ks:
        root = tr.root(0)[0]
        u = k / root
        assert np.float64(root) * np.float64(u) == k, (k, root)
        us.append(u)
        tr.draw(u)
    return np.array(us)


PLANTED_FRAME = fspec(12, 3000, 500)
PLANTED_LEAVES = ("planted", 2222)
TIE_FRAME = fspec(10, 1024)
BIG21, BIG22, BIG23 = (fspec(21, (1 << 20) + 5000, smax=21), fspec(22, (1 << 21) + 777, smax=22),
                       fspec(23, (1 << 22) + 31, smax=23))
F10 = fspec(10, 900, 50, rebased=True, start=3)

SAMPLE_CASES = [
    SampleCase("L0", fspec(0, 1), "f32", _us(1, 1), 1, 0.4, 0),
    SampleCase("L0_rebased", fspec(0, 1, rebased=True, start=3), "mixed", _us(2, 1), 0, 0.6, 7),
    SampleCase("L1_all", fspec(1, 2), "mixed", _us(3, 2), 2, 0.4, 0),
    SampleCase("L2_all", fspec(2, 3, 1), "mixed", _us(4, 3, [0.0]), 1, 1.0, 0),
    SampleCase("L8_full_B64", fspec(8, 256), "f32", _us(5, 64), 1, 0.4, 0),
    SampleCase("L8_part_B63", fspec(8, 200, 17, rebased=True, start=5), "mixed", _us(6, 63, [0.0]), 2, 0.6, 0),
    SampleCase("L9_B65", fspec(9, 400, 100), "mixed", _us(7, 65), 1, 0.5, 0),
    SampleCase("L10_B129", F10, "mixed", _us(8, 129), 1, 0.4, 0),
    SampleCase("L10_B129_shifted", F10._replace(shift=SHIFT), "mixed", _us(8, 129), 1, 0.4, 1000003),
    SampleCase("L10_all_f32_B64", fspec(10, 1000, 10), "f32", _us(9, 64), 0, 0.7, 0),
    SampleCase("L13_f32_B64", fspec(13, 6000, 1000), "f32", _us(10, 64), 1, 0.4, 0),
    SampleCase("L13_mixed_B65", fspec(13, 6000, 1000, rebased=True), "mixed", _us(11, 65), 2, 0.4, 0),
    SampleCase("L13_py_B2", fspec(13, 8192), "py", _us(12, 2), 1, 0.4, 0),
    SampleCase("L13_B1", fspec(13, 5000, 100), "mixed", _us(13, 1), 1, 0.0, 0),
    SampleCase("L13_B3", fspec(13, 5000, 100), "f32", _us(14, 3), 1, 0.4, 0),
    SampleCase("planted_miss", PLANTED_FRAME, PLANTED_LEAVES, _planted_us(), 1, 0.4, 0),
    # the repair chain's shapes: the heavy leaf takes the draw (u = 0.5)
    SampleCase("chain_three_runs_absent_mid", fspec(7, 100, 8),
               ("ranges", ((10, 12, F32), (16, 32, F64)), 8), np.array([0.5]), 1, 0.4, 0),
    SampleCase("chain_three_runs_absent_top", fspec(6, 48),
               ("ranges", ((34, 36, F32), (36, 40, F64)), 32), np.array([0.5]), 1, 0.4, 0),
    SampleCase("chain_none_wide_absent", fspec(6, 40, 3), "py", _us(15, 5, [0.0]), 1, 0.4, 0),
    SampleCase("chain_f32_to_root", fspec(6, 64), ("ranges", ((2, 4, F32),), 0), np.array([0.5]), 1, 0.4, 0),
    SampleCase("chain_f64_at_leaf", fspec(6, 64), ("ranges", ((1, 2, F64),), 0), np.array([0.5]), 1, 0.4, 0),
    # ties: integer np.float32 leaves, power-of-two total, u = k / total
    SampleCase("ties_top_and_bottom", TIE_FRAME, "ones32", _tie_us(TIE_FRAME, "ones32", [512, 1, 255]), 1, 0.4, 0),
    SampleCase("u_last_and_zero", TIE_FRAME, "ones_py", np.array([U_LAST, 0.0, U_LAST]), 1, 0.4, 0),
    SampleCase("L21_f32_B65", BIG21, "f32", _us(16, 65), 1, 0.4, 0),
    SampleCase("L22_mixed_B65", BIG22, "mixed", _us(17, 65, [0.0]), 1, 0.4, 0),
    SampleCase("L22_f32_B64", BIG22, "f32", _us(18, 64), 2, 0.6, 1000003),
]
SMALL_SAMPLE_CASES = [c for c in SAMPLE_CASES if c.frame.L <= 13]


@functools.lru_cache(maxsize=None)
def initial_leaves(spec, kind):
    return make_leaves(spec, kind)


@functools.lru_cache(maxsize=None)
def _initial_trees(spec, kind):
    return Trees(build_frame(spec), initial_leaves(spec, kind))


def initial_trees(spec, kind):
    """A fresh model of (frame, leaves); the 2^21 .. 2^23-leaf builds happen once."""
    return copy.deepcopy(_initial_trees(spec, kind))


# ---------------------------------------------------------------------------------------------
# repair cases
# ---------------------------------------------------------------------------------------------
RepairCase = collections.namedtuple(
    "RepairCase", "name entry frame leaves B n pick wpick dedupe cfg seed")
CFG = ErrCfg(0, 1, 0.01, 0.6)
CFG_OPEN = ErrCfg(None, None, 0.01, 0.6)
CFG_MIN = ErrCfg(0, None, 0.01, 0.6)
ENTRIES = ("write", "write_sum", "set_priorities", "update_errors", "update_errors_write")
W11 = fspec(11, 1800, 100, rebased=True, start=3)
H13 = fspec(13, 8192)
P16 = fspec(16, 65536)


def rcase(name, entry, frame, B, n=0, leaves="mixed", pick="random", wpick="edges", dedupe=1,
          cfg=CFG, seed=0):
    return RepairCase(name, entry, frame, leaves, B, n, pick, wpick, dedupe, cfg, seed)


REPAIR_CASES = []
for _e in ENTRIES:
    for _w in (1, 63, 64, 65, 1023, 1024):
        _n = _w // 3 if _e == "update_errors_write" else 0
        REPAIR_CASES.append(rcase("%s_w%d" % (_e, _w), _e, W11, _w - _n, _n, seed=_w))
for _w in (1, 63, 64, 65, 127, 128, 129, 1023, 1024):
    _n = _w // 4
    REPAIR_CASES.append(rcase("uew_sum%d" % _w, "update_errors_write", W11._replace(shift=SHIFT),
                              _w - _n, _n, seed=100 + _w))
REPAIR_CASES += [
    rcase("uew_L0", "update_errors_write", fspec(0, 1), 1, 0),
    rcase("uew_L0_write_wins", "update_errors_write", fspec(0, 1, rebased=True), 1, 1, wpick="same"),
    rcase("uew_L1", "update_errors_write", fspec(1, 2), 1, 1),
    rcase("uew_L9", "update_errors_write", fspec(9, 300, 100), 40, 24),
    rcase("uew_L9_open", "update_errors_write", fspec(9, 300, 100), 60, 40, cfg=CFG_OPEN),
    rcase("uew_L22_64", "update_errors_write", BIG22, 32, 32, leaves="f32"),
    rcase("uew_L22_128", "update_errors_write", BIG22, 100, 28, leaves="f32", seed=1),
    rcase("uew_L22_129", "update_errors_write", BIG22, 100, 29, leaves="f32", seed=2),
    rcase("uew_L23_64", "update_errors_write", BIG23, 32, 32, leaves="f32"),
    rcase("uew_L23_128", "update_errors_write", BIG23, 100, 28, leaves="f32", seed=1),
    # the hash table: three leaves whose level-0 keys share a home slot; the merge patterns
    rcase("hash3_64", "update_errors_write", H13, 40, 8, pick="hash3_128", seed=3),
    rcase("hash3_128", "update_errors_write", H13, 100, 20, pick="hash3_256", seed=4),
    rcase("adjacent_64", "update_errors_write", fspec(10, 900, 50), 48, 16, pick="adjacent", wpick="adjacent"),
    rcase("adjacent_128", "update_errors_write", fspec(10, 900, 50), 96, 32, pick="adjacent", wpick="adjacent"),
    rcase("subtree7_64", "update_errors_write", H13, 64, 0, pick="subtree7"),
    rcase("subtree7_128", "update_errors_write", H13, 128, 0, pick="subtree7"),
    rcase("per9_64", "update_errors_write", P16, 64, 0, pick="per9", leaves="f32"),
    rcase("per9_128", "update_errors_write", P16, 100, 28, pick="per9", wpick="per9", leaves="f32"),
    rcase("two_halves", "update_errors_write", H13, 2, 0, pick="halves"),
    # duplicates
    rcase("dup_dedupe", "update_errors_write", fspec(9, 300, 100), 30, 5, pick="dup"),
    rcase("dup_same_value_no_dedupe", "update_errors_write", fspec(9, 300, 100), 30, 5, pick="dup_same", dedupe=0),
    rcase("dup_dedupe_plain", "update_errors", fspec(9, 300, 100), 30, pick="dup"),
    rcase("dup_set_priorities", "set_priorities", fspec(9, 300, 100), 30, pick="dup"),
    rcase("write_wins", "update_errors_write", fspec(9, 300, 100), 20, 10, wpick="same"),
    rcase("maxp_raised", "update_errors_write", fspec(9, 300, 100), 20, 10, wpick="maxp", cfg=CFG_OPEN),
    # errors
    rcase("errors_clip", "update_errors", fspec(9, 300, 100), 64, pick="random", seed=9),
    rcase("errors_open", "update_errors", fspec(9, 300, 100), 64, cfg=CFG_OPEN, seed=9),
    rcase("errors_min_only", "update_errors_write", fspec(9, 300, 100), 64, 3, cfg=CFG_MIN, seed=9),
]
del _e, _w, _n
BIG_REPAIR = [c for c in REPAIR_CASES if c.frame.L >= 21]


def _pick(case, tr, rs, pattern, count, lay):
    f = tr.frame
    lo, hi = f.head - f.base, f.head - f.base + f.length
    if pattern == "random":
        return rs.choice(np.arange(lo, hi), size=count, replace=False)
    if pattern == "adjacent":
        a = lo + int(rs.randint(0, hi - lo - 2 * count))
        return np.arange(a, a + count)
    if pattern == "subtree7":
        a = 128 * int(rs.randint(lo // 128 + 1, hi // 128 - 1))
        return a + rs.permutation(128)[:count]
    if pattern == "per9":
        return 512 * rs.permutation((hi - lo) // 512)[:count] + rs.randint(0, 512, size=count)
    if pattern == "halves":
        return np.array([lo + 1, hi - 2])
    if pattern.startswith("hash3_"):
        slots = int(pattern[6:])
        home = collections.defaultdict(list)
        for j in range(lo, hi):
            home[path_hash(lay.index(f, 0, j), slots)].append(j)
        three = next(js for js in home.values() if len(js) >= 3)[:3]
        rest = rs.choice(np.setdiff1d(np.arange(lo, hi), three), size=count - 3, replace=False)
        return np.concatenate([three, rest])
    if pattern in ("dup", "dup_same"):
        js = rs.choice(np.arange(lo, hi), size=count, replace=False)
        js[count - 1] = js[0]
        js[count // 2] = js[1]
        js[count // 2 + 1] = js[1]
        return js
    raise ValueError(pattern)


def build_repair_case(case):
    """(model of the initial trees, layout, arguments of the launch as NumPy arrays)."""
    tr = initial_trees(case.frame, case.leaves)
    lay = Layout(case.frame.smax)
    f = tr.frame
    rs = np.random.RandomState(case.seed + 17)
    lo, hi = f.head - f.base, f.head - f.base + f.length
    joint = case.n and case.wpick == case.pick      # one pattern over errors and writes together
    js = _pick(case, tr, rs, case.pick, case.B + (case.n if joint else 0), lay)
    js, joint_w = js[:case.B], js[case.B:]
    a = dict(x=(f.base + js).astype(np.int64))
    err = (rs.rand(case.B) * 1.5).astype(np.float32)
    err[:8] = np.array([-0.5, 0.0, 1.0, 1.5, np.nan, 0.99999994, 1e-8, 1.0000001], np.float32)[:case.B]
    if case.cfg.error_min is None:
        err = np.where(np.isnan(err) | (err < 0), np.float32(0.25), err)
    elif case.cfg.error_max is None:
        err = np.where(np.isnan(err), np.float32(0.25), err)
    if case.pick == "dup_same":
        for j in np.unique(js):
            err[js == j] = err[js == j][0]
    a["err"] = err
    a["val"] = rs.rand(case.B) * 3.0 + 0.01
    a["tag"] = rs.choice([PY, F32, F64], size=case.B).astype(np.uint8)
    a["val"] = np.where(a["tag"] == F32, a["val"].astype(np.float32).astype(np.float64), a["val"])
    if case.entry == "write":           # appends at max_priority, pops, plain values
        a["use_maxp"] = (rs.rand(case.B) < 0.3).astype(np.uint8)
        a["tag"][rs.rand(case.B) < 0.2] = ABSENT
        a["val"] = np.where(a["tag"] == ABSENT, 0.0, a["val"])
    n = case.n
    if n:
        if case.wpick == "edges":       # pops at the head, appends past the end, overwrites
            cand = np.concatenate([np.arange(lo, lo + n), np.arange(hi, min(hi + n, f.size)),
                                   rs.choice(np.arange(lo + n, hi), size=min(n, hi - lo - n), replace=False)])
            wj = rs.permutation(np.setdiff1d(cand, js) if case.frame.L > 1 else cand)[:n]
            assert len(wj) == n, case.name
        elif case.wpick in ("same", "maxp"):
            wj = js[:n].copy()
        else:
            assert joint, case.name
            wj = joint_w
        a["wx"] = (f.base + wj).astype(np.int64)
        a["wtag"] = rs.choice([ABSENT, PY, F32, F64], size=n).astype(np.uint8)
        a["wval"] = np.where(a["wtag"] == ABSENT, 0.0, rs.rand(n) + 0.5)
        a["wval"] = np.where(a["wtag"] == F32, a["wval"].astype(np.float32).astype(np.float64), a["wval"])
        a["wmaxp"] = (rs.rand(n) < 0.3).astype(np.uint8)
        if case.wpick == "maxp":
            a["wmaxp"][:] = 1
            a["err"][0] = np.float32(40.0)      # raises max_priority above its initial 1.0
    return tr, lay, a


def apply_repair(case, tr, a):
    """The launch on the model.  Returns what the entry hands back (write_sum's old leaves)."""
    if case.entry == "write":
        return tr.write_leaves(a["x"], a["val"], a["tag"], a["use_maxp"])
    if case.entry == "write_sum":
        return tr.write_sum(a["x"], a["val"], np.where(a["tag"] == ABSENT, PY, a["tag"]))
    if case.entry == "set_priorities":
        return tr.set_last_priority(a["x"], a["val"], a["tag"])
    tr.update_errors(a["x"], a["err"], case.cfg)
    if case.n:
        tr.write_leaves(a["wx"], a["wval"], a["wtag"], a["wmaxp"])


FUSED_CASES = [c for c in REPAIR_CASES if c.entry == "update_errors_write"
               and fused_admits(c.frame.L, c.B, c.n)]
FAST_CASES = [c for c in REPAIR_CASES if c.entry == "update_errors_write"
              and repair_route(c.frame.L, c.B + c.n) != "levels"]


def fused_us(case):
    """The draws that follow the repair in the fused launch."""
    return _us(case.seed + 31, min(33, case.frame.length // 2 + 1), [0.0])


# =============================================================================================
# tests
# =============================================================================================
def _dump_oracle(o, which, L):
    return [o.dump_level(which, 1 << l) for l in range(L + 1)]


@pytest.mark.parametrize("cap", [1, 2, 5, 257, 3000])
def test_restatement_is_the_oracle(cap):
    """Seeded runs of appends, pops, samples and priority sets with mixed tags: every node of
    every level of both trees, the indices and removed priorities, the probabilities and the
    root statistics, all with ==."""
    rs = np.random.RandomState(cap)
    o = oracle.OraclePrioritizedBuffer(cap)
    tr = Trees(TreeFrame())

    def priority():
        k = rs.randint(5)
        if k == 0:
            return None
        v = rs.rand() * 2 + 0.01
        return [float(v), np.float32(v), np.float64(v), float(int(v * 4) + 1)][k - 1]

    def compare(full):
        f = tr.frame
        st = o.stats()
        assert st["length"] == f.length
        if f.length == 0:
            return
        assert st["bounds"] == f.bounds
        assert st["sum"] == tr.root(0) and st["min"] == tr.root(1) and st["max_priority"] == tr.maxp
        if not full:
            return
        for which in (0, 1):
            vect = build_levels(*tr.lv[which][0], which)
            for l, (ov, ot) in enumerate(_dump_oracle(o, which, f.log2_size)):
                mv, mt = tr.lv[which][l]
                mv = np.where(mt == ABSENT, 0.0, mv)
                assert np.array_equal(ov.view(np.int64), mv.view(np.int64)), (which, l)
                assert np.array_equal(ot, mt), (which, l)
                assert np.array_equal(vect[l][0].view(np.int64), mv.view(np.int64)), (which, l)
                assert np.array_equal(vect[l][1], mt), (which, l)

    steps = 60 if cap <= 5 else (700 if cap == 257 else 3600)
    for step in range(steps):
        k = rs.rand()
        n = len(o)
        if k < (0.9 if n < cap and step < steps // 2 else 0.45):
            p = priority()
            if n == cap:
                tr.popleft()
            o.append(step, p)
            tr.append(tr.maxp if p is None else (float(p), oracle.type_tag(p)))
        elif k < 0.6 and n > 0:
            o.popleft()
            tr.popleft()
        elif n > 0:
            B = int(rs.randint(1, min(n, 40) + 1))
            us = rs.random_sample(B)
            if step % 7 == 0:
                us[0] = 0.0
            want = o.sample(us)
            got = tr.sample(us, 1, 0.4)
            assert np.array_equal(want["indices"], got["x"] - tr.frame.head)
            assert np.array_equal(want["priorities"], got["pri"])
            assert np.array_equal(want["priority_tags"], got["pri_tag"])
            assert np.array_equal(want["probabilities"], got["prob"])
            assert (want["total"], want["total_tag"], want["min_prob"]) == (
                got["total"], got["total_tag"], got["min_prob"])
            compare(step % 5 == 0)
            ps = [priority() or 0.75 for _ in range(B)]
            vals, tags = [float(p) for p in ps], [oracle.type_tag(p) for p in ps]
            o.set_last_priority(vals, tags)
            tr.set_last_priority(got["x"], vals, tags)
        compare(step % (3 if cap <= 5 else 50) == 0 or step == steps - 1)


def test_write_sum_returns_the_old_leaves_and_leaves_the_min_tree():
    spec = fspec(6, 40, 3)
    tr = initial_trees(spec, "mixed")
    before = copy.deepcopy(tr.lv[1])
    xs = tr.frame.base + np.array([5, 9, 33])
    old_v, old_t = tr.write_sum(xs)
    lv, lt = initial_leaves(spec, "mixed")
    assert np.array_equal(old_v, lv[[5, 9, 33]]) and np.array_equal(old_t, lt[[5, 9, 33]])
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(before, tr.lv[1]))
    tr.write_sum(xs, old_v, old_t)
    fresh = initial_trees(spec, "mixed")
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
               for a, b in zip(fresh.lv[0], tr.lv[0]))
    assert {w for w, _, _ in tr.dirty} == {0}


@pytest.mark.parametrize("spec", [fspec(0, 1, rebased=True, start=3), fspec(2, 3, 1), F10,
                                  fspec(8, 200, 17, rebased=True, start=5), W11, BIG21])
def test_translating_a_frame_keeps_every_ring_index(spec):
    f, g = build_frame(spec), build_frame(spec._replace(shift=SHIFT))
    assert (g.base - f.base, g.head - f.head, g.length, g.log2_size) == (SHIFT, SHIFT, f.length, f.log2_size)
    lay = Layout(spec.smax)
    assert all(SHIFT % lay.ring(l) == 0 for l in range(spec.smax + 1))
    for l in range(spec.L + 1):
        j = np.arange(1 << (spec.L - l), dtype=np.int64)
        assert np.array_equal(lay.index(f, l, j), lay.index(g, l, j))
        assert len(np.unique(lay.index(f, l, j))) == len(j)         # the frame fits its ring
    assert g.base > 1 << 31


def test_frames_reach_what_they_claim():
    specs = {c.frame for c in SAMPLE_CASES} | {c.frame for c in REPAIR_CASES}
    built = {s: build_frame(s) for s in specs}
    # base != 0 with head > base (absent leaves on the left) and length < size (absent on the right)
    assert any(f.base != 0 and f.head > f.base and f.length < f.size and s.shift == 0
               for s, f in built.items())
    assert any(f.origin[1] not in (0, SHIFT) for f in built.values())   # origins that are not 0
    shifted = [c for c in SAMPLE_CASES if c.frame.shift]
    assert shifted and all(c.slot_mod & (c.slot_mod - 1) and c.slot_mod > 1 for c in shifted)
    assert any(c.frame._replace(shift=0) == d.frame and np.array_equal(c.us, d.us)
               for c in shifted for d in SAMPLE_CASES if not d.frame.shift)
    assert any(c.frame.shift for c in REPAIR_CASES)


@functools.lru_cache(maxsize=None)
def _small_traces():
    out = {}
    for c in SMALL_SAMPLE_CASES:
        tr = initial_trees(c.frame, c.leaves)
        out[c.name] = tr.sample(c.us, c.normalize, c.beta, c.slot_mod)
    return out


def test_sampler_cases_reach_every_route():
    Ls = {c.frame.L for c in SAMPLE_CASES}
    assert {0, 1, 2, 8, 9, 10, 13, 21, 22} <= Ls
    assert all(sampler_route(L) == "lean2" for L in (0, 1, 2, 8, 9, 10, 13, 21))
    assert sampler_route(22) == "one_wave"
    assert {1, 2, 3, 63, 64, 65, 129} <= {len(c.us) for c in SAMPLE_CASES}
    assert sum(len(c.us) == c.frame.length for c in SAMPLE_CASES if c.frame.L <= 2) >= 3
    assert all(len(c.us) <= 65 for c in SAMPLE_CASES if c.frame.L >= 21)
    assert all(len(c.us) <= c.frame.length for c in SAMPLE_CASES)
    assert {0, 1, 2} == {c.normalize for c in SAMPLE_CASES}
    # the LDS the last lean2 frame asks for
    assert ((1 << 13) + 2 * (1 << 10)) * 9 == 92160


def test_sampler_cases_share_subtrees_and_plant_a_miss():
    seen = fresh = late_seen = 0
    for c in SMALL_SAMPLE_CASES:
        r = min(c.frame.L, K_BOT_LEVELS)
        nodes = [j >> r for j, _, _ in _small_traces()[c.name]["trace"]]
        for i in range(1, len(nodes)):
            hit = nodes[i] in nodes[:i]
            seen += hit
            fresh += not hit
            late_seen += hit and i >= 64
    assert seen > 50 and fresh >= 20 and late_seen > 0
    c = next(c for c in SAMPLE_CASES if c.name == "planted_miss")
    tr = initial_trees(c.frame, c.leaves)
    before = tr.find(c.us[1])[0] >> K_BOT_LEVELS
    j0, old, _, _ = tr.draw(c.us[0])
    assert j0 == c.leaves[1] and old[0] > 0.98 * _small_traces()[c.name]["total"]
    assert tr.find(c.us[1])[0] >> K_BOT_LEVELS != before


def test_sampler_cases_reach_every_chain_shape():
    shapes = collections.defaultdict(set)
    py_after_f32 = False
    for c in SMALL_SAMPLE_CASES:
        for j, steps, sibs in _small_traces()[c.name]["trace"]:
            l2, l3, absent, py = chain_shape(c.frame.L, sibs)
            shapes[shape_name(c.frame.L, l2, l3)] |= absent
            py_after_f32 |= 0 < l2 < l3 < c.frame.L and 2 in py
    assert {"none_wide", "f64_at_leaf", "three_runs", "f32_to_root"} <= set(shapes)
    assert 0 in shapes["none_wide"] and 1 in shapes["three_runs"] and 2 in shapes["three_runs"]
    assert 1 in shapes["f32_to_root"]
    assert py_after_f32


def test_sampler_cases_reach_every_descent_step_and_tie():
    kinds, pairs = collections.Counter(), 0
    tie_top = tie_bottom = False
    for c in SMALL_SAMPLE_CASES:
        L = c.frame.L
        for j, steps, sibs in _small_traces()[c.name]["trace"]:
            kinds.update(step_kind(s.pt, s.lt) for s in steps)
            pairs += pair_steps(L, steps)
            for s in steps:
                if s.tie and s.lt != ABSENT and c.name.startswith("ties"):
                    tie_top |= s.level - 1 >= K_BOT_LEVELS
                    tie_bottom |= s.level - 1 < K_BOT_LEVELS
    assert all(kinds[k] > 0 for k in ("f32", "py_py", "f64", "absent_left")), kinds
    assert pairs > 100
    assert tie_top and tie_bottom
    us = np.concatenate([c.us for c in SAMPLE_CASES])
    assert (us == 0.0).any() and (us == U_LAST).any() and U_LAST < 1.0
    assert any(c.us[0] == 0.0 and c.frame.L >= 21 for c in SAMPLE_CASES)


def test_repair_cases_reach_every_width_gate_and_pattern():
    for e in ENTRIES:
        assert {1, 63, 64, 65, 1023, 1024} <= {c.B + c.n for c in REPAIR_CASES if c.entry == e}
    uew = [c for c in REPAIR_CASES if c.entry == "update_errors_write"]
    assert {1, 63, 64, 65, 127, 128, 129, 1023, 1024} <= {c.B + c.n for c in uew}
    assert {0, 1, 9, 22, 23} <= {c.frame.L for c in uew}
    route = {(c.frame.L, c.B + c.n): repair_route(c.frame.L, c.B + c.n) for c in uew}
    assert route[(0, 1)] == "levels" and route[(1, 2)] == "hashed64"
    assert route[(22, 64)] == "hashed64" and route[(22, 128)] == "hashed128"
    assert route[(22, 129)] == "levels" and route[(23, 64)] == "levels" and route[(23, 128)] == "levels"
    assert route[(11, 64)] == "hashed64" and route[(11, 65)] == "hashed128"
    assert route[(11, 128)] == "hashed128" and route[(11, 129)] == "levels"
    assert {"hashed64", "hashed128"} <= {repair_route(c.frame.L, c.B + c.n) for c in FAST_CASES}
    assert all(repair_route(c.frame.L, c.B + c.n, env_levels=True) == "levels" for c in uew)
    assert len(FUSED_CASES) >= 10 and {1, 9} <= {c.frame.L for c in FUSED_CASES}
    assert 64 in {c.B + c.n for c in FUSED_CASES}
    assert all(len(np.unique(build_repair_case(c)[2]["x"])) == c.B
               for c in REPAIR_CASES if c.frame.L < 21 and not c.pick.startswith("dup"))


def test_hash_cases_have_probe_chains_and_merge_patterns():
    for name, slots in (("hash3_64", 128), ("hash3_128", 256)):
        c = next(c for c in REPAIR_CASES if c.name == name)
        assert repair_route(c.frame.L, c.B + c.n) == "hashed%d" % (slots // 2)
        tr, lay, a = build_repair_case(c)
        keys = lay.index(tr.frame, 0, a["x"][:3] - tr.frame.base)
        assert len(set(keys)) == 3 and len({path_hash(k, slots) for k in keys}) == 1
    by = {c.name: build_repair_case(c) for c in REPAIR_CASES if c.frame.L < 21}
    for name in ("adjacent_64", "adjacent_128"):
        x = np.sort(by[name][2]["x"])
        assert (np.diff(x) == 1).all()
    for name in ("subtree7_64", "subtree7_128"):
        assert len(set(by[name][2]["x"] >> 7)) == 1
    for name in ("per9_64", "per9_128"):
        a = by[name][2]
        x = np.concatenate([a["x"], a.get("wx", a["x"][:0])])
        assert len(set(x >> 9)) == len(x)
    x = by["two_halves"][2]["x"]
    assert (x[0] >> 12) != (x[1] >> 12)


def test_duplicate_error_and_write_cases_are_what_they_claim():
    by = {c.name: (c, *build_repair_case(c)) for c in REPAIR_CASES if c.frame.L < 21}
    c, tr, lay, a = by["dup_dedupe"]
    v, _ = priorities_of_errors(a["err"], c.cfg)
    dup = [x for x in set(a["x"]) if (a["x"] == x).sum() > 1]
    assert dup and c.dedupe and any(len(set(v[a["x"] == x])) > 1 for x in dup)
    apply_repair(c, tr, a)
    for x in dup:       # the last occurrence wins
        assert tr.node(0, 0, x - tr.frame.base)[0] == v[np.nonzero(a["x"] == x)[0][-1]]
    c, tr, lay, a = by["dup_same_value_no_dedupe"]
    v, _ = priorities_of_errors(a["err"], c.cfg)
    assert not c.dedupe and all(len(set(v[a["x"] == x])) == 1 for x in set(a["x"]))
    assert len(set(a["x"])) < len(a["x"])
    c, tr, lay, a = by["write_wins"]
    assert set(a["wx"]) <= set(a["x"])
    c, tr, lay, a = by["maxp_raised"]
    before = tr.maxp
    apply_repair(c, tr, a)
    assert s_lt(before, tr.maxp) and a["wmaxp"].all()
    assert all(tr.node(0, 0, x - tr.frame.base) == tr.maxp for x in a["wx"])
    c, tr, lay, a = by["errors_clip"]
    e = a["err"]
    assert (e < 0).any() and (e > 1).any() and np.isnan(e).any() and (e == 0).any() and (e == 1).any()
    assert {c.cfg for c in REPAIR_CASES} >= {CFG, CFG_OPEN, CFG_MIN}


def test_dirty_log_is_every_changed_node():
    """The device comparison patches the expected arrays at the logged nodes only."""
    for c in [c for c in REPAIR_CASES if c.frame.L <= 11][::4]:
        tr, lay, a = build_repair_case(c)
        flat0 = lay.flatten(tr)
        apply_repair(c, tr, a)
        flat1 = lay.flatten(tr)
        for which in (0, 1):
            idx = {lay.index(tr.frame, l, j) for w, l, j in tr.dirty if w == which}
            changed = np.nonzero((flat0[2 * which].view(np.int64) != flat1[2 * which].view(np.int64))
                                 | (flat0[2 * which + 1] != flat1[2 * which + 1]))[0]
            assert set(changed) <= idx


def test_fused_cases_draw_from_the_repaired_tree():
    for c in FUSED_CASES:
        assert c.frame.L < 21 and repair_route(c.frame.L, c.B + c.n) == "hashed64"
        tr, lay, a = build_repair_case(c)
        apply_repair(c, tr, a)
        got = tr.sample(fused_us(c), 1, 0.4)
        assert (got["pri_tag"] != ABSENT).all() and len(got["x"]) >= 1
    assert not fused_admits(0, 1, 0) and not fused_admits(22, 1, 0) and not fused_admits(9, 0, 3)
    assert not fused_admits(9, 33, 32) and fused_admits(21, 32, 32)
