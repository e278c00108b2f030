"""CPU statement of the rejection sampling's trial window (mm_trace.h
shade_step, predraw_trials) against the reference's plain loop
(shaders.metal:315-318).

The reference draws trials from a path's RNG stream until one is accepted,
once per diffuse bounce.  The kernel now runs this statement (the two-trial
bank of tests/test_bank_model.py is the one it ran before): a path carries a
window (sb, mask) on its stream -- sb the state at the first trial no bounce
has consumed, bit i of mask set when trial i from there was accepted, the
highest set bit a sentinel above the trials drawn so far (room for 31).  A
chunk of new paths pre-draws K trials per path, acceptance only; a diffuse
bounce that will read its new direction runs rounds (every diffuse lane with
room draws its next trial, whose start is a table jump of 3 d steps from sb)
while any such lane has no accepted bit, then takes trial i = ctz(mask): the
three numbers redrawn from the jump of 3 i steps, sb the state after them,
mask >>= i + 1.  A full window without an accepted bit skips its 31 trials
(sb jumps 93 steps) and empties.  A diffuse lane at its last bounce
(n + 1 >= bounce_limit + mh) requests nothing.

This model runs that statement lane-parallel in numpy uint32 / float32 with
the device's operations over 60 bounces -- paths of random lengths end and new
ones start on their lanes, so windows run out and re-fill many times -- with
random diffuse / mirror masks and random parking of paths through the tail
record's words (sb, (n - mh) | mh << 15, mask), and checks that every path's
k-th diffuse direction sample is the k-th accepted trial of its stream.
"""
from __future__ import annotations

import numpy as np
import pytest

A, C = np.uint32(747796405), np.uint32(291336453)
HASH = np.uint32(277803737)
ONE_PLUS = np.float32(1.0) + np.float32(2.0 ** -23)      # length(r) > 1 <=> len2 > 1 + 2^-23
ACC_EDGE = np.float32(1.0) + np.float32(2.0 ** -22)      # accepted <=> q2 < 1 + 2^-22 (the kernel's sign test)
WINDOW = 31
FULL = np.uint32(1 << WINDOW)


def jump_table():
    """mm_trace.h lcg_jump3: entry i = (A3, C3), A3 s + C3 = the state 3 i steps after s."""
    a, c, out = 1, 0, []
    for _ in range(WINDOW + 1):
        out.append((a, c))
        for _ in range(3):
            a = (int(A) * a) % 2**32
            c = (int(A) * c + int(C)) % 2**32
    return np.array(out, dtype=np.uint32)


JUMP = jump_table()


def rand_pm1(s):
    """mm_device.h rand_pm1 on uint32 arrays: the new state and RN(RN(float(r)) * 2^-31 - 1)."""
    with np.errstate(over="ignore"):
        s = s * A + C
        r = ((s >> ((s >> np.uint32(28)) + np.uint32(4))) ^ s) * HASH
    r = (r >> np.uint32(22)) ^ r
    # float(r) * 2^-31 is exact, so the fma's single rounding is the float32 subtraction's
    return s, (r.astype(np.float32) * np.float32(2.0 ** -31)) - np.float32(1.0)


def trial(s):
    s, x = rand_pm1(s)
    s, y = rand_pm1(s)
    s, z = rand_pm1(s)
    q2 = (x * x + y * y) + z * z  # dot3 in the IR's order, float32 throughout
    return s, np.stack([x, y, z], axis=-1), q2


def jump(s, i):
    with np.errstate(over="ignore"):
        return s * JUMP[i & WINDOW, 0] + JUMP[i & WINDOW, 1]


def drawn(mask):
    """31 - clz(mask): the sentinel's position = trials drawn so far."""
    return np.array([int(m).bit_length() - 1 for m in mask], dtype=np.int64)


def first_set(mask):
    """ctz(mask | 1 << 31)"""
    return np.array([((int(m) | (1 << WINDOW)) & -(int(m) | (1 << WINDOW))).bit_length() - 1 for m in mask],
                    dtype=np.int64)


def no_accepted(mask):
    return (mask & (mask - np.uint32(1))) == 0


def reference_samples(seed, count):
    """The first `count` accepted trials of the stream from `seed`, in order (the reference's loop)."""
    s = np.array([seed], dtype=np.uint32)
    got = []
    while len(got) < count:
        s, d, q2 = trial(s)
        if not q2[0] > ONE_PLUS:  # shaders.metal:316-318: rejected iff length(r) > 1
            got.append(d[0])
    return got


def predraw(sb, k):
    """mm_trace.h predraw_trials: k trials from sb, acceptance only."""
    s, mask = sb.copy(), np.zeros(len(sb), np.uint32)
    for r in range(k):
        s, _, q2 = trial(s)
        mask |= (q2 < ACC_EDGE).astype(np.uint32) << np.uint32(r)
    return mask | np.uint32(1 << k)


def sample_step(sb, mask, diffuse, wants):
    """shade_step's diffuse branch on the lanes `diffuse`; returns (sb, mask, directions, rounds)."""
    sb, mask = sb.copy(), mask.copy()
    need = wants & no_accepted(mask)
    rounds = 0
    while need.any():
        rounds += 1
        full = diffuse & (mask == FULL)
        sb = np.where(full, jump(sb, np.full(len(sb), WINDOW)), sb)
        mask = np.where(full, np.uint32(1), mask)
        d = drawn(mask)
        _, _, q2 = trial(jump(sb, d))
        acc = (q2 < ACC_EDGE).astype(np.uint32)
        room = (mask >> np.uint32(WINDOW)) ^ np.uint32(1)
        with np.errstate(over="ignore"):
            grown = mask + ((room + (room & acc)) << (d & WINDOW).astype(np.uint32))
        mask = np.where(diffuse, grown, mask)
        need = need & no_accepted(mask)
    i = first_set(mask)
    s_end, rd, _ = trial(jump(sb, i))
    sb = np.where(diffuse, s_end, sb)
    mask = np.where(diffuse, (mask >> i.astype(np.uint32)) >> np.uint32(1), mask)
    return sb, mask, rd, rounds


def pack(n, mh):
    return (n - mh) | (mh << 15)


def unpack(w):
    mh = (w >> 15) & 0x7FFF
    return (w & 0x7FFF) + mh, mh


def test_jump_table_entries_are_3i_single_steps():
    s0 = np.arange(1, 2000, dtype=np.uint32) * np.uint32(2654435761)
    s = s0.copy()
    for i in range(WINDOW + 1):
        assert np.array_equal(jump(s0, np.full(len(s0), i)), s), i
        for _ in range(3):
            s, _ = rand_pm1(s)
    assert tuple(JUMP[0]) == (1, 0)


def test_tail_record_words_round_trip():
    rng = np.random.default_rng(3)
    for _ in range(2000):
        mh = int(rng.integers(0, 32767))
        n = mh + int(rng.integers(0, 32767))
        w = pack(n, mh)
        assert w < 2**30 and unpack(w) == (n, mh)  # (the two bits above: free)
    # sb and mask travel as whole 32-bit words
    for v in (0, 1, 0x80000000, 0xFFFFFFFF, 0x80000001):
        assert int(np.uint32(v)) == v


def test_full_window_without_an_accepted_trial_is_skipped():
    """Forced with a crafted mask: the window claims 31 rejected trials, so the lane's sample is the first
    accepted trial at or after trial 31 of the stream from sb, and the window then starts behind it."""
    rng = np.random.default_rng(11)
    lanes = 64
    sb = rng.integers(0, 2**32, size=lanes, dtype=np.uint64).astype(np.uint32)
    mask = np.full(lanes, FULL, np.uint32)
    mask[1::2] = np.uint32(1)  # every other lane: an empty window on the same stream position
    on = np.ones(lanes, bool)
    sb2, mask2, rd, rounds = sample_step(sb, mask, on, on)
    assert rounds >= 1
    for j in range(lanes):
        s = np.array([sb[j]], np.uint32)
        if mask[j] == FULL:
            for _ in range(3 * WINDOW):
                s, _ = rand_pm1(s)
        start = s.copy()
        want = reference_samples(int(start[0]), 1)[0]
        assert np.array_equal(rd[j], want), j
        # the window's base is the state right after the taken trial's three draws
        k = 0
        while True:
            s, d, q2 = trial(s)
            k += 1
            if not q2[0] > ONE_PLUS:
                break
        assert sb2[j] == s[0] and mask2[j] != 0, j


@pytest.mark.parametrize("K", [0, 1, 7, 20, 31])
def test_trial_window_yields_the_reference_samples(K):
    rng = np.random.default_rng(7 + K)
    lanes, bounces = 64, 60

    class Path:
        def __init__(self):
            self.seed = int(rng.integers(0, 2**32))
            self.bl = int(rng.integers(20, 50))  # >= 19 samples: more trials than a window holds
            self.ref = reference_samples(self.seed, 80)
            self.used = 0

    paths = [Path() for _ in range(lanes)]
    sb = np.array([p.seed for p in paths], np.uint32)
    mask = predraw(sb, K)
    n = np.zeros(lanes, np.int64)
    mh = np.zeros(lanes, np.int64)
    rounds = taken = finished = refills = 0
    for b in range(bounces):
        bl = np.array([p.bl for p in paths], np.int64)
        diffuse = rng.random(lanes) < 0.9
        wants = diffuse & (n + 1 < bl + mh)
        before = mask.copy()
        sb, mask, rd, r = sample_step(sb, mask, diffuse, wants)
        rounds += r
        refills += int((wants & no_accepted(before)).sum())
        for j in np.nonzero(wants)[0]:
            p = paths[j]
            assert np.array_equal(rd[j], p.ref[p.used]), (K, b, j, p.used)
            p.used += 1
            taken += 1
        mh += ~diffuse
        n += 1
        # paths at their limit end; new ones start on their lanes (a new-path chunk's pre-pass)
        for j in np.nonzero(~(n < bl + mh))[0]:
            paths[j] = Path()
            finished += 1
            sb[j] = np.uint32(paths[j].seed)
            mask[j] = predraw(sb[j:j + 1], K)[0]
            n[j] = mh[j] = 0
        # park a random subset through the tail record's words and resume the paths in other lanes
        idx = np.nonzero(rng.random(lanes) < 0.3)[0]
        if len(idx) > 1:
            perm = rng.permutation(idx)
            words = [(int(sb[i]), pack(int(n[i]), int(mh[i])), int(mask[i]), paths[i]) for i in idx]
            for j, (w_sb, w_nm, w_mask, p) in zip(perm, words):
                sb[j], mask[j] = np.uint32(w_sb), np.uint32(w_mask)
                n[j], mh[j] = unpack(w_nm)
                paths[j] = p
    assert taken > lanes * bounces // 2 and finished > lanes // 2
    # windows ran out in the bounces and were re-filled there: a path reads >= 19 samples, 36 trials on
    # average where a window holds 31, and a lane in need makes every diffuse lane of the wave draw
    assert refills >= lanes // 4
    if K == 0:
        assert rounds > bounces
