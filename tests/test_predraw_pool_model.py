"""CPU statement of the pre-pass's pooled top-up rounds (mm_trace.h pool_trials) against sequential drawing.

A path's trial window is (sb, mask): bit i of mask tells that trial i of the stream from sb is accepted, the
highest set bit is a sentinel above the trials drawn (tests/test_predraw_model.py states the window and its use
in the bounces).  After the own rounds of a new-path chunk, the lanes whose windows hold fewer accepted trials
than the path reads ("needy", and only with room in the window) have their next trials drawn by the whole
wave: per round a stable split sends needy rank j's stream state at its first undrawn trial to lane j
(ds_permute), helper lane h fetches the state of rank h >> k (ds_bpermute), jumps h & (2^k - 1) trials on and
runs that trial, one ballot returns the accept bits and the needy lane takes its share's first
min(2^k, 31 - d) bits, 2^k the largest power of two (at most 32) with n 2^k <= active lanes.

This model runs those operations lane by lane in numpy uint32 / float32 with the device's arithmetic --
permutes as gathers / scatters over the 64 lanes, with inactive lanes holding poison and every read of one an
error -- and checks, for every lane, that the window it ends with is the window sequential drawing of the same
number of trials from sb gives, that every lane ends satisfied or full, and that no lane lost a trial."""
from __future__ import annotations

import numpy as np
import pytest

A, C = np.uint32(747796405), np.uint32(291336453)
HASH = np.uint32(277803737)
ACC_EDGE = np.float32(1.0) + np.float32(2.0 ** -22)  # accepted <=> q2 < 1 + 2^-22 (the kernel's sign test)
WINDOW = 31
LANES = 64
POISON = np.uint32(0xDEADBEEF)


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
    with np.errstate(over="ignore"):
        s = s * A + C
        r = ((s >> ((s >> np.uint32(28)) + np.uint32(4))) ^ s) * HASH
    r = (r >> np.uint32(22)) ^ r
    return s, (r.astype(np.float32) * np.float32(2.0 ** -31)) - np.float32(1.0)


def trial_accepted(s):
    s, x = rand_pm1(s)
    s, y = rand_pm1(s)
    s, z = rand_pm1(s)
    q2 = (x * x + y * y) + z * z
    return s, (q2 < ACC_EDGE).astype(np.uint32)


def jump(s, i):
    i = np.asarray(i, dtype=np.int64) & WINDOW
    with np.errstate(over="ignore"):
        return s * JUMP[i, 0] + JUMP[i, 1]


def sequential(sb, count):
    """The window after drawing count[l] trials of lane l's stream one after another (predraw_trials' loop)."""
    out = np.zeros(len(sb), np.uint32)
    for l in range(len(sb)):
        s, mask = sb[l:l + 1].copy(), 0
        for r in range(int(count[l])):
            s, acc = trial_accepted(s)
            mask |= int(acc[0]) << r
        out[l] = mask | (1 << int(count[l]))
    return out


def drawn(mask):
    return np.array([int(m).bit_length() - 1 for m in mask], dtype=np.int64)


def accepted(mask):
    return np.array([bin(int(m)).count("1") - 1 for m in mask], dtype=np.int64)


def pool_trials(sb, mask, need, n_act):
    """mm_trace.h pool_trials on one wave whose active lanes are 0 .. n_act - 1; returns (mask, rounds)."""
    mask = mask.copy()
    lane = np.arange(LANES)
    act = lane < n_act
    lg_act = n_act.bit_length() - 1
    rounds = 0
    while True:
        d = drawn(mask)
        needy = act & (accepted(mask) + 1 <= need) & (d < WINDOW)
        if not needy.any():
            return mask, rounds
        rounds += 1
        assert rounds <= WINDOW
        n = int(needy.sum())
        k = lg_act - (n.bit_length() - 1)
        if (n << k) > n_act:
            k -= 1
        k = min(k, 5)
        assert k >= 0 and (n << k) <= max(n_act, 32 * n)
        j = np.cumsum(needy) - needy                        # mbcnt of the needy ballot
        to = np.where(needy, j, n + (lane - j))
        sd = jump(sb, d)
        # ds_permute: active lanes scatter; the split is a permutation of the active prefix
        assert sorted(to[act]) == list(range(n_act))
        posted = np.full(LANES, POISON)
        posted[to[act]] = sd[act]
        # ds_bpermute: active lanes gather from lane >> k, an active lane
        src = lane >> k
        assert act[src[act]].all()
        t = np.where(act, posted[src], POISON)
        t = jump(t, lane & ((1 << k) - 1))
        _, acc = trial_accepted(t)
        ab = sum(int(acc[l]) << l for l in range(LANES) if act[l])  # the ballot: active lanes only
        room = WINDOW - d
        m = np.minimum(room, 1 << k)
        for l in np.nonzero(needy)[0]:
            bits = (ab >> ((int(j[l]) << k) & 63)) & ((1 << int(m[l])) - 1)
            at = int(d[l])
            mask[l] = (int(mask[l]) ^ (1 << at)) | (bits << at) | (1 << (at + int(m[l])))


def check(sb, mask0, need, n_act):
    got, rounds = pool_trials(sb, mask0, need, n_act)
    act = np.arange(LANES) < n_act
    d0, d1 = drawn(mask0), drawn(got)
    # inactive lanes untouched; trials only added, in order, none lost
    assert np.array_equal(got[~act], mask0[~act])
    assert (d1 >= d0).all() and (d1 <= WINDOW).all()
    low = (np.uint64(1) << d0.astype(np.uint64)) - np.uint64(1)
    assert np.array_equal(got.astype(np.uint64) & low, mask0.astype(np.uint64) & low)
    # the window sequential drawing of the same number of trials gives
    assert np.array_equal(got[act], sequential(sb[act], d1[act]))
    # every active lane ends with what it reads, or with a full window (the in-bounce rounds' business)
    assert ((accepted(got) >= need) | (d1 == WINDOW))[act].all()
    # a lane that was not needy drew nothing
    still = (accepted(mask0) >= need) | (d0 == WINDOW)
    assert np.array_equal(got[still], mask0[still])
    return rounds


@pytest.mark.parametrize("n_act", [64, 63, 43, 37, 8, 3, 1])
@pytest.mark.parametrize("need", [1, 7, 15, 31])
@pytest.mark.parametrize("K1", [0, 1, 5, 12, 24, 30, 31])
def test_pool_after_own_rounds(K1, need, n_act):
    """The kernel's use: K1 own rounds on every lane, then the pooled rounds; partial waves included."""
    rng = np.random.default_rng(1000 * K1 + 10 * need + n_act)
    sb = rng.integers(0, 2**32, LANES, dtype=np.uint64).astype(np.uint32)
    mask0 = sequential(sb, np.full(LANES, K1))
    mask0[n_act:] = 1  # lanes outside the tile never ran the pre-pass
    rounds = check(sb, mask0, need, n_act)
    if K1 == WINDOW:
        assert rounds == 0  # a full window is never needy


@pytest.mark.parametrize("seed", range(12))
def test_pool_from_random_windows(seed):
    """Random needy sets: every lane starts from its own number of drawn trials -- empty, partly drawn, one
    short of full (one trial of room: the share is cut to it), full -- so needs, ranks and shares differ per
    round; random wave-uniform need and a random active prefix."""
    rng = np.random.default_rng(seed)
    sb = rng.integers(0, 2**32, LANES, dtype=np.uint64).astype(np.uint32)
    d0 = rng.choice([0, 1, 2, 7, 13, 22, 29, 30, 30, 31], LANES)
    n_act = int(rng.choice([64, 64, 61, 33, 32, 17, 2]))
    need = int(rng.integers(1, WINDOW + 1))
    mask0 = sequential(sb, d0)
    check(sb, mask0, need, n_act)


def test_one_short_of_full_takes_one_trial():
    """All lanes at 30 drawn trials, none accepted enough: each round gives every needy lane a share of one
    lane or more, of which exactly one trial fits; one round fills every window."""
    rng = np.random.default_rng(7)
    sb = rng.integers(0, 2**32, LANES, dtype=np.uint64).astype(np.uint32)
    mask0 = sequential(sb, np.full(LANES, WINDOW - 1))
    got, rounds = pool_trials(sb, mask0, WINDOW, LANES)
    assert rounds == 1 and (drawn(got) == WINDOW).all()
    assert np.array_equal(got, sequential(sb, np.full(LANES, WINDOW)))
