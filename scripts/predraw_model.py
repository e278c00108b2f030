"""Wave model of the rejection-sampling trial loop (mm_trace.h shade_step).

Counts, for one wave of 64 lanes, the wave-iterations the direction sampling
costs per 64-path chunk under

  bank   the two-trial look-ahead bank (the kernel up to this model), and
  mask   the trial window: K trials per lane pre-drawn at a new-path chunk's
         start into an accept mask (31 trials of room), rounds in the bounce
         only while a lane that will read its direction has no accepted trial,
         with and without the last-bounce rule (a diffuse lane at its last
         bounce requests no sample).

Inputs (profiles/cert_fast/lane_stats_c3_branch.txt): trials are
iid with acceptance pi/6; 3.8 % of lane-bounces are mirror bounces; paths run
bounce_limit non-mirror bounces; at most 32 live lanes park into the tail ring
and come back 64 at a time as tail chunks, which carry their bank / window and
run no pre-pass.  The model is believed only if its `bank` row reproduces the
measured 2.93 loop iterations per diffuse wave-bounce.

Cost columns are quad-cycles per new-path chunk (tail chunks' share included)
from the per-iteration figures given on the command line; the defaults are the
censuses of the bank loop (28), of the pre-pass round (20.5) and of the mask
scheme's in-bounce round (31; profiles/predraw/isa_census_*.txt) and desk
estimates for the straight-line parts (the bank's in-line trial, the mask
scheme's redraw of the taken trial).

    python scripts/predraw_model.py [--chunks 1500] [--bounce-limit 8] > profiles/predraw/model.txt
"""
from __future__ import annotations

import argparse
import math

import numpy as np

P_ACC = math.pi / 6.0
WINDOW = 31


class Stats:
    def __init__(self):
        self.new_chunks = 0
        self.tail_chunks = 0
        self.wave_bounces = 0      # wave-bounces with at least one diffuse lane
        self.loop_iters = 0        # in-bounce trial-loop iterations / rounds
        self.pre_rounds = 0        # pre-pass rounds
        self.iters_b0 = 0          # ... of a new chunk's first bounce
        self.last_iters = 0        # iterations run only for lanes at their last bounce
        self.samples = 0           # direction samples that were read or drawn for a lane-bounce
        self.trials = 0            # lane-trials drawn (any lane, any round)


def run(scheme: str, K: int, last_rule: bool, chunks: int, bl: int, ml: int, p_mirror: float, park_at: int,
        seed: int) -> Stats:
    rng = np.random.default_rng(seed)
    st = Stats()
    pool = []  # parked lanes: (n, mh, a, b) -- bank: (bank, 0); mask: (mask, 0)

    def wave(n, mh, a, fresh):
        """Run one chunk's bounce loop; a: bank count (bank) or accept mask with sentinel (mask)."""
        live = np.ones(len(n), bool)
        defer = len(n) > park_at
        first = True
        while live.any():
            mirror = live & (rng.random(len(n)) < p_mirror)
            diffuse = live & ~mirror
            # a diffuse lane reads its new direction unless this is its last bounce
            wants = diffuse & (n + 1 < bl + mh) if last_rule else diffuse
            it = 0
            if diffuse.any():
                st.wave_bounces += 1
            if scheme == "bank":
                banked = a > 0
                acc = rng.random(len(n)) < P_ACC
                st.trials += int((diffuse & ~banked).sum())
                need = diffuse & ~banked & ~acc
                a = np.where(diffuse & banked, a - 1, a)
                only_last = need & ~(n + 1 < bl + mh)
                while need.any():
                    if not (need & ~only_last).any():
                        st.last_iters += 1
                    it += 1
                    acc = rng.random(len(n)) < P_ACC
                    act = diffuse & (a < 2)
                    st.trials += int(act.sum())
                    take = need & acc
                    a = a + (acc & act & ~take)
                    need = need & ~take
            else:
                need = wants & ((a & (a - 1)) == 0)
                while need.any():
                    it += 1
                    full_empty = a == (1 << WINDOW)
                    a = np.where(diffuse & full_empty, 1, a)
                    room = diffuse & (a < (1 << WINDOW))
                    d = np.floor(np.log2(a)).astype(np.int64)
                    acc = rng.random(len(n)) < P_ACC
                    st.trials += int(room.sum())
                    a = np.where(room, a + ((1 + acc.astype(np.int64)) << d), a)
                    need = need & ((a & (a - 1)) == 0)
                i = np.floor(np.log2(a & -a)).astype(np.int64)
                a = np.where(wants, a >> (i + 1), a)
            st.loop_iters += it
            if first and fresh:
                st.iters_b0 += it
            first = False
            st.samples += int(wants.sum() if scheme == "mask" else diffuse.sum())
            mh = mh + mirror
            live = live & ~(mirror & (mh >= ml))
            n = n + live
            live = live & (n < bl + mh)
            if defer and 0 < live.sum() <= park_at:
                for j in np.nonzero(live)[0]:
                    pool.append((int(n[j]), int(mh[j]), int(a[j])))
                return

    for _ in range(chunks):
        st.new_chunks += 1
        a = np.zeros(64, np.int64)
        if scheme == "mask":
            a = np.ones(64, np.int64) << K
            for r in range(K):
                acc = rng.random(64) < P_ACC
                a |= acc.astype(np.int64) << r
            st.pre_rounds += K
            st.trials += 64 * K
        wave(np.zeros(64, np.int64), np.zeros(64, np.int64), a, True)
        while len(pool) >= 64:
            take, pool[:] = pool[:64], pool[64:]
            st.tail_chunks += 1
            t = np.array(take, np.int64)
            wave(t[:, 0].copy(), t[:, 1].copy(), t[:, 2].copy(), False)
    while pool:  # the drain: whatever the ring still holds, deferral off below park_at lanes
        take, pool[:] = pool[:64], pool[64:]
        st.tail_chunks += 1
        t = np.array(take, np.int64)
        wave(t[:, 0].copy(), t[:, 1].copy(), t[:, 2].copy(), False)
    return st


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=1500)
    ap.add_argument("--bounce-limit", type=int, default=8)
    ap.add_argument("--mirror-limit", type=int, default=8)
    ap.add_argument("--p-mirror", type=float, default=0.038)
    ap.add_argument("--park-at", type=int, default=32)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--qc-bank-iter", type=float, default=28.0, help="quad-cycles per bank loop iteration")
    ap.add_argument("--qc-inline", type=float, default=22.0, help="the bank scheme's in-line trial per diffuse bounce")
    ap.add_argument("--qc-pre", type=float, default=20.5, help="per pre-pass round")
    ap.add_argument("--qc-round", type=float, default=31.0, help="per in-bounce round of the mask scheme")
    ap.add_argument("--qc-take", type=float, default=24.0, help="the mask scheme's redraw of the taken trial")
    a = ap.parse_args()
    common = (a.chunks, a.bounce_limit, a.mirror_limit, a.p_mirror, a.park_at, a.seed)
    print(f"# wave model: {a.chunks} new-path chunks, bounce_limit {a.bounce_limit}, mirror_limit {a.mirror_limit}, "
          f"p(mirror) {a.p_mirror}, park at <= {a.park_at} live lanes, acceptance pi/6 = {P_ACC:.4f}")
    b = run("bank", 0, False, *common)
    print("# the two-trial bank (measured on C3: 2.93 loop iterations per diffuse wave-bounce)")
    print(f"bank: iterations per new-path chunk {b.loop_iters / b.new_chunks:6.2f} (tail chunks' share included), "
          f"per diffuse wave-bounce {b.loop_iters / b.wave_bounces:5.2f}, bounce 0 alone "
          f"{b.iters_b0 / b.new_chunks:5.2f}, for last-bounce lanes only {b.last_iters / b.new_chunks:5.2f}; "
          f"tail chunks per new chunk {b.tail_chunks / b.new_chunks:5.3f}; "
          f"trials drawn per lane-sample {b.trials / b.samples:5.2f}")
    cost_bank = (b.loop_iters * a.qc_bank_iter + b.wave_bounces * a.qc_inline) / b.new_chunks
    print(f"bank: cost {cost_bank:7.1f} quad-cycles per chunk "
          f"({a.qc_bank_iter} per iteration, {a.qc_inline} per in-line trial)")
    print("# the trial window; cost = K pre-pass rounds + in-bounce rounds + one redraw per diffuse wave-bounce")
    print("#  K  last-bounce rule | rounds/chunk  per wave-bounce  trials/sample | cost qc/chunk  vs bank")
    best = None
    for last_rule in (False, True):
        for K in range(0, WINDOW + 1):
            m = run("mask", K, last_rule, *common)
            cost = (m.pre_rounds * a.qc_pre + m.loop_iters * a.qc_round + m.wave_bounces * a.qc_take) / m.new_chunks
            print(f"  {K:2d}  {'on ' if last_rule else 'off'}              | {m.loop_iters / m.new_chunks:11.2f}  "
                  f"{m.loop_iters / m.wave_bounces:14.2f}  {m.trials / max(m.samples, 1):13.2f} | {cost:12.1f}  "
                  f"{100.0 * (cost / cost_bank - 1.0):+6.1f} %")
            if last_rule and (best is None or cost < best[1]):
                best = (K, cost)
    print(f"# cheapest K with the last-bounce rule at bounce_limit {a.bounce_limit}: {best[0]} "
          f"({best[1]:.1f} quad-cycles per chunk, {100.0 * (best[1] / cost_bank - 1.0):+.1f} % against the bank)")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
