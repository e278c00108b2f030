"""Wave model of the pre-pass with pooled top-up rounds (mm_trace.h predraw_trials, pool_trials).

One wave of 64 new paths, trials iid with acceptance pi / 6, a path reads `need` = bounce_limit - 1 accepted
trials (no mirrors, no tail chunks: scripts/predraw_model.py has those; their effect on the pre-pass is the
same in both arms).  Per chunk:

  own     K1 rounds, every lane one trial of its own stream (the loop of predraw_trials),
  pooled  rounds while a lane is needy (fewer than `need` accepted, window not full): the n needy lanes get
          2^k lanes each, the largest power of two (at most 32) with n 2^k <= 64, and take min(2^k, room),
  bounce  at bounce b = 1 .. need, rounds while a lane holds fewer than b accepted trials (every lane draws
          one trial per round: shade_step's loop; the window's sliding is ignored -- it only matters past
          31 undrawn trials).

Costs per round come from the ISA census of the compiled kernel (profiles/pool/isa_census_branch.txt,
scripts/isa_census.py --loops): VALU instructions and idealised quad-cycles (dual issue) of the own round, the
pooled round and the in-bounce round.

    python scripts/predraw_pool_model.py [--bounce-limit 8] > profiles/pool/model.txt
"""
from __future__ import annotations

import argparse
import math

import numpy as np

P_ACC = math.pi / 6.0
WINDOW = 31
LANES = 64


def chunk(rng, K1, pool, need):
    """(own rounds, pooled rounds, in-bounce rounds, lanes short after the pre-pass, trials drawn)."""
    acc = rng.random((LANES, 4096)) < P_ACC
    csum = np.cumsum(acc, axis=1)

    def have(d):  # accepted among the first d trials, per lane
        return np.where(d > 0, csum[np.arange(LANES), np.maximum(d, 1) - 1], 0)

    d = np.full(LANES, K1)
    trials = LANES * K1
    pooled = 0
    if pool:
        while True:
            needy = (have(d) < need) & (d < WINDOW)
            n = int(needy.sum())
            if not n:
                break
            pooled += 1
            k = 6 - (n.bit_length() - 1)
            if (n << k) > LANES:
                k -= 1
            k = min(k, 5)
            d = np.where(needy, np.minimum(d + (1 << k), WINDOW), d)
            trials += LANES
    short = int((have(d) < need).sum())
    inb = 0
    for b in range(1, need + 1):
        while (have(d) < b).any():
            d = d + 1
            inb += 1
            trials += LANES
    return K1, pooled, inb, short, trials


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=1500)
    ap.add_argument("--bounce-limit", type=int, default=8)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--valu-own", type=float, default=41.0)
    ap.add_argument("--valu-pool", type=float, default=73.0)
    ap.add_argument("--valu-round", type=float, default=62.0)
    ap.add_argument("--qc-own", type=float, default=20.5)
    ap.add_argument("--qc-pool", type=float, default=40.0)
    ap.add_argument("--qc-round", type=float, default=31.0)
    a = ap.parse_args()
    need = min(a.bounce_limit - 1, WINDOW)
    print(f"# pooled pre-pass, wave model: {a.chunks} chunks of 64 paths, bounce_limit {a.bounce_limit} (need {need}), "
          f"acceptance pi/6 = {P_ACC:.4f}")
    print(f"# per round, from the census of the compiled kernel: own {a.valu_own:.0f} VALU / {a.qc_own} quad-cycles, "
          f"pooled {a.valu_pool:.0f} / {a.qc_pool} (+ 2 table loads, 1 ds_permute, 1 ds_bpermute, 3 ballots), "
          f"in-bounce {a.valu_round:.0f} / {a.qc_round}")
    print("# share rule: n needy lanes get 2^k lanes each, k the largest with n 2^k <= active lanes, at most 32")
    print("# pool  K1 | pooled rounds  in-bounce rounds  lanes short after the pre-pass  trials/path | "
          "lane-VALU/path  quad-cycles/chunk")
    rows = {}
    for pool in (0, 1):
        for K1 in range(0, WINDOW + 1):
            rng = np.random.default_rng(a.seed)
            r = np.array([chunk(rng, K1, pool, need) for _ in range(a.chunks)], dtype=np.float64).mean(axis=0)
            valu = r[0] * a.valu_own + r[1] * a.valu_pool + r[2] * a.valu_round
            qc = r[0] * a.qc_own + r[1] * a.qc_pool + r[2] * a.qc_round
            rows[(pool, K1)] = (valu, qc)
            print(f"  {pool}    {K1:2d} | {r[1]:13.2f}  {r[2]:16.2f}  {100.0 * r[3] / LANES:29.3f}%  {r[4] / LANES:11.2f} | "
                  f"{valu:14.1f}  {qc:17.1f}")
    for pool in (0, 1):
        kv = min(range(WINDOW + 1), key=lambda k: rows[(pool, k)][0])
        kq = min(range(WINDOW + 1), key=lambda k: rows[(pool, k)][1])
        print(f"# pool {pool}: cheapest by lane-VALU at K1 = {kv} ({rows[(pool, kv)][0]:.1f} per path), by quad-cycles "
              f"at K1 = {kq} ({rows[(pool, kq)][1]:.1f} per chunk)")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
