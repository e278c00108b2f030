#!/usr/bin/env python
"""Timing of mm_trace_pixels on one GPU against mm_trace_tile, C3-sized (32x32
maze, 1920x1080, 8 spp, 8/8 bounces, the default camera):

  (a) the list of ALL pixels in row-major order against mm_trace_tile of the
      same frame: what the record load and the missing tail rings cost;
  (b) a seeded, uniformly random 5 % of the pixels (sorted row-major, as
      torch.nonzero lists them);
  (c) 5 % of the pixels as 16x16 clumps at seeded places: what a disocclusion
      looks like.
  (b) and (c) are each reported against 5 % of the full frame's time, and so
  is a control: mm_trace_tile of 5 % of the frame's rows, what a launch that
  small costs without a list.

    python scripts/pixels_bench.py [--warmup 3] [--steps 9] [--share 0.05]

Each figure is HIP-event time on the stream over one call, after --warmup calls
of the same case; the median of --steps calls is printed with their min and
max, none dropped.  A different build of the library: MIRROR_MAZE_LIB=/path/lib.so.
"""
from __future__ import annotations

import argparse
import statistics
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "mirror-maze_amd"))
sys.path.insert(0, str(REPO))


def timed(fn, warmup, steps):
    """HIP-event ms of each of `steps` fn() calls on the current stream."""
    import torch

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def row_major(mask):
    """(n, 2) int32 (x, y) list of a (H, W) bool mask, row-major."""
    import numpy as np

    j, i = np.nonzero(mask)
    return np.ascontiguousarray(np.stack([i, j], axis=1).astype(np.int32))


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--maze", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=9)
    ap.add_argument("--share", type=float, default=0.05)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args(argv)

    import numpy as np
    import torch

    from mirror_maze import Renderer, Scene, default_uniform, make_ext

    W, H = 1920, 1080
    scene = Scene.build(a.maze, 0)
    u = default_uniform(W, H, 0)
    e = make_ext(8, 8, 8, frame=0)
    rng = np.random.default_rng(a.seed)
    n_share = int(round(a.share * W * H))
    every = row_major(np.ones((H, W), bool))
    scattered = np.zeros(W * H, bool)
    scattered[rng.choice(W * H, n_share, replace=False)] = True
    clumps = np.zeros((H, W), bool)
    while clumps.sum() < n_share:  # 16x16 clumps at seeded places (overlaps just add fewer pixels)
        x, y = int(rng.integers(0, W - 15)), int(rng.integers(0, H - 15))
        clumps[y:y + 16, x:x + 16] = True
    lists = {"(a) all pixels, row-major": every, "(b) random": row_major(scattered.reshape(H, W)),
             "(c) 16x16 clumps": row_major(clumps)}
    with Renderer(0) as r:
        r.upload_scene(scene)
        dev = torch.device("cuda:0")
        tile = torch.empty((H, W, 4), dtype=torch.float32, device=dev)
        t_tile = timed(lambda: r.trace_tile(u, e, 0, 0, W, H, out=tile), a.warmup, a.steps)
        full = statistics.median(t_tile)
        print(f"# {W}x{H}, maze {a.maze}, 8 spp, 8/8 bounces; warmup {a.warmup}, steps {a.steps}; seed {a.seed}")
        print(f"mm_trace_tile, the frame: {full:.4f} ms (min {min(t_tile):.4f} max {max(t_tile):.4f})", flush=True)
        # control: a tile of that share of the frame's rows -- what so small a launch costs without a list
        rows = max(1, int(round(a.share * H)))
        band = torch.empty((rows, W, 4), dtype=torch.float32, device=dev)
        t_band = timed(lambda: r.trace_tile(u, e, 0, (H - rows) // 2, W, rows, out=band), a.warmup, a.steps)
        print(f"mm_trace_tile, {rows} rows in mid-frame ({W * rows} pixels): {statistics.median(t_band):.4f} ms "
              f"(min {min(t_band):.4f} max {max(t_band):.4f}), "
              f"{statistics.median(t_band) / (rows / H * full):.3f} of that share of the frame's time", flush=True)
        for name, px in lists.items():
            p = torch.from_numpy(px).to(dev)
            out = torch.empty((len(px), 4), dtype=torch.float32, device=dev)
            ms = timed(lambda: r.trace_pixels(u, e, p, out=out), a.warmup, a.steps)
            med = statistics.median(ms)
            share = len(px) / (W * H)
            if name.startswith("(a)"):
                same = torch.equal(out.view(H, W, 4), tile)
                print(f"{name}: {len(px)} entries, {med:.4f} ms (min {min(ms):.4f} max {max(ms):.4f}), "
                      f"{med / full:.3f} of mm_trace_tile; bit-identical: {same}", flush=True)
            else:
                print(f"{name}: {len(px)} entries ({100 * share:.2f} % of the frame), {med:.4f} ms "
                      f"(min {min(ms):.4f} max {max(ms):.4f}), {med / (share * full):.3f} of that share of the "
                      f"frame's time ({share * full:.4f} ms)", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
