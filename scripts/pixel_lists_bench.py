#!/usr/bin/env python
"""Timing of mm_trace_pixel_lists on one GPU against one mm_trace_pixels call per
frame, C3-sized (32x32 maze, 1920x1080, 8 spp, 8/8 bounces): the cameras of a
20-frame walk (scripts/flythrough.py's), a seeded random 5 % list per frame
(sorted row-major, as torch.nonzero lists them), RNG frames 2^20 + 64 f.

  (a) 20 mm_trace_pixels calls, one per frame: the way without the call;
  (b) one mm_trace_pixel_lists call over the 20 lists;
  (c) control: one mm_trace_pixels call over the same 20 x 5 % entries with the
      first frame's camera -- the same number of paths in one launch, so (b) - (c)
      is what the per-chunk list lookup and camera load cost (and what the other
      19 cameras' paths cost more or less than the first's).

    python scripts/pixel_lists_bench.py [--frames 20] [--share 0.05] [--steps 9] [--var]

The legs alternate in one process: each of --steps rounds times (a), (b), (c)
once, HIP events on the stream around the leg's calls, after --warmup untimed
rounds.  Printed per leg: the median with min and max, none dropped; then
(b)/(a) and (b)/(c).  --var times the variance forms (mm_trace_pixels_var, var_dev
set).  A different build of the library: MIRROR_MAZE_LIB=/path/lib.so.
"""
from __future__ import annotations

import argparse
import statistics
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "mirror-maze_amd"))
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(Path(__file__).resolve().parent))


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--maze", type=int, default=32)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--share", type=float, default=0.05)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=9)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--var", action="store_true", help="the variance forms of all three legs")
    a = ap.parse_args(argv)

    import numpy as np
    import torch

    from flythrough import key_script
    from mirror_maze import Player, Renderer, Scene, make_ext, mm_camera, mm_uniform, walk_cameras

    W, H = 1920, 1080
    scene = Scene.build(a.maze, 0)
    player = Player(scene, W, H)
    cams = walk_cameras(player, key_script(a.frames, 8, 40.0))
    u = player.uniform()
    us = []
    for c in cams:
        uk = mm_uniform.from_buffer_copy(u)
        uk.cam = mm_camera.from_buffer_copy(np.ascontiguousarray(c, dtype=np.float32).tobytes())
        us.append(uk)
    e = make_ext(8, 8, 8, frame=0)
    keys = [2**20 + 64 * f for f in range(a.frames)]
    rng = np.random.default_rng(a.seed)
    n_share = int(round(a.share * W * H))
    lists = []
    for _ in range(a.frames):
        flat = np.sort(rng.choice(W * H, n_share, replace=False))
        lists.append(np.stack([flat % W, flat // W], axis=1).astype(np.int32))
    offsets = np.arange(a.frames + 1, dtype=np.uint64) * n_share
    dev = torch.device("cuda:0")
    with Renderer(0) as r:
        r.upload_scene(scene)
        every = torch.from_numpy(np.ascontiguousarray(np.concatenate(lists))).to(dev)
        per = [every[f * n_share:(f + 1) * n_share] for f in range(a.frames)]
        n = every.shape[0]
        out_a = torch.empty((n, 4), dtype=torch.float32, device=dev)
        out_b, out_c = torch.empty_like(out_a), torch.empty_like(out_a)
        var_a = torch.empty((n,), dtype=torch.float32, device=dev)
        var_b, var_c = torch.empty_like(var_a), torch.empty_like(var_a)
        exts = [make_ext(8, 8, 8, frame=k) for k in keys]

        def leg_a():
            for f in range(a.frames):
                s = slice(f * n_share, (f + 1) * n_share)
                if a.var:
                    r.trace_pixels_var(us[f], exts[f], per[f], out=out_a[s], var=var_a[s])
                else:
                    r.trace_pixels(us[f], exts[f], per[f], out=out_a[s])

        def leg_b():
            r.trace_pixel_lists(u, cams, e, every, offsets, frame_keys=keys, out=out_b, var=var_b if a.var else None)

        def leg_c():
            if a.var:
                r.trace_pixels_var(us[0], exts[0], every, out=out_c, var=var_c)
            else:
                r.trace_pixels(us[0], exts[0], every, out=out_c)

        legs = {"(a) one mm_trace_pixels call per frame": leg_a, "(b) one mm_trace_pixel_lists call": leg_b,
                "(c) one mm_trace_pixels call, one camera": leg_c}
        ms = {k: [] for k in legs}
        for step in range(a.warmup + a.steps):
            for name, fn in legs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if step >= a.warmup:
                    ms[name].append(e0.elapsed_time(e1))
        same = torch.equal(out_a, out_b) and (not a.var or torch.equal(var_a, var_b))
        print(f"# {W}x{H}, maze {a.maze}, 8 spp, 8/8 bounces, {a.frames} frames of the walk, {n_share} entries "
              f"({100 * a.share:.1f} %) per frame{', with the variance' if a.var else ''}; warmup {a.warmup}, "
              f"steps {a.steps}, legs alternating; seed {a.seed}")
        med = {}
        for name, v in ms.items():
            med[name[:3]] = statistics.median(v)
            print(f"{name}: {statistics.median(v):.4f} ms (min {min(v):.4f} max {max(v):.4f}), "
                  f"{statistics.median(v) / a.frames:.4f} ms per frame")
        print(f"(b)/(a) {med['(b)'] / med['(a)']:.3f}   (b)/(c) {med['(b)'] / med['(c)']:.3f}   "
              f"(b) bit-identical to (a): {same}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
