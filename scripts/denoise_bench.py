#!/usr/bin/env python
"""Timing of mm_denoise_frames on one GPU, C3-sized (32x32 maze, 1920x1080, the
frames and guides of a 20-camera Player walk at 8 spp, 8/8 bounces):

  * 1 frame and 20 frames per call, n_passes 1..5, float and RGBA8 output;
  * per case: ms per frame, the algorithmic bandwidth of the 56 B per
    pixel-pass model (16 B colour in, 16 B out, 24 B of guides), its fraction
    of the HBM peak, and the share of the C3 frame's 2.006 ms;

    python scripts/denoise_bench.py [--warmup 2] [--steps 5]

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

MODEL_BYTES = 56          # per pixel-pass: 16 colour in + 16 colour out + 24 guides
HBM_PEAK_GBS = 8000.0     # MI355X, as bench.py's roofline has it
C3_FRAME_MS = 2.006       # the C3 frame, 20 frames per launch


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


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--maze", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--max-passes", type=int, default=5)
    a = ap.parse_args(argv)

    import torch

    from mirror_maze import Player, Renderer, Scene, default_uniform, make_ext, walk_cameras

    W, H, frames = 1920, 1080, a.frames
    scene = Scene.build(a.maze, 0)
    u = default_uniform(W, H, 0)
    script = [([Player.KEY_W], [40.0] if f % 8 == 7 else []) for f in range(frames)]
    cams = walk_cameras(Player(scene, W, H), script)
    with Renderer(0) as r:
        r.upload_scene(scene)
        color, _ = r.trace_tile_cameras(u, cams, make_ext(8, 8, 8, frame=0), 0, 0, W, H)
        aov = r.trace_aov(u, cams, 8, x0=0, y0=0, w=W, h=H)
        r.sync()
        outs = {False: torch.empty_like(color), True: torch.empty(color.shape, dtype=torch.uint8, device=color.device)}
        print(f"# {W}x{H}, maze {a.maze}, {frames} walk cameras, 8 spp; warmup {a.warmup}, steps {a.steps}; "
              f"model {MODEL_BYTES} B / pixel-pass, HBM peak {HBM_PEAK_GBS:.0f} GB/s, C3 frame {C3_FRAME_MS} ms")
        for n in (1, frames):
            c, g = color[:n], {k: t[:n] for k, t in aov.items()}
            for rgba8 in (False, True):
                o = outs[rgba8][:n]
                for n_passes in range(1, a.max_passes + 1):
                    ms = timed(lambda: r.denoise(c, g, n_passes=n_passes, out=o), a.warmup, a.steps)
                    med = statistics.median(ms) / n
                    gbs = MODEL_BYTES * W * H * n_passes / (med * 1e-3) / 1e9
                    print(f"frames {n:2d}  {'rgba8' if rgba8 else 'float'}  "
                          f"passes {n_passes}: {med:.4f} ms/frame (min {min(ms) / n:.4f} max {max(ms) / n:.4f}), "
                          f"{med / n_passes:.4f} ms/pass, {gbs:7.1f} GB/s = {gbs / HBM_PEAK_GBS:.3f} of peak, "
                          f"{100 * med / C3_FRAME_MS:.1f} % of the C3 frame", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
