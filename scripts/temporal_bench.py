#!/usr/bin/env python
"""Timing of mm_accumulate_frames on one GPU, C3-sized (32x32 maze, 1920x1080,
the frames and guides of a 20-camera Player walk at 8 spp, 8/8 bounces):

  * 1 frame and 20 frames per call, each with a prev frame, so that every
    frame has a history frame (and 20 frames without one: frame 0 is a copy);
  * per case: ms per frame, the algorithmic bandwidth of the 120 B per pixel
    model (the frame: 16 B colour + 36 B of guides; the history frame: 16 B
    colour + 36 B of guides, every pixel of it once; 16 B out), its fraction of
    the HBM peak, and the share of the C3 frame's 2.006 ms;
  * the share of the pixels that were blended with their history.

    python scripts/temporal_bench.py [--warmup 2] [--steps 5] [--still]

--still renders every frame from the walk's first camera: every projection then
lands on its own pixel, so the taps are as coherent as loads get -- the
difference to the walk is what the gathers cost.

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

MODEL_BYTES = 120         # per pixel of a frame with a history frame: 52 in + 52 history + 16 out
HBM_PEAK_GBS = 8000.0     # MI355X, as bench.py's roofline has it
C3_FRAME_MS = 2.006       # the C3 frame, 20 frames per launch
DENOISE_MS = 0.405        # mm_denoise_frames, four passes (profiles/denoise/ab.txt)


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
    ap.add_argument("--still", action="store_true", help="every frame from the walk's first camera (coherent taps)")
    a = ap.parse_args(argv)

    import torch

    from mirror_maze import Player, Renderer, Scene, default_uniform, make_ext, walk_cameras

    W, H, frames = 1920, 1080, a.frames
    scene = Scene.build(a.maze, 0)
    u = default_uniform(W, H, 0)
    script = [([Player.KEY_W], [40.0] if f % 8 == 7 else []) for f in range(frames + 1)]
    cams = walk_cameras(Player(scene, W, H), script)
    if a.still:
        cams[:] = cams[0]
    with Renderer(0) as r:
        r.upload_scene(scene)
        color, _ = r.trace_tile_cameras(u, cams, make_ext(8, 8, 8, frame=0), 0, 0, W, H)
        aov = r.trace_aov(u, cams, 8, x0=0, y0=0, w=W, h=H)
        r.sync()
        # frame 0 of the walk is the prev frame of every timed call; frames 1.. are accumulated
        first = r.accumulate(u, cams[:1], color[:1], {k: t[:1] for k, t in aov.items()})
        prev = (first[0], {k: t[:1] for k, t in aov.items()}, cams[0])
        out = torch.empty_like(color[1:])
        print(f"# {W}x{H}, maze {a.maze}, {frames} {'still' if a.still else 'walk'} cameras behind a prev frame, 8 spp; "
              f"warmup {a.warmup}, steps {a.steps}; model {MODEL_BYTES} B / pixel, HBM peak {HBM_PEAK_GBS:.0f} GB/s, C3 frame {C3_FRAME_MS} ms, "
              f"denoise {DENOISE_MS} ms")
        for n, pv in ((1, prev), (frames, prev), (frames, None)):
            c, g, o = color[1:1 + n], {k: t[1:1 + n] for k, t in aov.items()}, out[:n]
            ms = timed(lambda: r.accumulate(u, cams[1:1 + n], c, g, prev=pv, out=o), a.warmup, a.steps)
            med = statistics.median(ms) / n
            gbs = MODEL_BYTES * W * H / (med * 1e-3) / 1e9
            hit = (g["id"] != -1) & (g["id"] != -2)  # neither MM_AOV_ID_MISS nor MM_AOV_ID_FAILED (int32 view)
            blended = (o[..., 3] > 1.0)
            print(f"frames {n:2d}  {'prev' if pv is not None else 'no prev'}: {med:.4f} ms/frame "
                  f"(min {min(ms) / n:.4f} max {max(ms) / n:.4f}), {gbs:7.1f} GB/s = {gbs / HBM_PEAK_GBS:.3f} of peak, "
                  f"{100 * med / C3_FRAME_MS:.1f} % of the C3 frame, {med / DENOISE_MS:.2f} of the denoise; blended "
                  f"{100 * float(blended.float().mean()):.1f} % of the pixels, "
                  f"{100 * float(blended[hit].float().mean()):.1f} % of the non-miss ones, "
                  f"mean history length {float(o[..., 3].mean()):.2f}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
