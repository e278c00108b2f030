#!/usr/bin/env python
"""Timing of tracing a lattice and rebuilding from the AOVs against tracing every
pixel, in one process, on one GPU, C3-sized (32x32 maze, 1920x1080, a 20-camera
Player walk at 8 spp, 8/8 bounces, 8 mirrors), scales 2 and 4, w_min 0.25:

  * Renderer.trace_tile_cameras over the full view: ms per frame;
  * the chain's stages, each timed alone: the low trace (the view / s), trace_aov
    at full resolution, mm_upsample_frames, and the fill -- select_holes_frames,
    ONE mm_trace_pixel_lists launch over the holes of all frames and one
    mm_fill_pixels call per frame -- and Renderer.trace_upsampled as a whole;
  * the fill's trace launched per frame instead (mm_trace_pixels, 20 launches),
    which is why it is one launch per batch;
  * mm_upsample_frames alone, 20 frames per call, in its four instances: ms per
    frame and the fraction of the HBM peak on the bytes model below, and the same
    for mm_accumulate_frames (120 B / pixel, scripts/temporal_bench.py), the
    kernel of the same block shape that is the yardstick;
  * the A/B of MM_OPT_UPSAMPLE_LDS: the taps gathered from memory (0) against the
    block's lattice footprint staged in LDS (1, the default, which every other
    figure here runs), alternating, three rounds.

The bytes model of mm_upsample_frames, per output pixel: the pixel's guides 36
(id 4, normal_depth 16, albedo 16) and its colour out 16, + 4 with the weight
output, + 4 with the variance output; per lattice pixel, i.e. / s^2: its colour
16, + 4 with the variance.  The lattice pixels' guides are output pixels'
guides, counted there; the four taps of neighbouring lanes share them, so the
model takes them as read from HBM once.

    python scripts/upsample_bench.py [--warmup 2] [--steps 5]

Each figure is HIP-event time on the stream over one call (the fill: over its
calls, the host's selection between them included), after --warmup calls of the
same case; the median of --steps calls is printed with their min and max, none
dropped.  A different build of the library: MIRROR_MAZE_LIB=/path/lib.so.
"""
from __future__ import annotations

import argparse
import statistics
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "mirror-maze_amd"))
sys.path.insert(0, str(REPO))

ACC_BYTES = 120           # mm_accumulate_frames: 52 in + 52 history + 16 out
HBM_PEAK_GBS = 8000.0     # MI355X, as bench.py's roofline has it
SCALES, W_MIN, SPP = (2, 4), 0.25, 8


def up_bytes(s, weight, var):
    return 36 + 16 + (4 if weight else 0) + (4 if var else 0) + (16 + (4 if var else 0)) / float(s * s)


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
    a = ap.parse_args(argv)

    import numpy as np
    import torch

    from mirror_maze import (Player, Renderer, Scene, default_uniform, make_ext, mm_camera, mm_uniform,
                             select_holes_frames, walk_cameras)
    from mirror_maze._lib import MM_OPT_UPSAMPLE_LDS

    W, H, n = 1920, 1080, a.frames
    scene = Scene.build(a.maze, 0)
    u = default_uniform(W, H, 0)
    script = [([Player.KEY_W], [40.0] if f % 8 == 7 else []) for f in range(n + 1)]
    cams_all = walk_cameras(Player(scene, W, H), script)
    cams = cams_all[1:]
    e = make_ext(SPP, 8, 8, frame=0)

    def show(tag, ms, per=n, nbytes=None, base=None):
        med = statistics.median(ms) / per
        tail = ""
        if nbytes is not None:
            gbs = nbytes * W * H / (med * 1e-3) / 1e9
            tail += f", {gbs:7.1f} GB/s = {gbs / HBM_PEAK_GBS:.3f} of peak on {nbytes:.2f} B / pixel"
        if base is not None:
            tail += f", {med / base:.3f} of the full trace"
        print(f"  {tag:<46s}: {med:.4f} ms/frame (min {min(ms) / per:.4f} max {max(ms) / per:.4f}){tail}", flush=True)
        return med

    with Renderer(0) as r:
        r.upload_scene(scene)
        print(f"# {W}x{H}, maze {a.maze}, {n} walk cameras, {SPP} spp, 8/8 bounces, 8 mirrors; warmup {a.warmup}, steps "
              f"{a.steps}; HBM peak {HBM_PEAK_GBS:.0f} GB/s", flush=True)
        out_full = torch.empty((n, H, W, 4), dtype=torch.float32, device="cuda:0")
        full = show("trace_tile_cameras, every pixel",
                    timed(lambda: r.trace_tile_cameras(u, cams, e, 0, 0, W, H, out=out_full), a.warmup, a.steps))
        aov = r.trace_aov(u, cams, 8, x0=0, y0=0, w=W, h=H)
        t_aov = show("trace_aov, full resolution",
                     timed(lambda: r.trace_aov(u, cams, 8, x0=0, y0=0, w=W, h=H, out=aov), a.warmup, a.steps), base=full)
        for s in SCALES:
            print(f"== scale {s} ==", flush=True)
            ul = mm_uniform.from_buffer_copy(u)
            ul.view_w, ul.view_h = float(W // s), float(H // s)
            lw, lh = W // s, H // s
            low = torch.empty((n, lh, lw, 4), dtype=torch.float32, device="cuda:0")
            t_low = show("low trace (trace_tile_cameras, view / s)",
                         timed(lambda: r.trace_tile_cameras(ul, cams, e, 0, 0, lw, lh, out=low), a.warmup, a.steps),
                         base=full)
            up = torch.empty((n, H, W, 4), dtype=torch.float32, device="cuda:0")
            t_up = show("mm_upsample_frames (colour + weight)",
                        timed(lambda: r.upsample(low, aov, s, W_MIN, out=up), a.warmup, a.steps),
                        nbytes=up_bytes(s, True, False), base=full)
            _, weight, _ = r.upsample(low, aov, s, W_MIN, out=up)

            def fill():
                pixels, offsets = select_holes_frames(weight0, 0, 0)
                extra, _, _ = r.trace_pixel_lists(u, cams, e, pixels, offsets)
                for f in range(n):
                    lo, hi = int(offsets[f]), int(offsets[f + 1])
                    if hi > lo:
                        r.fill_pixels(up[f], pixels[lo:hi], extra[lo:hi], 1.0, weight=weight[f])

            weight0 = weight.clone()  # (the fill sets the holes' weights: every timed fill selects from the same image)
            pixels, offsets = select_holes_frames(weight0, 0, 0)
            share = float(offsets[-1]) / float(n * W * H)
            t_fill = show(f"fill: select + ONE list launch + {n} fills", timed(fill, a.warmup, a.steps), base=full)

            def trace_lists():
                r.trace_pixel_lists(u, cams, e, pixels, offsets)

            def trace_per_frame():
                for f in range(n):
                    lo, hi = int(offsets[f]), int(offsets[f + 1])
                    if hi > lo:
                        uf = mm_uniform.from_buffer_copy(u)
                        uf.cam = mm_camera.from_buffer_copy(np.ascontiguousarray(cams[f], dtype=np.float32).tobytes())
                        r.trace_pixels(uf, make_ext(SPP, 8, 8, frame=f), pixels[lo:hi])

            show("  the holes in ONE mm_trace_pixel_lists launch", timed(trace_lists, a.warmup, a.steps), base=full)
            show(f"  the holes in {n} mm_trace_pixels launches", timed(trace_per_frame, a.warmup, a.steps), base=full)
            print(f"  holes {100.0 * share:.2f} % of the pixels; rays traced {1.0 / (s * s) + share:.3f} of the full frame's",
                  flush=True)
            show("sum of the stages (low + aov + upsample + fill)", [n * (t_low + t_aov + t_up + t_fill)], base=full)
            show("Renderer.trace_upsampled, the whole chain",
                 timed(lambda: r.trace_upsampled(u, cams, e, s, 0, 0, W, H, mirror_limit=8, w_min=W_MIN), a.warmup, a.steps),
                 base=full)
            # the kernel's four instances
            vlow = torch.rand((n, lh, lw), dtype=torch.float32, device="cuda:0")
            for tag, vm, ww in (("colour only", None, False), ("colour + weight", None, True),
                                ("colour + variance", vlow, False), ("colour + weight + variance", vlow, True)):
                show(f"mm_upsample_frames, {tag}",
                     timed(lambda: r.upsample(low, aov, s, W_MIN, vm, ww, out=up), a.warmup, a.steps),
                     nbytes=up_bytes(s, ww, vm is not None))
            # the taps gathered from memory against the lattice footprint staged in LDS (the default), alternating
            for rep in range(3):
                for lds in (0, 1):
                    r.set_option(MM_OPT_UPSAMPLE_LDS, lds)
                    show(f"A/B {rep}: colour + weight, {'LDS staging' if lds else 'direct gathers'}",
                         timed(lambda: r.upsample(low, aov, s, W_MIN, out=up), a.warmup, a.steps),
                         nbytes=up_bytes(s, True, False))
            r.set_option(MM_OPT_UPSAMPLE_LDS, 1)
            del low, up, vlow, weight, weight0
        print("== the yardstick ==", flush=True)
        g0 = {k: t[:1] for k, t in aov.items()}
        first = r.accumulate(u, cams[:1], out_full[:1], g0)
        prev = (first[0], g0, cams[0])
        acc = torch.empty_like(out_full[1:])
        g1 = {k: t[1:] for k, t in aov.items()}
        show(f"mm_accumulate_frames, {n - 1} frames behind a prev",
             timed(lambda: r.accumulate(u, cams[1:], out_full[1:], g1, prev=prev, out=acc), a.warmup, a.steps),
             per=n - 1, nbytes=ACC_BYTES)
        r.sync()
    return 0


if __name__ == "__main__":
    sys.exit(main())
