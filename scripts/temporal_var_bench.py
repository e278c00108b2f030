#!/usr/bin/env python
"""Timing of mm_accumulate_frames_var against mm_accumulate_frames in the same
process, on one GPU, C3-sized (32x32 maze, 1920x1080, the frames, guides and
variances of a 20-camera Player walk at 8 spp, 8/8 bounces):

  * 1 frame and 20 frames per call, each behind a prev frame, so that every
    frame has a history frame; weights None and given (a per-pixel image of
    0.5 .. 4 frames in blocks);
  * per case: ms per frame of both calls, their ratio, and the fraction of the
    HBM peak on the bytes model below;
  * mm_accumulate_frames itself, timed first and again last: its code is
    the parent commit's, so its figures are the ones profiles/temporal/ab.txt
    holds.

The bytes model, per pixel of a frame with a history frame:

    frame colour + guides      16 + 36
    history colour + guides    16 + 36
    out                        16            = 120, mm_accumulate_frames' model
    vmean in                    4
    history variance in         4
    variance out                4            = 132: model ratio 1.10
    weights, when given        +4            = 136: model ratio 1.13

    python scripts/temporal_var_bench.py [--warmup 2] [--steps 5] [--still]

--still renders every frame from the walk's first camera (coherent taps), as
scripts/temporal_bench.py.  Each figure is HIP-event time on the stream over one
call, after --warmup calls of the same case; the median of --steps calls is
printed with their min and max, none dropped.  A different build of the
library: MIRROR_MAZE_LIB=/path/lib.so.
"""
from __future__ import annotations

import argparse
import statistics
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "mirror-maze_amd"))
sys.path.insert(0, str(REPO))

PLAIN_BYTES = 120         # mm_accumulate_frames: 52 in + 52 history + 16 out
VAR_BYTES = 132           # + vmean in, history variance in, variance out
WEIGHT_BYTES = 4          # + the weights, when given
HBM_PEAK_GBS = 8000.0     # MI355X, as bench.py's roofline has it


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
        color, var, _ = r.trace_tile_var(u, make_ext(8, 8, 8, frame=0), 0, 0, W, H, cameras=cams)
        aov = r.trace_aov(u, cams, 8, x0=0, y0=0, w=W, h=H)
        vmean = (var / 8.0).contiguous()
        del var
        gen = torch.Generator(device="cuda:0").manual_seed(1)
        blocks = torch.randint(0, 4, (frames + 1, (H + 7) // 8, (W + 15) // 16), generator=gen, device="cuda:0")
        weight = torch.tensor([0.5, 1.0, 2.0, 4.0], device="cuda:0")[blocks]
        weight = weight.repeat_interleave(8, 1).repeat_interleave(16, 2)[:, :H, :W].contiguous()
        r.sync()
        # frame 0 of the walk is the prev frame of every timed call; frames 1.. are accumulated
        g0 = {k: t[:1] for k, t in aov.items()}
        first = r.accumulate(u, cams[:1], color[:1], g0)
        prev = (first[0], g0, cams[0])
        first_v = r.accumulate_var(u, cams[:1], color[:1], g0, vmean[:1])
        prev_v = (first_v[0][0], g0, cams[0], first_v[1][0])
        out, vout = torch.empty_like(color[1:]), torch.empty_like(vmean[1:])
        print(f"# {W}x{H}, maze {a.maze}, {frames} {'still' if a.still else 'walk'} cameras behind a prev frame, 8 spp; "
              f"warmup {a.warmup}, steps {a.steps}; model {PLAIN_BYTES} B / pixel plain, {VAR_BYTES} with the variance "
              f"(ratio {VAR_BYTES / PLAIN_BYTES:.2f}), {VAR_BYTES + WEIGHT_BYTES} with weights "
              f"(ratio {(VAR_BYTES + WEIGHT_BYTES) / PLAIN_BYTES:.2f}); HBM peak {HBM_PEAK_GBS:.0f} GB/s")

        def plain(n):
            c, g, o = color[1:1 + n], {k: t[1:1 + n] for k, t in aov.items()}, out[:n]
            return timed(lambda: r.accumulate(u, cams[1:1 + n], c, g, prev=prev, out=o), a.warmup, a.steps)

        def show(tag, n, ms, nbytes, base=None):
            med = statistics.median(ms) / n
            gbs = nbytes * W * H / (med * 1e-3) / 1e9
            tail = "" if base is None else f", {med / base:.3f} of mm_accumulate_frames (model {nbytes / PLAIN_BYTES:.2f})"
            print(f"frames {n:2d}  {tag:<28s}: {med:.4f} ms/frame (min {min(ms) / n:.4f} max {max(ms) / n:.4f}), "
                  f"{gbs:7.1f} GB/s = {gbs / HBM_PEAK_GBS:.3f} of peak on {nbytes} B / pixel{tail}", flush=True)
            return med

        for n in (1, frames):
            base = show("mm_accumulate_frames", n, plain(n), PLAIN_BYTES)
            c, g, v = color[1:1 + n], {k: t[1:1 + n] for k, t in aov.items()}, vmean[1:1 + n]
            o, vo = out[:n], vout[:n]
            for tag, wt, nbytes in (("mm_accumulate_frames_var", None, VAR_BYTES),
                                    ("mm_accumulate_frames_var weights", weight[1:1 + n], VAR_BYTES + WEIGHT_BYTES)):
                ms = timed(lambda: r.accumulate_var(u, cams[1:1 + n], c, g, v, wt, prev=prev_v, out=o, var_out=vo),
                           a.warmup, a.steps)
                show(tag, n, ms, nbytes, base)
            show("mm_accumulate_frames again", n, plain(n), PLAIN_BYTES)
            hit = (g["id"] != -1) & (g["id"] != -2)
            print(f"frames {n:2d}  blended {100 * float((o[..., 3] > weight[1:1 + n])[hit].float().mean()):.1f} % of the "
                  f"non-miss pixels (weights given), mean Vout / mean vmean "
                  f"{float(vo.mean()) / float(v.mean()):.3f}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
