#!/usr/bin/env python
"""Timing of the closest-hit calls on one GPU, C3-sized (32x32 maze, 1920x1080):

  * mm_trace_aov, mirror_limit 8: the default camera, and 20 cameras of a
    Player walk in one launch;
  * the C3 frame itself in the same session (20 frames in one
    mm_trace_tile_frames launch, 8 spp, 8/8 bounces), for the ratio;
  * mm_query_rays at 2^24 coherent rays (the C3 primaries, 8 per pixel with the
    trace's jitter scale) and 2^24 seeded incoherent rays (origins in the maze,
    uniform directions): rays per second.

    python scripts/aov_bench.py [--reps 3] [--launches 20]

Each figure is wall clock from the first enqueue to the stream's
synchronisation over --launches back-to-back calls, after a warm-up of the
same call; --reps repetitions are printed, none dropped.  A different build of
the library: MIRROR_MAZE_LIB=/path/lib.so.
"""
from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "mirror-maze_amd"))
sys.path.insert(0, str(REPO))


def timed(r, fn, launches):
    """ms per call of `launches` back-to-back fn() calls, enqueue to sync."""
    import torch

    fn()
    r.sync()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(launches):
        fn()
    r.sync()
    return (time.perf_counter() - t0) * 1e3 / launches


def primary_rays(u, n, W, H, spp, seed):
    """n rays like the trace's primaries: pixel i // spp, the camera's direction
    through it plus a jitter of 1e-3 (float32 torch arithmetic: the same rays
    up to rounding, which a timing does not need bit for bit)."""
    import torch

    g = torch.Generator(device="cuda").manual_seed(seed)
    i = torch.arange(n, device="cuda") // spp % (W * H)
    px, py = (i % W).float(), (i // W).float()
    vx, vy = u.cam.viewport[0], u.cam.viewport[1]
    p = torch.stack([vx * px / W - vx / 2, vy * py / H - vy / 2, torch.full_like(px, u.cam.focal)], dim=1)
    d = p / p.norm(dim=1, keepdim=True)
    q = torch.tensor(list(u.cam.quat)[:3], device="cuda")
    qw = u.cam.quat[3]
    t = 2 * torch.cross(q.expand_as(d), d, dim=1)
    d = d - qw * t + torch.cross(q.expand_as(d), t, dim=1)  # (the kernel's quat_mult turns by the conjugate)
    d[:, :2] += 1e-3 * (2 * torch.rand((n, 2), device="cuda", generator=g) - 1)
    rays = torch.zeros((n, 2, 4), device="cuda")
    rays[:, 0, :3] = torch.tensor(list(u.cam.center), device="cuda")
    rays[:, 1, :3] = d
    return rays


def random_rays(scene, n, seed):
    import torch

    g = torch.Generator(device="cuda").manual_seed(seed)
    half = 10.0 * scene.maze_n / 2
    rays = torch.zeros((n, 2, 4), device="cuda")
    rays[:, 0, 0] = (2 * torch.rand(n, device="cuda", generator=g) - 1) * half
    rays[:, 0, 1] = torch.rand(n, device="cuda", generator=g) * 6 - 5
    rays[:, 0, 2] = (2 * torch.rand(n, device="cuda", generator=g) - 1) * half
    d = torch.randn((n, 3), device="cuda", generator=g)
    rays[:, 1, :3] = d / d.norm(dim=1, keepdim=True)
    return rays


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--maze", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--mirrors", type=int, default=8)
    a = ap.parse_args(argv)

    import torch

    from mirror_maze import Player, Renderer, Scene, default_uniform, make_ext, walk_cameras

    W, H, frames = 1920, 1080, 20
    scene = Scene.build(a.maze, 0)
    u = default_uniform(W, H, 0)
    script = [([Player.KEY_W], [40.0] if f % 8 == 7 else []) for f in range(frames)]
    cams = walk_cameras(Player(scene, W, H), script)
    with Renderer(0) as r:
        r.upload_scene(scene)
        out1 = {"normal_depth": torch.empty((1, H, W, 4), device="cuda"), "albedo": torch.empty((1, H, W, 4), device="cuda"),
                "id": torch.empty((1, H, W), dtype=torch.int32, device="cuda")}
        outn = {k: torch.empty((frames,) + tuple(v.shape[1:]), dtype=v.dtype, device="cuda") for k, v in out1.items()}
        img = torch.empty((frames, H, W, 4), device="cuda")
        e = make_ext(8, 8, 8, frame=0)
        n = 1 << 24
        coherent, scattered = primary_rays(u, n, W, H, 8, 1), random_rays(scene, n, 2)
        hits = torch.empty((n, 2), dtype=torch.int32, device="cuda")
        cases = [
            ("trace_aov default camera, 1 frame / launch", 1,
             lambda: r.trace_aov(u, None, a.mirrors, x0=0, y0=0, w=W, h=H, out=out1)),
            ("trace_aov id only, 1 frame / launch", 1,
             lambda: r.trace_aov(u, None, a.mirrors, x0=0, y0=0, w=W, h=H, want=("id",), out=out1)),
            (f"trace_aov {frames} walk cameras / launch", frames,
             lambda: r.trace_aov(u, cams, a.mirrors, x0=0, y0=0, w=W, h=H, out=outn)),
            (f"trace_tile_frames {frames} frames / launch (the C3 frame)", frames,
             lambda: r.trace_tile_frames(u, e, frames, 0, 0, W, H, out=img)),
            ("query_rays 2^24 coherent", 0, lambda: r.query_rays(coherent, out=hits)),
            ("query_rays 2^24 incoherent", 0, lambda: r.query_rays(scattered, out=hits)),
        ]
        for rep in range(a.reps):
            for name, per, fn in cases:
                launches = a.launches if per == 1 else max(3, a.launches // 4)
                ms = timed(r, fn, launches)
                if per:
                    print(f"rep {rep}  {name}: {ms / per:.4f} ms/frame ({ms:.3f} ms/launch)", flush=True)
                else:
                    print(f"rep {rep}  {name}: {ms:.3f} ms, {n / ms / 1e6:.2f} G rays/s", flush=True)
        ids = out1["id"].view(-1)
        k = hits[:, 1]
        print(f"# default camera: {(ids == -1).float().mean().item():.4f} of the pixels miss; mirror hits per pixel "
              f"{out1['albedo'][..., 3].mean().item():.3f} (max {int(out1['albedo'][..., 3].max().item())}); "
              f"incoherent rays that hit: {(k != -1).float().mean().item():.4f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
