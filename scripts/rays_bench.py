#!/usr/bin/env python
"""Timing of mm_trace_rays on one GPU, C3-sized (32x32 maze, 1920x1080, 8 spp,
8/8 bounces, the default camera):

  (a) ALL pixels of the frame as a ray list -- the primary rays, keyed
      y*view_w + x, with MM_RAYS_JITTER -- against mm_trace_pixels over the
      same pixels, the two alternating in one process: what 32 B per entry
      instead of 8 B and a primary direction cost or save.  The outputs are
      compared on bits when the directions are the product's own (float32
      torch arithmetic may differ from them by an ulp, which is then said);
  (b) as many INCOHERENT rays: origins uniform in the corridors, directions
      uniform on the sphere -- a rate in paths and in closest-hit queries per
      second, beside mm_query_rays' rate for the same rays;
  (c) a 2048x1024 equirectangular panorama from the same camera.

    python scripts/rays_bench.py [--warmup 3] [--steps 9]

Each figure is HIP-event time on the stream over one call, after --warmup
calls; the median of --steps calls with their min and max, none dropped.  (a)'s
two arms alternate call by call, so drift hits both alike; their spread is the
run-to-run spread the comparison is read against.  A different build of the
library: MIRROR_MAZE_LIB=/path/lib.so (as scripts/ab.py sets it per arm).
"""
from __future__ import annotations

import argparse
import statistics
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "mirror-maze_amd"))
sys.path.insert(0, str(REPO))


def timed_pair(fns, warmup, steps):
    """HIP-event ms of each call, the functions alternating: [ms of fns[0]], [ms of fns[1]], ..."""
    import torch

    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(steps):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return ms


def fmt(ms):
    return f"{statistics.median(ms):.4f} ms (min {min(ms):.4f} max {max(ms):.4f})"


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--maze", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=9)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args(argv)

    import numpy as np
    import torch

    from mirror_maze import Renderer, Scene, default_uniform, equirect_rays, make_ext, pack_rays
    from mirror_maze.rays import rotate

    W, H = 1920, 1080
    n = W * H
    scene = Scene.build(a.maze, 0)
    u = default_uniform(W, H, 0)
    e = make_ext(8, 8, 8, frame=0)
    dev = torch.device("cuda:0")
    centre, quat = list(u.cam.center), list(u.cam.quat)
    print(f"# {W}x{H}, maze {a.maze}, 8 spp, 8/8 bounces; warmup {a.warmup}, steps {a.steps}; seed {a.seed}")
    with Renderer(0) as r:
        r.upload_scene(scene)
        # (a) the frame's primary rays: the pinhole of mm_device.h primary_dir in float32 torch
        y, x = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
        x, y = x.reshape(-1), y.reshape(-1)
        vx, vy = u.cam.viewport[0], u.cam.viewport[1]
        p = torch.stack([(vx * x.float()) / u.view_w - vx * 0.5, (vy * y.float()) / u.view_h - vy * 0.5,
                         torch.full((n,), float(u.cam.focal), device=dev)], dim=1)
        d = rotate(quat, p / p.norm(dim=1, keepdim=True))
        rays = pack_rays(torch.tensor(centre, device=dev).expand(n, 3), d, y * W + x)
        pixels = torch.stack([x, y], dim=1).to(torch.int32).contiguous()
        out_r = torch.empty((n, 4), dtype=torch.float32, device=dev)
        out_p = torch.empty((n, 4), dtype=torch.float32, device=dev)
        t_r, t_p = timed_pair([lambda: r.trace_rays(e, rays, jitter=True, out=out_r),
                               lambda: r.trace_pixels(u, e, pixels, out=out_p)], a.warmup, a.steps)
        differ = int((out_r.view(torch.int32) != out_p.view(torch.int32)).any(dim=1).sum())
        print(f"(a) mm_trace_rays, all {n} primary rays with the jitter: {fmt(t_r)}", flush=True)
        print(f"    mm_trace_pixels, the same pixels:                     {fmt(t_p)}")
        print(f"    rays / pixels = {statistics.median(t_r) / statistics.median(t_p):.4f}; the arms' own spread "
              f"(max - min) / median: rays {(max(t_r) - min(t_r)) / statistics.median(t_r):.4f}, pixels "
              f"{(max(t_p) - min(t_p)) / statistics.median(t_p):.4f}; entries differing from the pixel list's (torch's "
              f"directions, not bit-promised): {differ} of {n}", flush=True)
        # (b) incoherent rays: origins in the corridors' cells at eye height, directions uniform on the sphere
        g = torch.Generator(device=dev).manual_seed(a.seed)
        cell = torch.randint(0, a.maze, (n, 2), generator=g, device=dev).float()
        off = torch.rand((n, 3), generator=g, device=dev)
        base = -10.0 * (a.maze / 2)
        o = torch.stack([base + 10.0 * cell[:, 0] + 1.0 + 8.0 * off[:, 0], off[:, 1] - 0.5,
                         base + 10.0 * cell[:, 1] + 1.0 + 8.0 * off[:, 2]], dim=1)
        v = torch.randn((n, 3), generator=g, device=dev)
        inc = pack_rays(o, v / v.norm(dim=1, keepdim=True), torch.arange(n, device=dev))
        (t_i,) = timed_pair([lambda: r.trace_rays(e, inc, out=out_r)], a.warmup, a.steps)
        _, st = r.trace_rays(e, inc, out=out_r, stats=True)
        med = statistics.median(t_i)
        print(f"(b) mm_trace_rays, {n} incoherent rays: {fmt(t_i)}; {st.paths / med / 1e6:.2f} G paths/s, "
              f"{st.rays / med / 1e6:.2f} G closest-hit queries/s ({st.rays / st.paths:.2f} per path)", flush=True)
        (t_q,) = timed_pair([lambda: r.query_rays(inc.view(n, 2, 4))], a.warmup, a.steps)
        print(f"    mm_query_rays, the same rays (first hit only): {fmt(t_q)}; "
              f"{n / statistics.median(t_q) / 1e6:.2f} G rays/s", flush=True)
        # (c) the panorama
        pano = equirect_rays(centre, quat, 2048, 1024)
        out_c = torch.empty((2048 * 1024, 4), dtype=torch.float32, device=dev)
        (t_c,) = timed_pair([lambda: r.trace_rays(e, pano, out=out_c)], a.warmup, a.steps)
        print(f"(c) mm_trace_rays, a 2048x1024 panorama from the C3 camera: {fmt(t_c)} per frame", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
