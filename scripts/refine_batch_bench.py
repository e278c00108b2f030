"""Wall time of one flythrough --refine batch (trace with variance + 2 refine rounds), the parent's way and the
branch's, alternating in one process; 20 frames of the walk, C3 scene, 1920x1080, 8 spp, tol 0.26, 24 spp extra."""
import statistics
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "mirror-maze_amd"))
sys.path.insert(0, str(Path(__file__).resolve().parent))

import numpy as np
import torch

from flythrough import key_script
from mirror_maze import Player, Renderer, Scene, make_ext, mm_camera, mm_uniform, walk_cameras

W, H, N, SPP, TOL, EXTRA, ROUNDS = 1920, 1080, 20, 8, 0.26, 24, 2
scene = Scene.build(32, 0)
player = Player(scene, W, H)
cams = walk_cameras(player, key_script(N, 8, 40.0))
u = player.uniform()
us = []
for c in cams:
    uk = mm_uniform.from_buffer_copy(u)
    uk.cam = mm_camera.from_buffer_copy(np.ascontiguousarray(c, dtype=np.float32).tobytes())
    us.append(uk)
e = make_ext(SPP, 8, 8, frame=0)

with Renderer(0) as r:
    r.upload_scene(scene)

    def before():
        img = torch.empty((N, H, W, 4), dtype=torch.float32, device="cuda:0")
        var = torch.empty((N, H, W), dtype=torch.float32, device="cuda:0")
        count = torch.full_like(var, float(SPP))
        for k in range(N):
            r.trace_tile_var(us[k], make_ext(SPP, 8, 8, frame=k), 0, 0, W, H, out=img[k], var=var[k])
        sel = []
        for k in range(N):
            for rnd in range(ROUNDS):
                n = r.refine(us[k], e, img[k], var[k], count[k], TOL, EXTRA, 2**20 + 64 * k + rnd)
                sel.append(n)
                if n == 0:
                    break
        return img, var, count, sum(sel)

    def after():
        img, var, _ = r.trace_tile_var(u, e, 0, 0, W, H, cameras=cams)
        count = torch.full_like(var, float(SPP))
        sel = 0
        for rnd in range(ROUNDS):
            n = r.refine_frames(u, cams, e, img, var, count, TOL, EXTRA, [2**20 + 64 * k + rnd for k in range(N)])
            sel += sum(n)
            if not any(n):
                break
        return img, var, count, sel

    t = {"before": [], "after": []}
    res = {}
    for step in range(1 + 5):
        for name, fn in (("before", before), ("after", after)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res[name] = fn()
            torch.cuda.synchronize()
            if step:
                t[name].append((time.perf_counter() - t0) * 1e3)
    same = all(torch.equal(a, b) for a, b in zip(res["before"][:3], res["after"][:3]))
    print(f"# one flythrough --refine batch: {N} frames {W}x{H}, maze 32, {SPP} spp, tol {TOL}, {EXTRA} spp extra, "
          f"{ROUNDS} rounds; wall time with a device sync, 5 alternating repeats after 1 warm-up")
    print(f"# selected pixel-rounds: before {res['before'][3]}, after {res['after'][3]} "
          f"({100.0 * res['after'][3] / (N * W * H * ROUNDS):.2f} % per frame and round); results bit-identical: {same}")
    for name, label in (("before", "frame by frame (trace_tile_var + refine per frame)"),
                        ("after", "batched (one trace_tile_var launch + refine_frames)")):
        v = t[name]
        print(f"{label}: {statistics.median(v):.2f} ms per batch (min {min(v):.2f} max {max(v):.2f}), "
              f"{statistics.median(v) / N:.3f} ms per frame")
    print(f"after / before {statistics.median(t['after']) / statistics.median(t['before']):.3f}")
