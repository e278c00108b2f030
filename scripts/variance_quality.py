#!/usr/bin/env python
"""What noise-driven sampling buys at equal total samples, and how well the
per-pixel variance is calibrated, on the 32x32 maze (640x360, the default
camera) and on the mirror corridor of the feature-buffer tests
(tests/golden/aov_corridor.npz, 536x384):

  * uniform 16 spp against 8 spp plus two rounds of Renderer.refine, each giving
    the noisiest quarter of the pixels 16 more samples -- 8 + 2 * 16 / 4 = 16
    samples per pixel on average, the same budget (each round's rel_tol is
    found by bisection on select_noisy so that the round selects a quarter);
    both as MSE against a 512-spp frame drawn with another RNG frame;
  * the calibration ratio mean(var / spp) / mean(squared luminance error of the
    8-spp mean against the 512-spp frame), 1 in expectation (the 512-spp frame's
    own variance, 1/64 of the 8-spp mean's, counts as error: expect ~0.98), with
    the pixel count, and the same ratio after the rounds (var / count).

    python scripts/variance_quality.py [--out profiles/variance/quality.txt]

Nothing here is a threshold; the figures are written down as measured.
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "mirror-maze_amd"))
sys.path.insert(0, str(REPO))


def lum(c):
    return 0.25 * c[..., 0] + 0.5 * c[..., 1] + 0.25 * c[..., 2]


def quarter_tol(select_noisy, color, var, count, share):
    """rel_tol at which select_noisy names `share` of the pixels (bisection)."""
    lo, hi = 0.0, 64.0
    n = color.shape[0] * color.shape[1]
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        if select_noisy(color, var, count, mid).shape[0] > share * n:
            lo = mid
        else:
            hi = mid
    return hi


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", type=Path, default=REPO / "profiles" / "variance" / "quality.txt")
    a = ap.parse_args(argv)

    import ctypes as C

    import numpy as np
    import torch

    from mirror_maze import Renderer, Scene, default_uniform, make_ext, mm_uniform, select_noisy

    z = np.load(REPO / "tests" / "golden" / "aov_corridor.npz")
    corridor = Scene(0, z["rects"], np.ascontiguousarray(z["nodes"]), z["idx"], z["is_mirror"], z["emission"],
                     np.zeros((0, 0), np.uint8), 0)
    uc = mm_uniform()
    C.memmove(C.byref(uc), np.ascontiguousarray(z["camera"], dtype=np.float32).ctypes.data, 40)
    uc.view_w, uc.view_h, uc.chunk_w, uc.time = 536.0, 384.0, 4, 0
    cases = [("maze 32, 640x360", Scene.build(32, 0), default_uniform(640, 360, 0), 640, 360, 8),
             ("mirror corridor, 536x384", corridor, uc, 536, 384, 15)]
    lines = ["# variance_quality: 8/8 bounces (corridor: 8 bounces, 15 mirrors); MSE over rgb against a 512-spp frame "
             "(RNG frame 777)"]
    for name, scene, u, w, h, mirrors in cases:
        with Renderer(0) as r:
            r.upload_scene(scene)
            truth, _ = r.trace_tile(u, make_ext(512, 8, mirrors, frame=777), 0, 0, w, h)
            t = truth.double()
            uniform16, _ = r.trace_tile(u, make_ext(16, 8, mirrors, frame=0), 0, 0, w, h)
            e8 = make_ext(8, 8, mirrors, frame=0)
            color, var, _ = r.trace_tile_var(u, e8, 0, 0, w, h)
            count = torch.full((h, w), 8.0, dtype=torch.float32, device=color.device)

            def mse(img):
                return float(((img.double()[..., :3] - t[..., :3]) ** 2).mean())

            def calib(img, v, cnt):
                err2 = (lum(img.double()) - lum(t)) ** 2
                return float((v.double() / cnt).mean() / err2.mean())

            lines.append(f"== {name}: {w * h} pixels ==")
            lines.append(f"  uniform 8 spp:   MSE {mse(color):.6g}   ({8 * w * h} samples)")
            lines.append(f"  uniform 16 spp:  MSE {mse(uniform16):.6g}   ({16 * w * h} samples)")
            lines.append(f"  calibration at 8 spp: mean(var/spp) / mean(lum error^2) = {calib(color, var, 8.0):.4f} "
                         f"over {w * h} pixels")
            for rnd in range(2):
                tol = quarter_tol(select_noisy, color, var, count, 0.25)
                n = r.refine(u, e8, color, var, count, tol, 16, 2**20 + rnd)
                lines.append(f"  refine round {rnd + 1}: rel_tol {tol:.4f}, {n} pixels ({100.0 * n / (w * h):.2f} %) x 16 spp")
            spent = int(count.double().sum())
            lines.append(f"  8 spp + refine:  MSE {mse(color):.6g}   ({spent} samples, {spent / (w * h):.3f} per pixel)  "
                         f"= {mse(color) / mse(uniform16):.3f} x the uniform 16 spp's")
            lines.append(f"  calibration after the rounds: mean(var/count) / mean(lum error^2) = "
                         f"{calib(color, var, count.double()):.4f}")
    text = "\n".join(lines) + "\n"
    a.out.parent.mkdir(parents=True, exist_ok=True)
    a.out.write_text(text)
    sys.stdout.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
