#!/usr/bin/env python
"""What the variance-guided filter (Renderer.denoise_var) buys over the
fixed-stop filter (Renderer.denoise), on the two scenes of the README's denoise
line: the maze N=4 at 160x120 and the mirror corridor of the feature-buffer
tests (tests/golden/aov_corridor.npz) at 140x32, 8 spp, 8/8 bounces, 8 mirrors.
Every figure is MSE over rgb against a 512-spp frame drawn with another RNG
frame, as a fraction of the raw 8-spp frame's:

  * three inputs: the 8-spp frame; a uniform 16-spp frame; and the 8-spp frame
    after one Renderer.refine round that gives the noisiest quarter of the
    pixels 32 more samples (8 + 32 / 4 = 16 on average, the 16-spp frame's
    budget; the round's rel_tol is found by bisection on select_noisy) --
    neighbours then hold 8 and 40 samples, which only denoise_var is told;
  * on each: denoise at its defaults and denoise_var at its defaults;
  * the sweep the defaults of denoise_var were chosen from: n_passes x sigma_l x
    eps_l around SVGF's 5 / 4 / 1e-3, on the 8-spp frame and on the refined one,
    ranked by the geometric mean of the four fractions (two scenes, two inputs);
  * how well the returned variance predicts the error: mean(var_out) / mean
    (squared luminance error of the output against the 512-spp frame), per
    n_passes.  var_out takes a pass's taps as independent; from the second pass
    on they share inputs, so it understates the variance more with every pass.
    The measured error also holds what no variance predicts: the filter's bias
    and the 512-spp frame's own noise (printed: 1/64 of the 8-spp mean's).

    python scripts/denoise_var_quality.py [--out profiles/denoise_var/quality.txt]

Nothing here is a threshold; the figures are written down as measured.
"""
from __future__ import annotations

import argparse
import inspect
import itertools
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "mirror-maze_amd"))
sys.path.insert(0, str(REPO))

PASSES = (3, 4, 5)
SIGMA_L = (2.0, 4.0, 8.0, 16.0)
EPS_L = (1e-3, 1e-2, 5e-2)


def lum(c):
    return 0.25 * c[..., 0] + 0.5 * c[..., 1] + 0.25 * c[..., 2]


def share_tol(select_noisy, color, var, count, share, ids):
    """rel_tol at which select_noisy names `share` of the pixels (bisection)."""
    lo, hi = 0.0, 64.0
    n = color.shape[0] * color.shape[1]
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        if select_noisy(color, var, count, mid, ids=ids).shape[0] > share * n:
            lo = mid
        else:
            hi = mid
    return hi


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", type=Path, default=REPO / "profiles" / "denoise_var" / "quality.txt")
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
    uc.view_w, uc.view_h, uc.chunk_w, uc.time = 140.0, 32.0, 4, 0
    cases = [("maze 4, 160x120", Scene.build(4, 0), default_uniform(160, 120, 0), 160, 120),
             ("mirror corridor, 140x32", corridor, uc, 140, 32)]
    sig = inspect.signature(Renderer.denoise_var).parameters
    dflt = {k: sig[k].default for k in ("n_passes", "sigma_z", "sigma_l", "eps_l")}
    lines = ["# denoise_var_quality: 8 spp, 8/8 bounces, 8 mirrors; MSE over rgb against a 512-spp frame (RNG frame "
             "777), as a fraction of the raw 8-spp frame's",
             f"# denoise_var defaults: n_passes {dflt['n_passes']}, sigma_z {dflt['sigma_z']}, sigma_l "
             f"{dflt['sigma_l']}, eps_l {dflt['eps_l']}; denoise defaults: 4 / 0.02 / 0.5"]
    sweep = {}
    for name, scene, u, w, h in cases:
        with Renderer(0) as r:
            r.upload_scene(scene)
            truth, _ = r.trace_tile(u, make_ext(512, 8, 8, frame=777), 0, 0, w, h)
            t = truth.double()
            aov = r.trace_aov(u, None, 8, x0=0, y0=0, w=w, h=h)
            e8 = make_ext(8, 8, 8, frame=0)
            c8, v8, _ = r.trace_tile_var(u, e8, 0, 0, w, h)
            c16, v16, _ = r.trace_tile_var(u, make_ext(16, 8, 8, frame=0), 0, 0, w, h)

            def mse(img):
                return float(((img.double()[..., :3] - t[..., :3]) ** 2).mean())

            raw = mse(c8)
            cr, vr = c8.clone(), v8.clone()
            nr = torch.full((h, w), 8.0, dtype=torch.float32, device=c8.device)
            tol = share_tol(select_noisy, cr, vr, nr, 0.25, aov["id"])
            n = r.refine(u, e8, cr, vr, nr, tol, 32, 2**20, ids=aov["id"])
            lines.append(f"== {name}: {w * h} pixels; raw 8 spp MSE {raw:.6g}; "
                         f"{100.0 * float((v8 > 0).double().mean()):.1f} % of the pixels have a variance above 0 ==")
            lines.append(f"  refine round: rel_tol {tol:.4f}, {n} pixels ({100.0 * n / (w * h):.2f} %) x 32 spp -> "
                         f"{float(nr.double().sum()) / (w * h):.3f} samples per pixel")
            inputs = (("8 spp", c8, v8, 8.0), ("16 spp", c16, v16, 16.0), ("8 spp + refine", cr, vr, nr))
            lines.append("  input            raw     denoise  denoise_var  (defaults)")
            for what, c, v, cnt in inputs:
                lines.append(f"  {what:15s}  {mse(c) / raw:.4f}  {mse(r.denoise(c, aov)) / raw:.4f}   "
                             f"{mse(r.denoise_var(c, aov, v, cnt)) / raw:.4f}")
            lines.append("  sweep of denoise_var, sigma_z 0.02: fraction on the 8-spp frame / on the refined frame "
                         "(rows: n_passes, sigma_l; columns: eps_l " + ", ".join(f"{e:g}" for e in EPS_L) + "):")
            for n_passes, sl in itertools.product(PASSES, SIGMA_L):
                row = []
                for eps in EPS_L:
                    kw = dict(n_passes=n_passes, sigma_l=sl, eps_l=eps)
                    m8 = mse(r.denoise_var(c8, aov, v8, 8.0, **kw)) / raw
                    mr = mse(r.denoise_var(cr, aov, vr, nr, **kw)) / raw
                    sweep.setdefault((n_passes, sl, eps), []).extend((m8, mr))
                    row.append(f"{m8:.4f} / {mr:.4f}")
                lines.append(f"    passes {n_passes}  sigma_l {sl:4.1f}:  " + "    ".join(row))
            # the returned variance against the measured error
            floor = float((v8.double() / 8.0).mean()) / 64.0
            lines.append(f"  the 512-spp frame's own luminance variance, mean(var / 8) / 64: {floor:.4g}")
            for what, c, v, cnt in inputs[::2]:
                for n_passes in (1, 2, 3, 4, 5):
                    out, vout = r.denoise_var(c, aov, v, cnt, n_passes=n_passes, return_var=True)
                    err2 = float(((lum(out.double()) - lum(t)) ** 2).mean())
                    pred = float(vout.double().mean())
                    lines.append(f"  {what}, {n_passes} passes: mean(var_out) {pred:.4g} / mean(lum error^2) {err2:.4g} "
                                 f"= {pred / err2:.3f}")
    lines.append("== sweep, geometric mean of the four fractions (maze 8 spp, maze refined, corridor 8 spp, corridor "
                 "refined), best ten ==")
    best = sorted(sweep.items(), key=lambda kv: float(np.prod(kv[1])))[:10]
    for (n_passes, sl, eps), ms in best:
        lines.append(f"  passes {n_passes}  sigma_l {sl:4.1f}  eps_l {eps:g}:  {float(np.prod(ms)) ** 0.25:.4f}  ("
                     + ", ".join(f"{m:.4f}" for m in ms) + ")")
    text = "\n".join(lines) + "\n"
    a.out.parent.mkdir(parents=True, exist_ok=True)
    a.out.write_text(text)
    sys.stdout.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
