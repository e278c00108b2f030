#!/usr/bin/env python3
"""Desk model behind mm_accumulate_frames_var's variance estimator: iid noise
under repeated bilinear reprojection.

Every frame is an image of independent unit-variance noise.  Frame f's history
is frame f-1's accumulated image resampled bilinearly at a constant sub-pixel
shift (a, b), and the two are blended as the library does: N = min(N' + 1,
n_max), out = H + (C - H) / N.  The accumulated pixel is then a linear
combination of the frames' noise values, so its ACTUAL variance is the sum of
the squared coefficients -- tracked here exactly, as a coefficient image per
frame, no sampling.  Against it stand two estimators carried through the same
recursion (the model is translation invariant, so each is one number per frame):

  squared   VH = sum g^2 V' / W^2     what the library computes: the taps taken
                                      as independent (mm_denoise_frames_var's form)
  linear    VH = sum g V' / W         the SVGF-style moment interpolation

with Vout = (1 - 1/N)^2 VH + (1/N)^2 Vc in both.  Printed: estimate / actual
after `--frames` frames for the shifts (a, a) from (0, 0) to (0.5, 0.5)
(8 frames, n_max 32: squared 0.78 .. 1.00, linear 1.00 .. 4.66), or with
--grid for every (a, b) of the grid (a shift along one axis only is the
squared form's worst case: 0.63 at (0.5, 0)).
The squared form is exact at shift 0 and falls short once neighbouring history
pixels share ancestors (it ignores their covariance); the linear form ignores
the averaging a resample does and overshoots.  A model of iid noise, not a
measurement on rendered frames: profiles/temporal_var/quality.txt has that."""
from __future__ import annotations

import argparse
import sys

import numpy as np

SHIFTS = (0.0, 0.125, 0.25, 0.375, 0.5)


def run(a: float, b: float, frames: int = 8, n_max: int = 32):
    """(actual, squared estimate, linear estimate) of the accumulated pixel's
    variance after `frames` frames of unit-variance noise at shift (a, b)."""
    g = np.array([[(1 - a) * (1 - b), a * (1 - b)], [(1 - a) * b, a * b]])  # taps (dy, dx)
    size = frames + 2
    # coef[k]: the accumulated pixel's coefficients on frame k's noise image (around the pixel)
    coef = [np.zeros((size, size)) for _ in range(frames)]
    coef[0][0, 0] = 1.0
    n_hist, v_sq, v_lin = 1.0, 1.0, 1.0
    for f in range(1, frames):
        n = min(n_hist + 1.0, float(n_max))
        bw = 1.0 / n
        cw = 1.0 - bw
        for k in range(f):
            c = coef[k]
            r = np.zeros_like(c)
            for dy in range(2):
                for dx in range(2):
                    r[dy:, dx:] += g[dy, dx] * c[:size - dy, :size - dx]
            coef[k] = cw * r
        coef[f][0, 0] = bw
        v_sq = cw * cw * (g * g).sum() * v_sq + bw * bw
        v_lin = cw * cw * v_lin + bw * bw
        n_hist = n
    actual = float(sum((c * c).sum() for c in coef))
    return actual, float(v_sq), float(v_lin)


def table(frames: int = 8, n_max: int = 32, grid: bool = False):
    """[(a, b, actual, squared / actual, linear / actual)] over the shifts (a, a)
    from (0, 0) to (0.5, 0.5), or with `grid` over every (a, b) of SHIFTS."""
    rows = []
    for a in SHIFTS:
        for b in (SHIFTS if grid else (a,)):
            act, sq, lin = run(a, b, frames, n_max)
            rows.append((a, b, act, sq / act, lin / act))
    return rows


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--n-max", type=int, default=32)
    ap.add_argument("--grid", action="store_true", help="every (a, b) of the grid, not only the diagonal a = b")
    args = ap.parse_args(argv)
    rows = table(args.frames, args.n_max, args.grid)
    print(f"{args.frames} frames, n_max {args.n_max}: estimate / actual variance of the accumulated pixel")
    print("  shift a     b   actual   squared   linear")
    for a, b, act, sq, lin in rows:
        print(f"     {a:5.3f} {b:5.3f}  {act:7.4f}   {sq:7.3f}  {lin:7.3f}")
    sq = [r[3] for r in rows]
    lin = [r[4] for r in rows]
    print(f"squared form: {min(sq):.2f} .. {max(sq):.2f}   linear form: {min(lin):.2f} .. {max(lin):.2f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
