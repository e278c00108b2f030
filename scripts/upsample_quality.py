#!/usr/bin/env python
"""What tracing a lattice and rebuilding from the AOVs (Renderer.trace_upsampled)
costs in quality, on the maze N=4 at 160x120, the mirror corridor
(tests/golden/aov_corridor.npz) at 140x48 and the maze N=32 at 640x360; 8-frame
slow walks (0.013, 0.021 per frame in x, z) at 8 spp, 8/8 bounces, 8 mirrors,
scales 2 and 4, w_min 0.25.  Every MSE is over rgb against a 512-spp frame of
the last camera drawn with another RNG frame, as a fraction of the raw full
8-spp last frame's; beside every figure of the rebuilt frames stands the same
figure of the frames traced in full:

  (a) the last frame, upsampled and its holes filled;
  (b) that through denoise (defaults), against the denoised full frame;
  (c) the walk through accumulate_var -> denoise_var (sigma_l 2, count 1) --
      the rebuilt frames enter with their weight and variance -- against the
      same chain over the full frames;

and per scale the share of holes and the rays traced (lattice + holes) as a
share of the full frame's.

    python scripts/upsample_quality.py [--out profiles/upsample/quality.txt]

Nothing here is a threshold; the figures are written down as measured, where the
rebuilt frames lose as plainly as where they win.
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "mirror-maze_amd"))
sys.path.insert(0, str(REPO))

SPP, SCALES, W_MIN, SIGMA_L = 8, (2, 4), 0.25, 2.0


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", type=Path, default=REPO / "profiles" / "upsample" / "quality.txt")
    a = ap.parse_args(argv)

    import ctypes as C

    import numpy as np

    from mirror_maze import Renderer, Scene, default_uniform, make_ext, mm_camera, mm_uniform
    from mirror_maze._lib import MM_OPT_DEFER_MIN

    z = np.load(REPO / "tests" / "golden" / "aov_corridor.npz")
    corridor = Scene(0, z["rects"], np.ascontiguousarray(z["nodes"]), z["idx"], z["is_mirror"], z["emission"],
                     np.zeros((0, 0), np.uint8), 0)
    uc = mm_uniform()
    C.memmove(C.byref(uc), np.ascontiguousarray(z["camera"], dtype=np.float32).ctypes.data, 40)
    uc.view_w, uc.view_h, uc.chunk_w, uc.time = 140.0, 48.0, 4, 0
    cases = [("maze 4, 160x120", Scene.build(4, 0), default_uniform(160, 120, 0), 160, 120),
             ("mirror corridor, 140x48", corridor, uc, 140, 48),
             ("maze 32, 640x360", Scene.build(32, 0), default_uniform(640, 360, 0), 640, 360)]
    lines = [f"# upsample_quality: 8-frame walks at {SPP} spp, 8/8 bounces, 8 mirrors; trace_upsampled with w_min {W_MIN}, "
             f"holes filled at {SPP} spp; MSE over rgb against a 512-spp frame of the last camera (RNG frame 777), as a "
             f"fraction of the raw full last frame's; 'full' is the same stage over the frames traced at every pixel"]

    for name, scene, u, w, h in cases:
        with Renderer(0) as r:
            r.set_option(MM_OPT_DEFER_MIN, 0)  # a multi-frame variance launch of any size
            r.upload_scene(scene)
            n = 8
            cams = np.tile(np.frombuffer(bytes(u.cam), dtype=np.float32), (n, 1)).copy()
            cams[:, 0] += np.float32(0.013) * np.arange(n, dtype=np.float32)
            cams[:, 2] += np.float32(0.021) * np.arange(n, dtype=np.float32)
            e = make_ext(SPP, 8, 8, frame=0)
            full, fvar, _ = r.trace_tile_var(u, e, 0, 0, w, h, cameras=cams)
            aov = r.trace_aov(u, cams, 8, x0=0, y0=0, w=w, h=h)
            ul = mm_uniform.from_buffer_copy(u)
            ul.cam = mm_camera.from_buffer_copy(np.ascontiguousarray(cams[-1], dtype=np.float32).tobytes())
            truth, _ = r.trace_tile(ul, make_ext(512, 8, 8, frame=777), 0, 0, w, h)
            t = truth.double()
            last = {k: v[-1:] for k, v in aov.items()}

            def mse(img):
                return float(((img.double().reshape(h, w, 4)[..., :3] - t[..., :3]) ** 2).mean())

            raw = mse(full[-1])
            f_dn = mse(r.denoise(full[-1], last)) / raw
            f_acc, f_vout = r.accumulate_var(u, cams, full, aov, (fvar / float(SPP)).contiguous())
            f_accm = mse(f_acc[-1]) / raw
            f_chain = mse(r.denoise_var(f_acc[-1], last, f_vout[-1], 1.0, sigma_l=SIGMA_L)) / raw
            lines.append(f"== {name}: {n} frames, {w * h} pixels, raw full last frame MSE {raw:.6g} ==")
            lines.append(f"  full frames: raw 1.0000; (b) denoise {f_dn:.4f}; (c) accumulate_var {f_accm:.4f} -> denoise_var "
                         f"{f_chain:.4f}")
            for s in SCALES:
                up, _, wt, vo, share = r.trace_upsampled(u, cams, e, s, 0, 0, w, h, mirror_limit=8, w_min=W_MIN, var=True)
                lat = (-(-w // s)) * (-(-h // s)) / float(w * h)
                holes = float(np.mean(share))
                u_acc, u_vout = r.accumulate_var(u, cams, up, aov, vo, wt)
                lines.append(f"  scale {s}: holes {100.0 * holes:.2f} % of the pixels (last frame {100.0 * share[-1]:.2f} %), "
                             f"rays traced {lat + holes:.3f} of the full frame's (lattice {lat:.4f})")
                lines.append(f"    (a) upsampled + filled {mse(up[-1]) / raw:.4f}  (full 1.0000)")
                lines.append(f"    (b) -> denoise {mse(r.denoise(up[-1], last)) / raw:.4f}  (full {f_dn:.4f})")
                lines.append(f"    (c) accumulate_var {mse(u_acc[-1]) / raw:.4f} -> denoise_var "
                             f"{mse(r.denoise_var(u_acc[-1], last, u_vout[-1], 1.0, sigma_l=SIGMA_L)) / raw:.4f}  "
                             f"(full {f_accm:.4f} -> {f_chain:.4f})")
            r.sync()
    text = "\n".join(lines) + "\n"
    a.out.parent.mkdir(parents=True, exist_ok=True)
    a.out.write_text(text)
    sys.stdout.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
