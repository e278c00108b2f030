#!/usr/bin/env python
"""Timing of mm_denoise_frames_var against mm_denoise_frames on one GPU, C3-sized
(32x32 maze, 1920x1080, the frame, its sample variance and its guides at 8 spp,
8/8 bounces), the two interleaved in one process:

  * n_passes 1..5, float output, one frame per call; per n_passes the sequence
    denoise, denoise_var, denoise, denoise_var, each timed on its own;
  * per case: ms per frame and per pass, the algorithmic bandwidth of the bytes
    per pixel-pass model -- denoise 56 B (16 B colour in, 16 B out, 24 B of
    guides), denoise_var 64 B (+ 4 B variance in, + 4 B out) -- and its fraction
    of the HBM peak.

    python scripts/denoise_var_bench.py [--warmup 2] [--steps 5]

Each figure is HIP-event time on the stream over one call, after --warmup calls
of the same case; the median of --steps calls is printed with their min and
max, none dropped.  var / count is formed once, outside the timed calls
(Renderer.denoise_var forms it in torch per call: bookkeeping, timed on its own
line).  A different build of the library: MIRROR_MAZE_LIB=/path/lib.so.
"""
from __future__ import annotations

import argparse
import ctypes as C
import inspect
import statistics
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "mirror-maze_amd"))
sys.path.insert(0, str(REPO))

MODEL_BYTES = {"denoise": 56, "denoise_var": 64}
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
    ap.add_argument("--max-passes", type=int, default=5)
    a = ap.parse_args(argv)

    import torch

    from mirror_maze import Renderer, Scene, _lib, default_uniform, make_ext

    W, H = 1920, 1080
    scene = Scene.build(a.maze, 0)
    u = default_uniform(W, H, 0)
    with Renderer(0) as r:
        r.upload_scene(scene)
        color, var, _ = r.trace_tile_var(u, make_ext(8, 8, 8, frame=0), 0, 0, W, H)
        aov = r.trace_aov(u, None, 8, x0=0, y0=0, w=W, h=H)
        vmean = (var / 8.0).contiguous()
        out, vout = torch.empty_like(color), torch.empty_like(var)
        r.sync()
        guides = _lib.mm_aov(*[aov[k].data_ptr() for k in Renderer.AOV_NAMES])
        L = _lib.lib()
        r._follow(color.device)

        sig = inspect.signature(Renderer.denoise_var).parameters  # the sigmas are denoise_var's defaults
        sz, sl, eps = (float(sig[k].default) for k in ("sigma_z", "sigma_l", "eps_l"))

        def run_var(n_passes, with_var_out=True):
            p = _lib.mm_denoise_var_params(n_passes, sz, sl, eps, 0, 0)
            r._check(L.mm_denoise_frames_var(r._ctx, color.data_ptr(), C.byref(guides), vmean.data_ptr(), C.byref(p),
                                             1, W, H, out.data_ptr(), vout.data_ptr() if with_var_out else None))

        print(f"# {W}x{H}, maze {a.maze}, one frame, 8 spp; warmup {a.warmup}, steps {a.steps}; model "
              f"{MODEL_BYTES['denoise']} / {MODEL_BYTES['denoise_var']} B per pixel-pass, HBM peak {HBM_PEAK_GBS:.0f} GB/s; "
              f"denoise 0.02 / 0.5, denoise_var {sz:g} / {sl:g} / {eps:g}")
        for n_passes in range(1, a.max_passes + 1):
            cases = {"denoise": lambda: r.denoise(color, aov, n_passes=n_passes, out=out),
                     "denoise_var": lambda: run_var(n_passes)}
            for what in ("denoise", "denoise_var", "denoise", "denoise_var"):
                ms = timed(cases[what], a.warmup, a.steps)
                med = statistics.median(ms)
                gbs = MODEL_BYTES[what] * W * H * n_passes / (med * 1e-3) / 1e9
                print(f"{what:11s}  passes {n_passes}: {med:.4f} ms/frame (min {min(ms):.4f} max {max(ms):.4f}), "
                      f"{med / n_passes:.4f} ms/pass, {gbs:7.1f} GB/s = {gbs / HBM_PEAK_GBS:.3f} of peak", flush=True)
        ms = timed(lambda: run_var(a.max_passes, with_var_out=False), a.warmup, a.steps)
        print(f"denoise_var  passes {a.max_passes}, no variance output: {statistics.median(ms):.4f} ms/frame "
              f"(min {min(ms):.4f} max {max(ms):.4f})")
        ms = timed(lambda: r.denoise_var(color, aov, var, 8.0, n_passes=a.max_passes, out=out, var_out=vout),
                   a.warmup, a.steps)
        print(f"Renderer.denoise_var (var / count in torch per call)  passes {a.max_passes}: "
              f"{statistics.median(ms):.4f} ms/frame (min {min(ms):.4f} max {max(ms):.4f})")
    return 0


if __name__ == "__main__":
    sys.exit(main())
