#!/usr/bin/env python
"""What the variance calls cost on one GPU, C3-sized (32x32 maze, 1920x1080,
8/8 bounces, the default camera), at 8 spp (the samples stay in registers
between the resolve's two passes) and at 16 spp (the second pass reads them
again), against a checkout of the PARENT commit built beside this one:

  (i)   one frame: trace_tile_var against the parent's mm_trace_tile with
        MM_OPT_FUSE_RESOLVE 0 (the same staging, the plain resolve), and
        against the parent's default, the fused resolve;
  (ii)  20 frames in one launch (10 at 16 spp; tail deferral on, the samples
        staged anyway): trace_tile_var(n_frames=20) against the parent's
        mm_trace_tile_frames;
  (iii) the resolve alone, k_resolve8_var against k_resolve8: the one-frame
        call's HIP-event time less its trace kernel's (mm_kernel_timing), with
        the fraction of the 8 TB/s HBM peak on a model of 12 B per path + 20 B
        per pixel (the plain resolve: + 16 B per pixel).

    python scripts/variance_bench.py --parent-tree /path/to/parent/checkout [--rounds 3] [--warmup 3] [--steps 9]

Each build runs in a process of its own (one library per process), parent and
new alternating, --rounds times; a figure is the median of a leg's --steps
HIP-event times after --warmup calls, and the table gives the median of the
legs' figures with their lowest and highest.  The new build's own plain calls
are printed too, as a control -- never as the baseline.  The result goes to
--out (default profiles/variance/ab.txt) and to stdout.
"""
from __future__ import annotations

import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
W, H = 1920, 1080
FRAMES = {8: 20, 16: 10}  # 16 spp: 20 frames' staged samples would exceed the 2^29 paths of one launch
SPPS = (8, 16)
HBM_PEAK = 8.0e12


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


def leg(tree: Path, new: bool, maze: int, warmup: int, steps: int) -> dict:
    """The figures of one build (its package and library under `tree`), in ms."""
    sys.path.insert(0, str(tree / "mirror-maze_amd"))
    sys.path.insert(0, str(tree))
    import torch

    from mirror_maze import Renderer, Scene, default_uniform, make_ext
    from mirror_maze._lib import MM_OPT_FUSE_RESOLVE

    med = statistics.median
    scene = Scene.build(maze, 0)
    u = default_uniform(W, H, 0)
    dev = torch.device("cuda:0")
    res = {}
    one = torch.empty((H, W, 4), dtype=torch.float32, device=dev)
    var1 = torch.empty((H, W), dtype=torch.float32, device=dev)

    def resolve_alone(r, fn):
        """The call's event time less its trace kernel's, per call."""
        r.set_profiling(True)
        for _ in range(warmup):
            fn()
        r.sync()
        r.kernel_timing(reset=True)
        rest = []
        for _ in range(steps):
            t = timed(fn, 0, 1)[0]
            k, n = r.kernel_timing(reset=True)
            assert n == 1
            rest.append(t - k)
        r.set_profiling(False)
        return med(rest)

    for spp in SPPS:
        e = make_ext(spp, 8, 8, frame=0)
        n = FRAMES[spp]
        many = torch.empty((n, H, W, 4), dtype=torch.float32, device=dev)
        varn = torch.empty((n, H, W), dtype=torch.float32, device=dev)
        with Renderer(0) as r:
            r.upload_scene(scene)
            res[f"fused_1@{spp}"] = med(timed(lambda: r.trace_tile(u, e, 0, 0, W, H, out=one), warmup, steps))
            res[f"plain_n@{spp}"] = med(timed(lambda: r.trace_tile_frames(u, e, n, 0, 0, W, H, out=many),
                                              warmup, steps)) / n
            if new:
                res[f"var_1@{spp}"] = med(timed(lambda: r.trace_tile_var(u, e, 0, 0, W, H, out=one, var=var1),
                                                warmup, steps))
                res[f"var_n@{spp}"] = med(timed(
                    lambda: r.trace_tile_var(u, e, 0, 0, W, H, n_frames=n, out=many, var=varn), warmup, steps)) / n
                res[f"var_resolve@{spp}"] = resolve_alone(r, lambda: r.trace_tile_var(u, e, 0, 0, W, H, out=one, var=var1))
                plain, _ = r.trace_tile(u, e, 0, 0, W, H)
                res[f"same_bits@{spp}"] = bool(torch.equal(plain.view(torch.int32), one.view(torch.int32)))
        with Renderer(0) as r:
            r.set_option(MM_OPT_FUSE_RESOLVE, 0)
            r.upload_scene(scene)
            res[f"staged_1@{spp}"] = med(timed(lambda: r.trace_tile(u, e, 0, 0, W, H, out=one), warmup, steps))
            res[f"plain_resolve@{spp}"] = resolve_alone(r, lambda: r.trace_tile(u, e, 0, 0, W, H, out=one))
    return res


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-tree", type=Path, help="a built checkout of the parent commit")
    ap.add_argument("--maze", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=9)
    ap.add_argument("--out", type=Path, default=REPO / "profiles" / "variance" / "ab.txt")
    ap.add_argument("--leg", choices=("parent", "new"), help=argparse.SUPPRESS)
    ap.add_argument("--tree", type=Path, help=argparse.SUPPRESS)
    a = ap.parse_args(argv)
    if a.leg:
        print(json.dumps(leg(a.tree, a.leg == "new", a.maze, a.warmup, a.steps)))
        return 0
    if not a.parent_tree or not (a.parent_tree / "mirror-maze_amd" / "lib" / "libmirror_maze.so").exists():
        ap.error("--parent-tree must be a checkout of the parent commit with its library built")

    legs = {"parent": [], "new": []}
    for _ in range(a.rounds):
        for name, tree in (("parent", a.parent_tree), ("new", REPO)):
            p = subprocess.run([sys.executable, __file__, "--leg", name, "--tree", str(tree), "--maze", str(a.maze),
                                "--warmup", str(a.warmup), "--steps", str(a.steps)], capture_output=True, text=True,
                               timeout=900)
            if p.returncode != 0:
                sys.stderr.write(p.stdout + p.stderr)
                return 1
            legs[name].append(json.loads(p.stdout.strip().splitlines()[-1]))

    def fig(name, key):
        v = [x[key] for x in legs[name]]
        return statistics.median(v), min(v), max(v)

    def row(label, name, key, base=None):
        m, lo, hi = fig(name, key)
        s = f"  {label:<58} {m:8.4f} ms  (legs {lo:.4f} .. {hi:.4f})"
        if base is not None:
            s += f"  {m / base:6.3f} x"
        return s

    lines = [f"# variance_bench: {W}x{H}, maze {a.maze}, 8/8 bounces; {a.rounds} legs per build, alternating, each the "
             f"median of {a.steps} HIP-event times after {a.warmup} warm-up calls; ms per frame"]
    for spp in SPPS:
        paths, pix = W * H * spp, W * H
        staged, _, _ = fig("parent", f"staged_1@{spp}")
        fused, _, _ = fig("parent", f"fused_1@{spp}")
        multi, _, _ = fig("parent", f"plain_n@{spp}")
        lines += [f"== {spp} spp ==",
                  " (i) one frame",
                  row("parent mm_trace_tile, MM_OPT_FUSE_RESOLVE 0", "parent", f"staged_1@{spp}"),
                  row("parent mm_trace_tile, default (fused resolve)", "parent", f"fused_1@{spp}"),
                  row("new    mm_trace_tile_var, against the staged parent", "new", f"var_1@{spp}", staged),
                  row("new    mm_trace_tile_var, against the fused parent", "new", f"var_1@{spp}", fused),
                  row("new    mm_trace_tile, MM_OPT_FUSE_RESOLVE 0 (control)", "new", f"staged_1@{spp}", staged),
                  row("new    mm_trace_tile, default (control)", "new", f"fused_1@{spp}", fused),
                  f" (ii) {FRAMES[spp]} frames in one launch",
                  row("parent mm_trace_tile_frames", "parent", f"plain_n@{spp}"),
                  row("new    mm_trace_tile_var", "new", f"var_n@{spp}", multi),
                  row("new    mm_trace_tile_frames (control)", "new", f"plain_n@{spp}", multi),
                  " (iii) the resolve alone (the one-frame call less its trace kernel)"]
        pr, _, _ = fig("parent", f"plain_resolve@{spp}")
        vr, _, _ = fig("new", f"var_resolve@{spp}")
        lines += [row("parent k_resolve8", "parent", f"plain_resolve@{spp}") +
                  f"  {(12 * paths + 16 * pix) / (pr * 1e-3) / HBM_PEAK:.2f} of HBM peak (12 B/path + 16 B/pixel)",
                  row("new    k_resolve8_var", "new", f"var_resolve@{spp}", pr) +
                  f"  {(12 * paths + 20 * pix) / (vr * 1e-3) / HBM_PEAK:.2f} of HBM peak (12 B/path + 20 B/pixel)",
                  f"  out of mm_trace_tile_var == mm_trace_tile on all bits: "
                  f"{all(x[f'same_bits@{spp}'] for x in legs['new'])}"]
    text = "\n".join(lines) + "\n"
    a.out.parent.mkdir(parents=True, exist_ok=True)
    a.out.write_text(text)
    sys.stdout.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
