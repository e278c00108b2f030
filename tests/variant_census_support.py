"""The census of the wave-persistent trace kernel's built variants, shared by tests/test_variant_census.py
(CPU: the launch policy plans each case's variant, the table is complete, its inputs keep paths alive) and
tests/test_gpu_variant_census.py (GPU: each case runs the variant it names, bit for bit against the oracle).

A variant is a cell (LDS mode, internal form, tail-ring kind): MM_INFO_LAST_LDS_MODE,
MM_INFO_LAST_KERNEL_FORM and MM_INFO_LAST_RING after a launch, mm_variant_built for what the build holds
(mirror-maze_amd/csrc/mm_variants.h).  Which cell a call runs follows from the uploaded scene's grid image and
the options (mm_plan.cpp), so a case is a scene, options and an entry point, and the table below is found with
the CPU plan harness (tests/launch_plan/launch_plan_test.cpp) alone:

  mazes (Scene.build(N, 0); the grid image grows with N)
    N <= 44   wide words, the whole image in LDS (11, 17): ring 2 to N = 32 (image <= grid_lds_cap<2>),
              ring 1 at N = 36 / 40, no ring at N = 44 (image > grid_lds_cap<1>: a forced deferral is dropped)
    N 48..64  plain words, records + index in LDS (14, 15): ring 2 at N = 48 (off_box 45152), ring 1 from N = 56
    N 72..96  plain words, index only (12, 15): ring 2 at N = 72 (off_data 39216), ring 1 at N = 80 / 96
    N >= 112  no longer flat (coarser cells): the general form (12, 11)
    MM_OPT_GRID_WIDE 0 gives the plain maze form (.., 15) at small N, MM_OPT_LDS_NODES 0 placement 13
  soups (test_gpu_random_scene.random_scene; MM_OPT_GRID_CELL coarsens the cells until the wide image fits)
    fine (seed 7: SLOW records, forms 12 / 14) and lattice (seed 11: forms 11 / 13), n = 200 at cell scales
    100 .. 400 for every band of placement 11, n = 1200 at scale 200 for placement 12 with a small index

The ring kind of a dynamic-LDS placement (12, 13, 3) depends on the kernels' static LDS, which the harness is
given as STATIC_LDS: the static words of grid_lds_cap (mm_variants.h) less the grid array's alignment slack,
2192 B with ring kind 1 and 34960 B with kind 2 (profiles/bounce_trim/kernel_resources_branch.txt).  The GPU
test asserts MM_INFO_LAST_STATIC_LDS against the same figures."""
from __future__ import annotations

import ctypes as C
import functools
import json
import subprocess
from collections import namedtuple
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
REPO = HERE.parent
CSRC = REPO / "mirror-maze_amd" / "csrc"
HARNESS_SRC = [HERE / "launch_plan" / "launch_plan_test.cpp",
               *(CSRC / f for f in ("scene.cpp", "rect_compact.cpp", "grid_build.cpp", "mm_plan.cpp"))]
HARNESS_BUILDS = {"plain": ["-O2"],
                  "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}

MM_OPT_LDS_NODES, MM_OPT_TRAVERSAL, MM_OPT_LDS_RECTS, MM_OPT_DEFER, MM_OPT_DEFER_MIN = 1, 7, 8, 21, 22
MM_OPT_GRID_CELL, MM_OPT_GRID_WIDE = 25, 26
# option key -> the plan harness's argument
HARNESS_ARG = {MM_OPT_LDS_NODES: "lds", MM_OPT_TRAVERSAL: "ww", MM_OPT_LDS_RECTS: "lds_rects", MM_OPT_DEFER: "defer",
               MM_OPT_DEFER_MIN: "defer_min", MM_OPT_GRID_CELL: "grid_cell", MM_OPT_GRID_WIDE: "grid_wide"}
RINGS = {MM_OPT_DEFER: 32, MM_OPT_DEFER_MIN: 0}  # tail deferral forced on, at any launch size

MODES = (0, 1, 3, 11, 12, 13, 14)
FORMS = (5, 7, 11, 12, 13, 14, 15, 16, 17, 18)
RING_KINDS = (0, 1, 2)
STATIC_GRID_MODES = (11, 14)
LDS_PER_BLOCK = 80 * 1024
GRID_CAP = {0: 81728, 1: 79664, 2: 46896}    # grid_lds_cap<kRing>, mm_variants.h
STATIC_LDS = {1: LDS_PER_BLOCK - GRID_CAP[1] - 64, 2: LDS_PER_BLOCK - GRID_CAP[2] - 64}
assert STATIC_LDS == {1: 2192, 2: 34960}

VIEW = (640, 480)
ORIGIN = (288, 224)            # the horizon down the corridors (tests/test_gpu_predraw.py)
SPP, BOUNCES, MIRRORS = 8, 8, 8
FRAME0 = 1                     # RNG frame of a case's first frame
N_FRAMES = 2
ENTRIES = ("tile", "frames", "cameras", "pixels", "pixel_lists")
MIN_RAYS_PER_PATH = 3.0        # of a ringed case's window, by the oracle

MAZE_LADDER = (4, 10, 16, 24, 32, 36, 40, 44, 48, 56, 64, 72, 80, 96, 112, 128, 160, 200)
GPU_MAZE_MAX = 128

# ---- scenes ---------------------------------------------------------------------
# ("maze", N) or ("soup", n, seed, lattice)
FINE, LATTICE = ("soup", 200, 7, False), ("soup", 200, 11, True)
FINE_BIG, LATTICE_BIG = ("soup", 1200, 7, False), ("soup", 1200, 11, True)
SOUPS = (FINE, LATTICE, FINE_BIG, LATTICE_BIG)


def maze(n):
    return ("maze", n)


def scene_id(key):
    return f"maze{key[1]}" if key[0] == "maze" else f"{'lattice' if key[3] else 'fine'}{key[1]}"


@functools.lru_cache(maxsize=None)
def scene(key):
    """The Scene of a key, built once."""
    from mirror_maze import Scene

    if key[0] == "maze":
        return Scene.build(key[1], 0)
    from test_gpu_random_scene import random_scene

    return random_scene(*key[1:])


@functools.lru_cache(maxsize=None)
def oracle(key):
    from oracle.oracle import Oracle

    return Oracle.from_scene(scene(key))


# Soup cameras (centre, view direction).  A path that leaves a sparse soup ends on its first miss, so the
# default camera's window traces one ray per path.  Each camera here stands 4 in front of a mirror rect and
# looks at it so that the reflection meets a near rect: two hits are certain and the paths live on from there
# (found with the oracle alone; test_variant_census.py test_ringed_windows_keep_paths_alive holds them to it).
SOUP_CAMERAS = {
    FINE: (((-122.375, -46.140625, -158.8125), (-0.724609375, -0.4013671875, -0.5595703125)),
           ((-125.75, -45.96875, -164.59375), (0.1162109375, -0.4443359375, 0.888671875))),
    LATTICE: (((12.921875, -103.359375, 110.03125), (-0.23046875, 0.8388671875, 0.4931640625)),
              ((12.8125, -102.421875, 108.921875), (-0.2021484375, 0.6064453125, 0.7685546875))),
    FINE_BIG: (((-40.765625, 32.3125, -122.203125), (-0.7197265625, 0.1171875, 0.68359375)),
               ((-42.59375, 29.71875, -121.828125), (-0.259765625, 0.7646484375, 0.5888671875))),
    LATTICE_BIG: (((-99.515625, 2.328125, 20.40625), (-0.1201171875, 0.419921875, 0.8994140625)),
                  ((-142.671875, -34.671875, -106.671875), (-0.3330078125, 0.6669921875, 0.6669921875))),
}


@functools.lru_cache(maxsize=None)
def cameras(key):
    """The (2, 10) camera rows of a scene's cases (read-only).  Mazes: camera 0 is the default camera at the
    spawn, its window on the horizon down the corridors; camera 1 stands in the maze's middle cell looking
    along a corridor and a little sideways, as test_gpu_frames.py test_cameras_inside_the_maze puts one.
    Soups: SOUP_CAMERAS."""
    from mirror_maze import calculate_quaternion, default_uniform

    u = default_uniform(*VIEW, 0)
    rows = np.zeros((N_FRAMES, 10), np.float32)
    for f in range(N_FRAMES):
        rows[f] = [*u.cam.center, u.cam.focal, *u.cam.quat, *u.cam.viewport]
    if key[0] == "maze":
        n = key[1]
        base = -10.0 * (n / 2)
        rows[1, 0:3] = (base + 10.0 * (n // 2) + 5.0, 0.0, base + 10.0 * (n // 2) + 5.0)
        rows[1, 4:8] = calculate_quaternion(np.float32([1.0, 0.05, 0.3]))
    else:
        for f, (centre, direction) in enumerate(SOUP_CAMERAS[key]):
            rows[f, 0:3] = centre
            rows[f, 4:8] = calculate_quaternion(np.float32(direction))
    rows.setflags(write=False)
    return rows


def uniform(key, cam):
    """default_uniform of the view with camera `cam` of the scene."""
    from mirror_maze import default_uniform

    u = default_uniform(*VIEW, 0)
    row = cameras(key)[cam]
    for i in range(3):
        u.cam.center[i] = float(row[i])
    u.cam.focal = float(row[3])
    for i in range(4):
        u.cam.quat[i] = float(row[4 + i])
    for i in range(2):
        u.cam.viewport[i] = float(row[8 + i])
    return u


def ext(frame=FRAME0):
    from mirror_maze import make_ext

    return make_ext(SPP, BOUNCES, MIRRORS, frame=frame)


@functools.lru_cache(maxsize=None)
def reference(key, cam, frame, x0, y0, w, h):
    """(pixels (h, w, 4), rays, paths) of the oracle for a window, camera and RNG frame; computed once, shared
    and read-only."""
    out, st = oracle(key).trace_tile(uniform(key, cam), ext(frame), x0, y0, w, h)
    out.setflags(write=False)
    return out, int(st.rays), int(st.paths)


# ---- cases ----------------------------------------------------------------------
Case = namedtuple("Case", "scene opts entry stats expect")


def case_id(c):
    opts = ",".join(f"{k}={v}" for k, v in sorted(c.opts.items())) or "auto"
    return f"{scene_id(c.scene)}-{opts}-{c.entry}{'-stats' if c.stats else ''}-" + "m{}f{}r{}".format(*c.expect)


def forced(c):
    """Whether the case forces tail deferral on (the larger window: several waves park per block)."""
    return c.opts.get(MM_OPT_DEFER, 0) > 0


def window(c):
    """(x0, y0, w, h): 32 x 16 as the parity tests trace it; 64 x 32 (256 chunks) where rings are asked for."""
    return (*ORIGIN, 64, 32) if forced(c) else (*ORIGIN, 32, 16)


def frames_of(c):
    """[(camera, RNG frame)] of the case's frames, in the order of its output."""
    if c.entry in ("tile", "pixels"):
        return [(0, FRAME0)]
    if c.entry == "frames":
        return [(0, FRAME0 + f) for f in range(N_FRAMES)]
    return [(f, FRAME0 + f) for f in range(N_FRAMES)]  # cameras, pixel_lists


def pixel_list(c, seed=0):
    """The case's window as a pixel list: every pixel once in shuffled order, then one of them again and one
    entry outside the view.  Returns (pixels (n, 2) int32, index of the duplicated pixel in the list)."""
    x0, y0, w, h = window(c)
    rng = np.random.default_rng(1000 + seed)
    xy = np.stack(np.meshgrid(np.arange(x0, x0 + w), np.arange(y0, y0 + h)), axis=-1).reshape(-1, 2)
    xy = xy[rng.permutation(len(xy))]
    dup = int(rng.integers(len(xy)))
    return np.ascontiguousarray(np.concatenate([xy, xy[dup:dup + 1], [[VIEW[0], y0]]]).astype(np.int32)), dup


# The (scene, options) that run each built (LDS mode, form) pair without rings ...
PAIR_SITES = {
    (11, 17): (maze(32), {}),
    (11, 15): (maze(32), {MM_OPT_GRID_WIDE: 0}),
    (14, 15): (maze(48), {}),
    (12, 15): (maze(72), {}),
    (13, 17): (maze(32), {MM_OPT_LDS_NODES: 0}),
    (13, 15): (maze(32), {MM_OPT_LDS_NODES: 0, MM_OPT_GRID_WIDE: 0}),
    (12, 11): (maze(128), {}),
    (11, 11): (LATTICE, {MM_OPT_GRID_CELL: 300, MM_OPT_GRID_WIDE: 0}),
    (13, 11): (LATTICE, {MM_OPT_GRID_CELL: 300, MM_OPT_GRID_WIDE: 0, MM_OPT_LDS_NODES: 0}),
    (11, 13): (LATTICE, {MM_OPT_GRID_CELL: 300}),
    (13, 13): (LATTICE, {MM_OPT_GRID_CELL: 300, MM_OPT_LDS_NODES: 0}),
    (11, 12): (FINE, {MM_OPT_GRID_CELL: 200, MM_OPT_GRID_WIDE: 0}),
    (12, 12): (FINE, {}),
    (13, 12): (FINE, {MM_OPT_GRID_CELL: 200, MM_OPT_GRID_WIDE: 0, MM_OPT_LDS_NODES: 0}),
    (11, 14): (FINE, {MM_OPT_GRID_CELL: 200}),
    (13, 14): (FINE, {MM_OPT_GRID_CELL: 200, MM_OPT_LDS_NODES: 0}),
    (3, 7): (maze(24), {MM_OPT_TRAVERSAL: 7}),
    (3, 5): (maze(24), {MM_OPT_TRAVERSAL: 5}),
    (1, 5): (maze(24), {MM_OPT_TRAVERSAL: 5, MM_OPT_LDS_RECTS: 0}),
    (0, 5): (maze(24), {MM_OPT_TRAVERSAL: 5, MM_OPT_LDS_NODES: 0}),
}
# ... and, with RINGS, each ringed cell: (mode, form, ring) -> [(scene, options, entry)].  The staged bytes
# that decide the ring kind are in the comments (static grid: against GRID_CAP; dynamic: + STATIC_LDS <= 80 KB).
RING_SITES = {
    (11, 17, 2): [(maze(32), {}, "cameras")],                                      # 45120
    (11, 17, 1): [(maze(36), {}, "cameras"), (maze(40), {}, "frames")],            # 55200, 67824
    (11, 15, 2): [(maze(32), {MM_OPT_GRID_WIDE: 0}, "cameras")],                   # 39216
    (11, 15, 1): [(maze(40), {MM_OPT_GRID_WIDE: 0}, "cameras")],                   # 58784
    (14, 15, 2): [(maze(48), {}, "cameras")],                                      # 45152
    (14, 15, 1): [(maze(56), {}, "cameras")],                                      # 59424
    (12, 15, 2): [(maze(72), {}, "cameras")],                                      # 39216 + 34960
    (12, 15, 1): [(maze(96), {}, "cameras"), (maze(80), {}, "frames")],            # 68960, 48176 (+ 34960 > 80 KB)
    (13, 17, 2): [(maze(32), {MM_OPT_LDS_NODES: 0}, "cameras")],                   # 0
    (13, 15, 2): [(maze(32), {MM_OPT_LDS_NODES: 0, MM_OPT_GRID_WIDE: 0}, "cameras")],
    (12, 11, 2): [(LATTICE_BIG, {MM_OPT_GRID_CELL: 200}, "cameras")],              # 21344 + 34960
    (12, 11, 1): [(maze(128), {}, "cameras")],                                     # 73568
    (11, 11, 2): [(LATTICE, {MM_OPT_GRID_CELL: 300, MM_OPT_GRID_WIDE: 0}, "cameras")],   # 39104
    (11, 11, 1): [(LATTICE, {}, "cameras")],                                       # 61456
    (13, 11, 2): [(LATTICE, {MM_OPT_GRID_CELL: 300, MM_OPT_GRID_WIDE: 0, MM_OPT_LDS_NODES: 0}, "cameras")],
    (11, 13, 2): [(LATTICE, {MM_OPT_GRID_CELL: 400}, "cameras")],                  # 35840
    (11, 13, 1): [(LATTICE, {MM_OPT_GRID_CELL: 300}, "cameras")],                  # 65248
    (13, 13, 2): [(LATTICE, {MM_OPT_GRID_CELL: 300, MM_OPT_LDS_NODES: 0}, "cameras")],
    (12, 12, 2): [(FINE_BIG, {MM_OPT_GRID_CELL: 200}, "cameras")],                 # 29664 + 34960
    (12, 12, 1): [(FINE, {}, "cameras")],                                          # 77616 + 2192
    (11, 12, 2): [(FINE, {MM_OPT_GRID_CELL: 200, MM_OPT_GRID_WIDE: 0}, "cameras")],      # 30928
    (11, 12, 1): [(FINE, {MM_OPT_GRID_CELL: 150}, "cameras")],                     # 57296
    (13, 12, 2): [(FINE, {MM_OPT_GRID_CELL: 200, MM_OPT_GRID_WIDE: 0, MM_OPT_LDS_NODES: 0}, "cameras")],
    (11, 14, 2): [(FINE, {MM_OPT_GRID_CELL: 300}, "cameras")],                     # 23872
    (11, 14, 1): [(FINE, {MM_OPT_GRID_CELL: 200}, "cameras")],                     # 49536
    (13, 14, 2): [(FINE, {MM_OPT_GRID_CELL: 200, MM_OPT_LDS_NODES: 0}, "cameras")],
    (3, 7, 2): [(maze(24), {MM_OPT_TRAVERSAL: 7}, "cameras")],                     # 45040 + 34960
    (3, 7, 1): [(maze(32), {MM_OPT_TRAVERSAL: 7}, "cameras")],                     # 77184 + 2192
}
# Built cells no launch reaches, with the rule of mm_plan.cpp that keeps them out.
_MODE13 = ("placement 13 stages 0 bytes, so plan_tile's loop over ring kinds {2, 1} always takes kind 2 "
           "(0 + its static LDS <= 80 KB); kind 1 would run only if kind 2 were not built")
UNREACHED = {(13, form, 1): _MODE13 for form in (11, 12, 13, 14, 15, 17)}


def _cases():
    out = []
    for (mode, form), (sc, opts) in PAIR_SITES.items():
        for entry, stats in (("tile", True), ("cameras", False), ("pixels", False), ("pixel_lists", True)):
            out.append(Case(sc, dict(opts), entry, stats, (mode, form, 0)))
    out.append(Case(maze(32), {}, "frames", False, (11, 17, 0)))
    out.append(Case(FINE, {MM_OPT_GRID_CELL: 200}, "frames", True, (11, 14, 0)))
    for (mode, form, ring), sites in RING_SITES.items():
        for sc, opts, entry in sites:
            out.append(Case(sc, {**opts, **RINGS}, entry, ring == 1, (mode, form, ring)))
    # N = 44: the image fits the array without rings only -- the forced deferral is dropped
    out.append(Case(maze(44), dict(RINGS), "cameras", False, (11, 17, 0)))
    out.append(Case(maze(44), {}, "tile", True, (11, 17, 0)))
    return out


CASES = _cases()
# the smallest wide slow soup of the table: FINE at the coarsest cells that still give wide words
WIDE_SLOW_SOUP = (FINE, {MM_OPT_GRID_CELL: 300})


# ---- the plan harness -----------------------------------------------------------
def build_harness(tmp_dir, build="plain"):
    exe = Path(tmp_dir) / f"launch_plan_{build}"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *HARNESS_BUILDS[build], f"-I{CSRC}",
                    f"-I{REPO / 'include'}", "-o", str(exe), *map(str, HARNESS_SRC)], check=True)
    return exe


def scene_args(key, tmp_dir):
    """The harness arguments that name a scene: n=N, or rects=FILE of a soup (written once per directory)."""
    if key[0] == "maze":
        return [f"n={key[1]}"]
    path = Path(tmp_dir) / f"{scene_id(key)}_{key[2]}.bin"
    if not path.exists():
        np.ascontiguousarray(scene(key).rects, dtype=np.float32).tofile(path)
    return [f"rects={path}"]


def plan(exe, key, opts, tmp_dir, entry="tile", w=32, h=16):
    """The harness's JSON for a scene, options and a call shape."""
    args = [str(exe), *scene_args(key, tmp_dir), *(f"{HARNESS_ARG[k]}={v}" for k, v in opts.items()),
            f"w={w}", f"h={h}", f"spp={SPP}", f"bounce={BOUNCES}", f"mirror={MIRRORS}",
            f"s1={STATIC_LDS[1]}", f"s2={STATIC_LDS[2]}"]
    if entry in ("frames", "cameras"):
        args += [f"frames={N_FRAMES}", f"multi=mm_trace_tile_{entry}"]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
    return json.loads(r.stdout)


def planned(j):
    """(mode, form, ring) of a harness answer every stage accepted."""
    assert j["method"]["code"] == 0 and j["placement"]["code"] == 0 and j["plan"]["code"] == 0, j
    assert j["placement"]["built"] == 1, j
    return j["placement"]["mode"], j["placement"]["form"], j["plan"]["ring"]


def built_cells():
    """Every (mode, form, ring) the library says it holds (mm_variant_built; host code, no GPU)."""
    from mirror_maze import lib

    fn = lib().mm_variant_built
    return {(m, f, r) for m in MODES for f in FORMS for r in RING_KINDS if fn(C.c_int(m), C.c_int(f), C.c_int(r)) == 1}
