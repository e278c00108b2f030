"""Shared by tests/test_grid_forms.py (CPU: the build facts, the image's structure
and the rays' input conditions) and tests/test_gpu_grid_forms.py (GPU against the
reference walk): hand-built "gallery" scenes that take each side of the decisions
grid_build.cpp makes for the maze forms (compact 16-byte records + class table,
the x / z walk, the slab shortcut), and three ray families for them.

The gallery is a 6 x 6 lattice of rooms 10 wide and 4 high between the planes
y = Y0 (the ceiling: y points down the image) and y = Y1 (the floor).  Its walls
cycle through the eight ways of writing the same rect -- (v, u) = (vertical,
horizontal) or the reverse, each side vector from either end -- so both normal
signs, both values of build_grid's `swap`, the y_first swap of z-normal records
and negative fold scales all reach the compact records.  Some walls are windows
(a strip under the ceiling and a strip on the floor), some are half height.
No coordinate of the scene is 0, so every edge has an ulp of the scene's scale.

Everything here is tuned on the host build (tests/grid_forms/grid_forms_host.cpp)
and the reference walk (tests/aov_ref.c) alone."""
from __future__ import annotations

import json
import subprocess
from pathlib import Path

import numpy as np

from grid_stress_support import _pack, camera  # noqa: F401  (camera: the GPU tests' views)

HERE = Path(__file__).resolve().parent
REPO = HERE.parent
CSRC = REPO / "mirror-maze_amd" / "csrc"
HOST_SRC = [HERE / "grid_forms" / "grid_forms_host.cpp",
            *(CSRC / f for f in ("scene.cpp", "rect_compact.cpp", "grid_build.cpp", "mm_plan.cpp"))]
HOST_BUILDS = {"plain": ["-O2"],
               "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}

MM_OPT_LDS_NODES, MM_OPT_TRAVERSAL, MM_OPT_DEFER, MM_OPT_DEFER_MIN, MM_OPT_GRID_CELL = 1, 7, 21, 22, 25
MM_INFO_GRID_OK, MM_INFO_GRID_CELLS_X, MM_INFO_GRID_CELLS_Y, MM_INFO_GRID_CELLS_Z, MM_INFO_GRID_GLOBAL = 1, 2, 3, 4, 5
MM_INFO_LEAN, MM_INFO_LAST_FORM, MM_INFO_GRID_FACES = 8, 11, 13
MM_INFO_GRID_FLAT, MM_INFO_GRID_SLAB, MM_INFO_GRID_CLASSES = 19, 20, 21

ROOM, ROOMS, HEIGHT = 10.0, 6, 4.0
X0, Y0, Z0 = 3.0, -1.5, -25.0                # the gallery's minimum corner
X1, Y1, Z1 = X0 + ROOM * ROOMS, Y0 + HEIGHT, Z0 + ROOM * ROOMS
WINDOW = (1.25, 1.25)                        # heights of a window wall's ceiling strip and floor strip
# twin_floor: its two coincident floors are a deck at mid height that reaches PLAZA beyond the gallery, and the
# whole scene is scaled by TWIN_SCALE (a power of two: every record stays as it is up to the exponent) -- rays
# from either side then meet the deck, few walls stand in the way, and fewer of the unnormalised rays are too
# close for a > 0.1: the general rays' tie share is 0.307 (tests/test_grid_forms.py has the other designs' shares)
PLAZA, TWIN_Y, TWIN_SCALE = 160.0, Y0 + 2.0, 4.0
N_RAYS = 4096 + 37

# scene -> the facts of its build (tests/test_grid_forms.py asserts them on the host program's output; a key
# that is absent is not asserted).  longest: the longest cell list; classes: threshold classes (flat only).
FACTS = {
    "base":        dict(flat_ok=1, slab=1, wide=1, n_glob=2, n_slow=0),
    "floor_only":  dict(flat_ok=1, slab=0, n_glob=1, n_slow=0),
    "no_planes":   dict(flat_ok=1, slab=0, n_glob=0, n_slow=0),
    "shelf3":      dict(flat_ok=1, slab=0, n_glob=3, glob_axes=["y"] * 3, n_slow=0),
    "shelf4":      dict(flat_ok=1, slab=0, n_glob=4, glob_axes=["y"] * 4, n_slow=0),
    "shelf5":      dict(flat_ok=0, n_glob=4, glob_axes=["y"] * 4, n_slow=0, cells_y=1),
    "twin_floor":  dict(flat_ok=1, slab=0, n_glob=2, n_slow=0),
    "classes64":   dict(flat_ok=1, n_class=64, n_slow=0),
    "classes65":   dict(flat_ok=0, n_slow=0, cells_y=1),
    "dense_cells": dict(flat_ok=1, wide=0, n_slow=0, longest_over=7),
    "tilted":      dict(flat_ok=0, n_slow_min=1, cells_y=1),
    "ledge":       dict(flat_ok=0, n_slow=0),
    "split_y":     dict(flat_ok=0, n_slow=0, cells_y_over=1),
}
SCENES = tuple(FACTS)
CELL = {"dense_cells": 300}                  # MM_OPT_GRID_CELL of the upload (default 100)
FLAT = tuple(n for n in SCENES if FACTS[n]["flat_ok"])


def check_facts(name, f):
    """The branch scene `name` was made for, on the facts of a build (host program or MM_INFO_* keys)."""
    want = FACTS[name]
    assert f["ok"] == 1, (name, f)
    for key in ("flat_ok", "slab", "wide", "n_glob", "n_slow", "n_class", "glob_axes"):
        if key in want and key in f:
            assert f[key] == want[key], (name, key, f[key], want[key])
    if "cells_y" in want:
        assert f["cells"][1] == want["cells_y"], (name, f["cells"])
    if "cells_y_over" in want:
        assert f["cells"][1] > want["cells_y_over"], (name, f["cells"])
    if "n_slow_min" in want and "n_slow" in f:
        assert f["n_slow"] >= want["n_slow_min"], (name, f["n_slow"])
    if "longest_over" in want and "longest" in f:
        assert f["longest"] > want["longest_over"], (name, f["longest"])


# ---- rects ----------------------------------------------------------------------
def _rect(axis, plane, h0, h1, y0, y1, conv):
    """The 9 floats (o, v, u) of the rect in the plane `axis` = plane over [h0, h1] of the
    horizontal in-plane axis (z for an x-normal rect, x for a z-normal one) and [y0, y1].
    conv bit 0: v is the horizontal side (else the vertical one); bit 1: v runs from the far end
    backwards; bit 2: u does.  A y-normal rect (axis 1, plane y): [h0, h1] along x and [y0, y1]
    along z, bit 0: v along z."""
    a, b = ((2, 1) if axis == 0 else (0, 1)) if axis != 1 else (0, 2)  # (horizontal, "vertical") in-plane axes
    ext = {a: (h0, h1), b: (y0, y1)}
    av, au = (a, b) if conv & 1 else (b, a)
    o, v, u = np.zeros(3), np.zeros(3), np.zeros(3)
    o[axis] = plane
    for side, ax_, neg in ((v, av, conv & 2), (u, au, conv & 4)):
        lo, hi = ext[ax_]
        o[ax_] = hi if neg else lo
        side[ax_] = lo - hi if neg else hi - lo
    return [*o, *v, *u]


def _fast(la, lb):
    """rect_compact.cpp's FAST condition for an axis-aligned la x lb rect, restated in float32:
    normalize(cross(v, u)) is exactly +-1."""
    c = np.float32(la) * np.float32(lb)
    rs = np.float32(1.0) / np.sqrt(np.float32(c * c))
    return np.float32(rs * c) == np.float32(1.0)


def _wall_slots(half_share=0):
    """The base gallery's walls: (axis, plane, h0, h1, kind, conv, w).  kind 0 full height, 1 a window
    (two strips), 2 half height (the floor half), 3 the ceiling half (split_y only).  w numbers the walls
    of one direction; conv = w % 8 cycles the eight conventions per direction."""
    out = []
    for axis in (0, 2):
        w = 0
        for i in range(ROOMS + 1):
            for j in range(ROOMS):
                outer = i in (0, ROOMS)
                if (outer and (i + j + axis // 2) % 6 == 2) or (not outer and (5 * i + 3 * j + axis) % 3 == 0):
                    continue  # a doorway
                plane = (X0 if axis == 0 else Z0) + ROOM * i
                h0 = (Z0 if axis == 0 else X0) + ROOM * j
                q = w + w // 8
                kind = 1 if q % 6 == 1 else (2 if q % 7 == 3 else 0)
                if half_share and q % 4 != 0:
                    kind = 2 + (q % 2)
                out.append([axis, plane, h0, h0 + ROOM, kind, w % 8, w, WINDOW[1], WINDOW[0]])
                w += 1
    return out


def _strips(kind, floor_strip=WINDOW[1], ceiling_strip=WINDOW[0]):
    if kind == 1:
        return [(Y0, Y0 + ceiling_strip), (Y1 - floor_strip, Y1)]
    if kind == 2:
        return [(Y0 + 2.25, Y1)]
    if kind == 3:
        return [(Y0, Y0 + 1.75)]
    return [(Y0, Y1)]


# classes64 / classes65: the window walls' floor strips and ceiling strips get heights of their own
# (1.25 -+ m / 16 for the m that keep the record FAST), then full-height walls are shortened to lengths of
# their own (10 - m / 8, likewise): each step is one new threshold class, and classes65 takes one step more
# than classes64 -- one more wall shortened
N_STEPS = 54  # (the gallery's own 12 classes, less the two these steps use up, plus 54)


def _class_steps(slots):
    lengths = [ROOM - 0.125 * m for m in range(1, 46) if _fast(HEIGHT, ROOM - 0.125 * m)]
    heights = [WINDOW[1] - 0.0625 * m for m in range(1, 16) if _fast(WINDOW[1] - 0.0625 * m, ROOM)]
    full, windows = [s for s in slots if s[4] == 0], [s for s in slots if s[4] == 1]
    raised = [WINDOW[0] + 0.0625 * m for m in range(1, 13) if _fast(WINDOW[0] + 0.0625 * m, ROOM)]
    return [(s, 7, v) for s, v in zip(windows, heights)] + [(s, 8, v) for s, v in zip(windows, raised)] + \
           [(s, "length", v) for s, v in zip(full, lengths)]


def build_rects(name):
    """(rects (n, 12) float32, is_mirror (n,), emission (n, 4), info): info["axis"][k] / ["conv"][k] /
    ["wall"][k] are rect k's normal axis, its convention and its wall number (-1: not a wall)."""
    assert name in SCENES, name
    planes = {"floor_only": [Y1], "no_planes": [], "twin_floor": [TWIN_Y, TWIN_Y]}.get(name, [Y1, Y0])
    rows, axis, conv, wall, mirror = [], [], [], [], []

    def add(r, a, c=-1, w=-1, m=0):
        rows.append(r), axis.append(a), conv.append(c), wall.append(w), mirror.append(m)

    # the planes first, the floor (the higher y) before the ceiling: the slab pair then needs its sort
    for i, y in enumerate(planes):
        m = PLAZA if name == "twin_floor" else 0.0
        add(_rect(1, y, X0 - m, X1 + m, Z0 - m, Z1 + m, (1, 6, 3, 4)[i]), 1)
    if name.startswith("shelf"):  # big y-normal rects between the planes, each over more than half of the cells
        shelves = [(Y0 + 1.0, X0, X1 - 8.0, Z0, Z1, 5), (Y0 + 3.0, X0 + 12.0, X1, Z0 + 6.0, Z1, 2),
                   (Y0 + 2.0, X0, X1, Z0 + 18.0, Z1, 7)]
        for y, xa, xb, za, zb, c in shelves[: int(name[5:]) - 2]:
            add(_rect(1, y, xa, xb, za, zb, c), 1)
    slots = _wall_slots(half_share=name == "split_y")
    if name.startswith("classes"):
        for s, what, value in _class_steps(slots)[: N_STEPS + (name == "classes65")]:
            if what != "length":
                s[what] = value
            elif s[6] % 2:
                s[2] = s[3] - value  # shortened from the near end, or from the far end
            else:
                s[3] = s[2] + value
    for a, plane, h0, h1, kind, c, w, floor_strip, ceiling_strip in slots:
        q = w + w // 8
        for (ya, yb) in _strips(kind, floor_strip, ceiling_strip):
            add(_rect(a, plane, h0, h1, ya, yb, c), a, c, w + 100 * a, int(q % 4 == 2))
    if name == "tilted":  # one wall whose normal is not axis-exact
        add([X0 + 14.0, Y0, Z0 + 12.0, 0.0, HEIGHT, 0.0, 0.5, 0.0, 6.0], -1)
    if name == "ledge":  # one small y-normal rect inside a room: a listed y-normal record
        add(_rect(1, Y0 + 2.0, X0 + 22.0, X0 + 26.0, Z0 + 32.0, Z0 + 36.0, 0), 1)
    n = len(rows)
    rects = np.zeros((n, 12), np.float32)
    rows = np.array(rows) * (TWIN_SCALE if name == "twin_floor" else 1.0)
    rects[:, 0:9] = rows
    assert (rects[:, 0:9].astype(np.float64) == rows).all()  # every coordinate is an exact float
    rng = np.random.default_rng(7)
    rects[:, 9:12] = rng.uniform(0.3, 0.9, (n, 3))
    emission = np.tile(np.float32([1, 0, 0, 0]), (n, 1))
    emission[len(planes) + 3] = np.float32([1.0, 0.9, 0.7, 3.0])  # one emitter
    info = {"axis": np.array(axis), "conv": np.array(conv), "wall": np.array(wall), "n_planes": len(planes)}
    return rects, np.array(mirror, np.uint8), emission, info


_SCENES = {}


def scene(name):
    """(Scene, info) of a gallery variant, built once (its BVH is Scene.bvh's)."""
    from mirror_maze import Scene

    if name not in _SCENES:
        rects, is_mirror, emission, info = build_rects(name)
        nodes, idx = Scene.bvh(rects)
        _SCENES[name] = (Scene(0, rects, nodes, idx, is_mirror, emission, np.zeros((0, 0), np.uint8), 0), info)
    return _SCENES[name]


# ---- the host program -----------------------------------------------------------
def build_host(tmp_dir, build="plain"):
    exe = Path(tmp_dir) / f"grid_forms_host_{build}"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *HOST_BUILDS[build], f"-I{CSRC}",
                    f"-I{REPO / 'include'}", "-o", str(exe), *map(str, HOST_SRC)], check=True)
    return exe


def run_host(exe, rects, tmp_dir, cell=100, wide=1, merge=1, dump=False):
    """The host program's facts for a rect array (and the image's bytes with dump)."""
    tmp_dir = Path(tmp_dir)
    path = tmp_dir / "rects.bin"
    np.ascontiguousarray(rects, dtype=np.float32).tofile(path)
    args = [str(exe), f"rects={path}", f"cell={cell}", f"wide={wide}", f"merge={merge}"]
    if dump:
        args.append(f"dump={tmp_dir / 'image.bin'}")
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
    facts = json.loads(r.stdout)
    return (facts, (tmp_dir / "image.bin").read_bytes()) if dump else facts


def host_facts(exe, name, tmp_dir, **kw):
    return run_host(exe, build_rects(name)[0], tmp_dir, cell=CELL.get(name, 100), **kw)


# ---- rays -----------------------------------------------------------------------
def _ulps(x, k):
    """float32 x moved k floats away from zero (k < 0: towards it); x != 0, |k| small."""
    return (np.ascontiguousarray(x, dtype=np.float32).view(np.int32) + k.astype(np.int32)).view(np.float32)


def _extent(rects):
    """(lo, hi) (n, 3) of every rect's box, float64 (the coordinates are exact floats)."""
    r = np.asarray(rects[:, 0:9], dtype=np.float64)
    c = np.stack([r[:, 0:3], r[:, 0:3] + r[:, 3:6], r[:, 0:3] + r[:, 6:9], r[:, 0:3] + r[:, 3:6] + r[:, 6:9]])
    return c.min(axis=0), c.max(axis=0)


def edge_groups(info):
    """The groups the edge rays are dealt over: the 16 (wall direction, convention) pairs, and the
    y-normal rects (planes, shelves, the ledge) as one more where the scene has any."""
    groups = [(a, c) for a in (0, 2) for c in range(8)]
    return groups + ([(1, -1)] if (info["axis"] == 1).any() else [])


def edge_rays(name, ref, n=N_RAYS, seed=200):
    """Family 1: rays aimed at points on the edges and corners of the scene's rects -- window sills,
    wall ends, shelf rims -- from 3 to 40 away, inside and outside the scene box, and with a clear view:
    the reference walk, asked from the same origin for a point 0.05 inside the rect, answers that rect.
    The direction is the float32 normalised difference with each component moved by -3..3 floats.
    Returns (rays, target rect, edge axis, edge coordinate, group index), the groups being
    edge_groups' and each getting n / len(groups) rays (the first ones one more)."""
    s, info = scene(name)
    lo, hi = _extent(s.rects)
    groups = edge_groups(info)
    rng = np.random.default_rng(seed)
    quota = [n // len(groups) + (g < n % len(groups)) for g in range(len(groups))]
    out = [[] for _ in groups]
    for g, (a, c) in enumerate(groups):
        ks = np.flatnonzero((info["axis"] == a) & (info["conv"] == c))
        assert len(ks), (name, a, c)
        have = 0
        for _ in range(40):
            if have >= quota[g]:
                break
            m = 4 * quota[g]
            k = rng.choice(ks, m)
            inplane = np.array([x for x in range(3) if x != a])
            e = inplane[rng.integers(2, size=m)]          # the edge's axis: the edge is e = lo or hi
            other = inplane.sum() - e
            end = rng.integers(2, size=m)
            P = np.zeros((m, 3))
            P[:, a] = lo[k, a]
            rows = np.arange(m)
            edge = np.where(end == 1, hi[k, e], lo[k, e])
            P[rows, e] = edge
            t = rng.uniform(0.0, 1.0, m)
            t = np.where(rng.random(m) < 0.2, np.round(t), t)  # one in five at a corner
            P[rows, other] = lo[k, other] + t * (hi[k, other] - lo[k, other])
            inside = P.copy()                             # 0.05 inside the rect from the aim point
            inside[rows, e] += np.where(end == 1, -0.05, 0.05)
            inside[rows, other] += np.where(t == 0.0, 0.05, np.where(t == 1.0, -0.05, 0.0))
            d = rng.normal(size=(m, 3))
            d /= np.linalg.norm(d, axis=1, keepdims=True)
            d[:, a] = np.where(np.abs(d[:, a]) < 0.2, np.copysign(0.2, d[:, a]), d[:, a])
            d /= np.linalg.norm(d, axis=1, keepdims=True)
            O = np.float32(P + rng.uniform(3.0, 40.0, (m, 1)) * d).astype(np.float64)
            los = inside - O
            los /= np.linalg.norm(los, axis=1, keepdims=True)
            _, seen = ref.query(_pack(O, los, rng))
            aim = P - O
            aim = np.float32(aim / np.linalg.norm(aim, axis=1, keepdims=True))
            moved = _ulps(np.where(aim == 0, np.float32(1e-30), aim), rng.integers(-3, 4, size=(m, 3)))
            aim = np.where(aim == 0, aim, moved)
            for i in np.flatnonzero(seen == k)[: quota[g] - have]:
                out[g].append((O[i], aim[i], k[i], e[i], edge[i]))
            have = len(out[g])
        assert have == quota[g], (name, a, c, have)
    flat = [(x, g) for g, rows_ in enumerate(out) for x in rows_]
    O = np.array([x[0][0] for x in flat])
    d = np.array([x[0][1] for x in flat])
    rays = _pack(O, d, rng)
    return (rays, np.array([x[0][2] for x in flat]), np.array([x[0][3] for x in flat]),
            np.array([x[0][4] for x in flat]), np.array([x[1] for x in flat]))


def near_edge(rays, rects, target, e_axis, e_coord, ulps=4):
    """Which edge rays cross their target's plane within `ulps` floats of the targeted edge coordinate
    (the crossing in float64 from the float32 ray)."""
    lo, _ = _extent(rects)
    o, d = rays[:, 0, :3].astype(np.float64), rays[:, 1, :3].astype(np.float64)
    n = len(rays)
    rows = np.arange(n)
    normal = np.array([int(np.flatnonzero(np.ptp(np.stack([rects[k, 0:3], rects[k, 0:3] + rects[k, 3:6],
                                                           rects[k, 0:3] + rects[k, 6:9]]), axis=0) == 0)[0])
                       for k in target])
    a = (lo[target, normal] - o[rows, normal]) / d[rows, normal]
    p = o[rows, e_axis] + a * d[rows, e_axis]
    return np.abs(p - e_coord) <= ulps * np.spacing(np.float32(np.abs(e_coord))).astype(np.float64)


def slab_rays(n=N_RAYS, seed=210):
    """Family 2: origins on the ceiling and floor planes y = Y0, Y1 and off them by one float and by
    0.05 |d_y| (the slab shortcut's own bound, mm_grid.h grid_search) to either side; d_y of both signs,
    zero and +-2^-20.  Rays come in groups of 64 (a wave of mm_query_rays): in the even groups the lanes
    alternate between up and down, with lanes of d_y = 0, d_y = +-2^-20 and origins outside the slab
    heading in (no plane can be skipped for those, so the wave tests every global rect); the odd groups
    point one way from origins on a plane (every lane skips one plane).
    Returns (rays, on_plane): on_plane marks origins within one float of a plane."""
    rng = np.random.default_rng(seed)
    f32 = np.float32
    o, d = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    on_plane = np.zeros(n, bool)
    for i in range(n):
        grp, lane = divmod(i, 64)
        plane = f32((Y0, Y1)[int(rng.integers(2))])
        mixed = grp % 2 == 0
        if mixed:
            sign = 1.0 if lane % 2 else -1.0
            kind = 2 if lane % 16 == 7 else (3 if lane % 16 == 12 else 0)
        else:
            sign = 1.0 if grp % 4 == 1 else -1.0
            kind = 3 if lane % 16 == 5 else 0
        dy = f32(sign * rng.uniform(0.05, 1.0)) if kind == 0 else (f32(0.0) if kind == 2 else f32(sign * 2.0 ** -20))
        th = rng.uniform(0, 2 * np.pi)
        hz = np.sqrt(max(0.0, 1.0 - float(dy) ** 2))
        d[i] = (f32(hz * np.cos(th)), dy, f32(hz * np.sin(th)))
        off = int(rng.integers(5)) if mixed else int(rng.integers(3))
        q = f32(0.05) * f32(abs(dy))
        y = (plane, np.nextafter(plane, f32(np.inf)), np.nextafter(plane, f32(-np.inf)), f32(plane + q),
             f32(plane - q))[off]
        on_plane[i] = off < 3 or q == 0
        x, z = rng.uniform(X0, X1), rng.uniform(Z0, Z1)
        if rng.random() < 0.125:
            x += float(rng.choice([-1, 1])) * ROOM * ROOMS * rng.uniform(0.5, 1.0) * (rng.random() < 0.5)
            z += float(rng.choice([-1, 1])) * ROOM * ROOMS * rng.uniform(0.5, 1.0) * (rng.random() < 0.5)
        o[i] = (f32(x), y, f32(z))
    return _pack(o, d, rng), on_plane


def slab_ballots(rays):
    """Per group of 64 rays, whether mm_grid.h's slab shortcut applies to the whole wave (every lane can
    skip one of the two planes), restated in float32 for the planes Y0 < Y1."""
    oy, dy = rays[:, 0, 1], rays[:, 1, 1]
    q = np.float32(0.05) * dy
    lo_dead = (dy > 0) & (np.float32(Y0) - oy <= q)
    hi_dead = (dy < 0) & (np.float32(Y1) - oy >= q)
    dead = lo_dead | hi_dead
    return np.array([dead[i:i + 64].all() for i in range(0, len(rays), 64)])


def general_rays(name, n=N_RAYS, seed=300):
    """Family 3: the eight ray kinds of test_gpu_aov.py's test_query_rays_bit_exact, as they are."""
    from test_gpu_aov import _rays

    return _rays(scene(name)[0], n, seed)


_RAYS = {}


def rays(name, family, ref=None):
    """The (N_RAYS, 2, 4) rays of a family for a scene, made once (edge rays: needs a Ref of the scene)."""
    key = (name, family) if family != "slab" else family
    if key not in _RAYS:
        v = {"edge": lambda: edge_rays(name, ref), "slab": slab_rays, "general": lambda: (general_rays(name),)}[family]()
        for a in v:
            a.setflags(write=False)
        _RAYS[key] = v
    return _RAYS[key]


FAMILIES = ("edge", "slab", "general")


# ---- cameras --------------------------------------------------------------------
VIEW = (80, 60)       # test_gpu_aov.py's frame, for its ragged TILES
WINDOW_VIEW = (96, 64)
WINDOWS = [(24, 20), (40, 30)]  # 32 x 16 each


def mirror_wall():
    """The first interior full-height x-normal mirror of the base gallery: (plane x, z0, z1)."""
    for a, plane, h0, h1, kind, c, w, *_ in _wall_slots():
        if a == 0 and kind == 0 and (w + w // 8) % 4 == 2 and X0 < plane < X1:
            return plane, h0, h1
    raise AssertionError("no mirror wall")


def cameras(view=VIEW):
    """{"inside": in a room beside a mirror wall, looking along it and a little into it;
    "above": outside the box over the (open, in floor_only) roof, looking down into the rooms}."""
    plane, z0, z1 = mirror_wall()
    inside = camera((plane + 0.75, Y0 + 1.75, z0 + 0.5), (-0.08, 0.03, 1.0), 1.6, 1.6 * view[1] / view[0], view)
    above = camera((X0 + 27.0, Y0 - 30.0, Z0 + 31.0), (0.05, 1.0, 0.08), 1.2, 1.2 * view[1] / view[0], view)
    return {"inside": inside, "above": above}
