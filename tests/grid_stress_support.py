"""Shared by tests/test_grid_stress.py (CPU: the input conditions, and the CPU
twin of the grid search against the walk) and tests/test_gpu_grid_stress.py
(GPU against the walk): seeded scenes, cameras and rays that put the certified
grid search (mm_grid.h, mm_path.h GridQuery) where its eps argument is thin.

  A  bounce rays whose origin lies outside the grid box (a telephoto camera far
     from the scene rounds ori + t * dir to ulp(distance)); GridQuery skips the
     box check for them
  B  hits on the scene box's extreme faces and grazing bounces off them, in the
     3-D walk
  C  rays whose x and z crossing times tie, and rays that leave the grid through
     a vertical box edge
  D  test_gpu_aov.py's eight ray kinds on the 3-D grids (soup, lattice)

Everything here is tuned on the reference walk alone (tests/aov_ref.c), as
aov_support.make_corridor was."""
from __future__ import annotations

import math

import numpy as np

import aov_support as A

MM_OPT_LDS_NODES, MM_OPT_TRAVERSAL, MM_OPT_DEFER, MM_OPT_DEFER_MIN = 1, 7, 21, 22
MM_OPT_GRID_CELL, MM_OPT_GRID_WIDE = 25, 26
MM_INFO_GRID_OK, MM_INFO_GRID_CELLS_X, MM_INFO_GRID_CELLS_Y, MM_INFO_GRID_CELLS_Z = 1, 2, 3, 4
MM_INFO_GRID_FACES, MM_INFO_GRID_FLAT = 13, 19

PITCH = 8.0      # the crate's lattice (placement 1 and 3; 2^-3 in placement 2)
HALF = 64.0      # its half-width
# placement 3's centre: the y faces at -8192 and -8064 (C = 8192 = 2^6 extents); the x and z faces at
# coordinates with fraction bits, off every float grid coarser than 1/8 -- the -x mirror at -8191.375, 0.625
# inside the grid point -8192 of every coarser float grid, which is 0.125 beyond the widened box (eps = 0.5):
# a hit point computed by a camera whose coordinates have ulp >= 2 lands there or 2 or more inside
CENTRE3 = (-8127.375, -8128.0, 4095.375)
# Lines along which two of the crate's rects cross, as ((axis, plane), (axis, plane)); each rect reaches 16 to
# either side of the line and runs 8 along it.  The first lies in x = 0 and z = 0, which at MM_OPT_GRID_CELL 100 are cell boundaries to the last bit
# (boundary 8 of 16 of a grid symmetric about 0): a ray aimed at the line finds two hits an ulp apart on either
# side of a boundary whose crossing time is an ulp off too -- the case the lists' eps is for.
JUNCTIONS = (((0, 0.0), (2, 0.0)), ((0, -24.0), (1, 8.0)))
JUNCTION_AT = -40.0  # where along its line each pair runs (8 long), out of the way of the cameras' paths
CELLS = (100, 130, 70)  # MM_OPT_GRID_CELL: at 100 the lattice lies on the cell boundaries (16 cells of 8 + eps/8)
PLACEMENTS = (1, 2, 3)
A_DISTANCES = {1: (20,), 3: (12, 16)}  # log2(D / C) per placement (telephoto's docstring has the ones left out)
VIEW = (96, 64)
A_WINDOWS = [(32, 0), (64, 16), (32, 48)]     # 32 x 16 each
A_TILE = (14, 20, 67, 5, 6)                   # x0, y0, w, h, y_stride
B_WINDOWS = [(24, 20), (40, 30)]
B_TILE = (14, 4, 67, 5, 13)


# ---- scenes --------------------------------------------------------------------
def _face(axis, side, lo, hi):
    """The rect of face `axis` = +-HALF over [lo, hi]^2 of the other two axes,
    its normal (cross(v, u), the kernel's) pointing into the crate."""
    b, c = [a for a in range(3) if a != axis]
    o, v, u = np.zeros(3), np.zeros(3), np.zeros(3)
    o[axis] = side * HALF
    o[b], o[c] = lo[0], lo[1]
    v[b], u[c] = hi[0] - lo[0], hi[1] - lo[1]
    if np.cross(v, u)[axis] * side > 0:  # pointing out: swap
        v, u = u, v
    return [*o, *v, *u]


def crate(placement: int):
    """A closed axis-aligned cube of six face rects -- the two x faces mirrors
    facing each other, the -y face a light, the +x face's rect covering only
    z <= 0 (the opening case A's cameras look through) -- with 44 axis-aligned
    rects inside it on a lattice of PITCH: the first 10 start on a face, the
    next 8 continue a neighbour in its own plane (sharing an edge), the last
    four cross in pairs (JUNCTIONS).
    placement 1: centred at the origin, half-width 64; 2: that scaled by 2^-6;
    3: half-width 64 around CENTRE3, C / extent = 2^6."""
    from mirror_maze import Scene

    rng = np.random.default_rng(20)
    full = ([-HALF, -HALF], [HALF, HALF])
    rects = [_face(0, -1, *full), _face(0, 1, [-HALF, -HALF], [HALF, 0.0]), _face(1, -1, *full), _face(1, 1, *full),
             _face(2, -1, *full), _face(2, 1, *full)]
    n_in = 40
    for i in range(n_in):
        if 10 <= i < 18:  # continue rect i - 10 along its v edge, in its plane
            o, v, u = (np.array(rects[6 + i - 10][j:j + 3]) for j in (0, 3, 6))
            o2 = o + v
            room = HALF - np.abs(o2 + v)  # stay inside the crate
            if (room < 0).any():
                o2 = o - v
            rects.append([*o2, *v, *u])
            continue
        k = int(rng.integers(3))
        b, c = [a for a in range(3) if a != k]
        o, v, u = np.zeros(3), np.zeros(3), np.zeros(3)
        o[k] = PITCH * int(rng.integers(-6, 7))
        lv, lu = PITCH * int(rng.integers(1, 3)), PITCH * int(rng.integers(1, 4))
        o[b] = -HALF if i < 10 else PITCH * int(rng.integers(-8, 8 - lv // PITCH + 1))
        o[c] = PITCH * int(rng.integers(-8, 8 - lu // PITCH + 1))
        v[b], u[c] = lv, lu
        if rng.random() < 0.5:
            v, u = u, v
        rects.append([*o, *v, *u])
    for line in JUNCTIONS:  # two rects that cross along `line`, each in a lattice plane
        (ax, a), (bx, b) = line
        free = 3 - ax - bx
        for k, c, other, d in ((ax, a, bx, b), (bx, b, ax, a)):
            o, v, u = np.zeros(3), np.zeros(3), np.zeros(3)
            o[k], o[other], o[free] = c, d - 2 * PITCH, JUNCTION_AT
            v[other], u[free] = 4 * PITCH, PITCH  # (8 along the line: the median rect extent stays 8)
            rects.append([*o, *v, *u])
    rects = np.array(rects)
    shift = {1: (0.0, 0.0, 0.0), 2: (0.0, 0.0, 0.0), 3: CENTRE3}[placement]
    rects[:, 0:3] += shift
    if placement == 2:
        rects *= 2.0 ** -6
    n = len(rects)
    out = np.zeros((n, 12), np.float32)
    out[:, 0:9] = rects
    out[:, 9:12] = rng.uniform(0.3, 0.9, (n, 3))
    assert (out[:, 0:9].astype(np.float64) == rects).all()  # lattice coordinates are exact floats
    is_mirror = np.zeros(n, np.uint8)
    is_mirror[0:2] = 1
    emission = np.tile(np.float32([1, 0, 0, 0]), (n, 1))
    emission[2] = np.float32([1.0, 0.9, 0.7, 3.0])
    nodes, idx = Scene.bvh(out)
    return Scene(0, out, nodes, idx, is_mirror, emission, np.zeros((0, 0), np.uint8), 0)


def crate_centre(placement):
    return {1: np.zeros(3), 2: np.zeros(3), 3: np.array(CENTRE3)}[placement]


def crate_scale(placement):
    return 2.0 ** -6 if placement == 2 else 1.0


_SCENES = {}


def scene(name):
    """crate1 / crate2 / crate3, soup, lattice, maze10, maze64 -- built once."""
    from mirror_maze import Scene

    if name not in _SCENES:
        if name.startswith("crate"):
            s = crate(int(name[5:]))
        elif name in ("soup", "lattice"):
            from test_gpu_random_scene import random_scene

            s = random_scene(3000, 11 if name == "lattice" else 7, name == "lattice")
        else:
            s = Scene.build(int(name[4:]), 0)
        _SCENES[name] = s
    return _SCENES[name]


# ---- the grid, restated ----------------------------------------------------------
def corners(rects):
    r = np.asarray(rects, dtype=np.float64)
    return np.stack([r[:, 0:3], r[:, 0:3] + r[:, 3:6], r[:, 0:3] + r[:, 6:9], r[:, 0:3] + r[:, 3:6] + r[:, 6:9]])


def grid_of(s, cell_pct: int = 100):
    """grid_build.cpp build_lists' geometry (lines 121-150) and build_grid's first
    cell size, restated: the box of every rect corner widened by eps = 2^-14 C
    and one float outwards, n = round(extent / s) cells per axis for s = the
    median second-largest rect extent x cell_pct / 100.  (Not restated: the
    merge of an axis into one cell -- the mazes' y -- and the growth of s when
    the index does not fit LDS; the GPU tests compare n with MM_INFO_GRID_CELLS_*.)"""
    c = corners(s.rects)
    lo, hi = c.min(axis=0), c.max(axis=0)  # (n, 3) per rect
    smin, smax = lo.min(axis=0), hi.max(axis=0)
    C = max(1.0, float(np.abs(c).max()))
    eps = C * 2.0 ** -14
    e = np.sort(hi - lo, axis=1)[:, 1]
    e = np.sort(e[e > 0])
    size = float(e[len(e) // 2]) * cell_pct / 100.0
    mn = np.nextafter(np.float32(smin - eps), np.float32(-np.inf))
    mx = np.nextafter(np.float32(smax + eps), np.float32(np.inf))
    ext = mx.astype(np.float64) - mn.astype(np.float64)
    n = np.clip(np.floor(ext / size + 0.5), 1, 256).astype(int)
    cell = (ext / n).astype(np.float32)
    return {"mn": mn, "mx": mx, "cell": cell, "n": n, "eps": eps, "C": C, "smin": smin, "smax": smax}


def outside(g, pts, margin=0.0):
    """Which (n, 3) points lie outside the grid box [mn, mx] (grid_ray_ok would
    refuse them), by more than `margin`."""
    p = np.asarray(pts, dtype=np.float64)
    return ((p < g["mn"].astype(np.float64) - margin) | (p > g["mx"].astype(np.float64) + margin)).any(axis=1)


def bounce_starts(rec, centre):
    """Of recorded queries (Ref.recorded): the mask of those that do not start
    at the camera, i.e. at a hit point."""
    return (rec[:, 0:3] != np.float32(centre)).any(axis=1)


# ---- cameras --------------------------------------------------------------------
def look_quat(f):
    """The camera quaternion (x, y, z, w) whose view axis (+z of the image
    plane) is f.  (quat_mult applies the conjugate: hence the sign.)"""
    f = np.asarray(f, dtype=np.float64)
    f = f / np.linalg.norm(f)
    ax = np.cross([0.0, 0.0, 1.0], f)
    s = np.linalg.norm(ax)
    if s < 1e-12:
        return np.float32([0, 0, 0, 1]) if f[2] > 0 else np.float32([0, 1, 0, 0])
    th = math.atan2(s, f[2])
    ax = ax / s
    return np.float32([*(-math.sin(th / 2) * ax), math.cos(th / 2)])


def camera(centre, forward, vw, vh, view=VIEW):
    cam = np.float32([*centre, 1.0, *look_quat(forward), vw, vh])
    return A.uniform_of(cam, *view)


# from the crate towards case A's cameras: along x through the +x opening onto the -x mirror, and steep enough
# in y and z that the reflected ray soon meets a matte face (every later bounce origin is an accurate one)
A_DIAGONAL = np.array([0.93, 0.17, 0.33])


def telephoto(placement, log2_d):
    """Case A: a camera at D = 2^log2_d C from the crate's centre on a diagonal,
    looking back at it through a viewport 1.6 crate diagonals wide at that
    distance.  Its hit points ori + t * dir are multiples of ulp(D), which is
    4 eps at 2^12 C (eps = 2^-14 C).

    Distances kept per placement (A_DISTANCES), by the rule that at least one
    quarter of the bounce origins of every compared tile lie outside the grid
    box (tests/test_grid_stress.py):
      placement 3, 2^12 C and 2^16 C   the -x mirror is off the float grid of
          the hit points (CENTRE3): about 3/4 and all of them land outside;
      placement 3, 2^20 C   left out: ulp(D) = 1024 there, eight crates wide --
          the pixels share one direction, and it misses the crate;
      placement 1, 2^20 C   kept (the hit points' y and z are 4 apart as well);
      placement 1, 2^12 C and 2^16 C   left out: the faces at +-64 lie ON the
          hit points' float grid, the computed point is face + m ulp(D) with
          m = the rounded error of t * dir_x in units of ulp(D), |error| <
          1.5 ulp, so m = 0 for more than half of them and m = -1 (outside)
          for fewer than a quarter: measured 17 % and 21 %."""
    sc, c = crate_scale(placement), crate_centre(placement) * crate_scale(placement)
    C = max(1.0, float(np.abs(c).max() + HALF * sc))
    D = 2.0 ** log2_d * C
    u = A_DIAGONAL / np.linalg.norm(A_DIAGONAL)
    wide = 1.6 * 2 * HALF * sc * math.sqrt(3.0) / D
    return camera(c + D * u, -u, wide, wide * VIEW[1] / VIEW[0])


def grazing(placement, which):
    """Case B: a camera inside the crate 2^-3 of a cell (PITCH / 8) from a face,
    looking along it and 0.012 rad towards it through a viewport 0.05 wide, so
    that half of its rays meet the face at |d . n| < 0.04 and the mirror sends
    them on at the same angle.  which 0: along the -x mirror towards +z;
    1: along it towards -z."""
    sc, c = crate_scale(placement), crate_centre(placement)
    d = PITCH / 8
    if which == 0:
        p, f = np.array([-HALF + d, 10.0, -HALF + 5.0]), np.array([-0.012, 0.03, 1.0])
    else:
        p, f = np.array([-HALF + d, -20.0, HALF - 5.0]), np.array([-0.012, -0.02, -1.0])
    return camera((c + p) * sc, f, 0.05, 0.4)


# Distance (in t) of case C's outbound rays from the face they leave through: the wall is nearer than the
# reference's a > 0.1 and so not hit, and the grid's boundary is past the point at t = 3/32 the walk starts from
REACH = (0.0945, 0.0995)


# ---- rays -----------------------------------------------------------------------
def _pack(o, d, rng):
    n = len(o)
    rays = np.zeros((n, 2, 4), np.float32)
    rays[:, 0, :3], rays[:, 1, :3] = o, d
    rays[:, :, 3] = rng.normal(size=(n, 2))  # the w components are ignored
    return rays


def face_rays(placement, n, seed):
    """Case B's three kinds in turn: origin exactly on a face rect, direction
    within 2^-10 rad of the face (either side of it); origin on an edge or a
    corner of the box, direction into the box; origin on a face, direction
    exactly within it."""
    rng = np.random.default_rng(seed)
    sc, c = crate_scale(placement), crate_centre(placement)
    o, d = np.zeros((n, 3)), np.zeros((n, 3))
    for i in range(n):
        a = int(rng.integers(3))
        side = int(rng.choice([-1, 1]))
        p = np.round(rng.uniform(-HALF, HALF, 3) * 16) / 16
        p[a] = side * HALF
        v = rng.normal(size=3)
        if i % 3 == 0:
            v[a] = 0.0
            v /= np.linalg.norm(v)
            v[a] = rng.uniform(2.0 ** -20, 2.0 ** -10) * rng.choice([-1, 1])
        elif i % 3 == 1:
            others = [x for x in range(3) if x != a]
            for b in others[: 1 + int(rng.integers(2))]:
                p[b] = int(rng.choice([-1, 1])) * HALF
            v = -np.sign(p) * np.abs(v)
            v /= np.linalg.norm(v)
        else:
            v[a] = 0.0
            v /= np.linalg.norm(v)
        o[i], d[i] = (c + p) * sc, v
    return _pack(o, d, rng)


def junction_rays(placement, n, seed):
    """Case B, fourth kind: rays from 20 to 40 away aimed at a point of a
    JUNCTIONS line (the aim is a float64 point, the direction its float32
    rounding: the ray passes the line within about 1e-6 of the distance, on
    either side), from all four quadrants around the line."""
    rng = np.random.default_rng(seed)
    sc, c = crate_scale(placement), crate_centre(placement)
    o, d = np.zeros((n, 3)), np.zeros((n, 3))
    for i in range(n):
        (ax, a), (bx, b) = JUNCTIONS[i % len(JUNCTIONS)]
        free = 3 - ax - bx
        p = np.zeros(3)
        p[ax], p[bx], p[free] = a, b, JUNCTION_AT + rng.uniform(0.05, 0.95) * PITCH
        v = rng.normal(size=3)
        v[free] *= 0.3
        v /= np.linalg.norm(v)
        dist = rng.uniform(20.0, 40.0)
        org = np.float32((c + p - dist * v) * sc).astype(np.float64)
        p[ax] += rng.normal() * 4e-7 * dist  # a few ulp of the distance off the line: few exact ties (the walk's)
        p[bx] += rng.normal() * 4e-7 * dist
        aim = (c + p) * sc - org
        o[i], d[i] = org, aim / np.linalg.norm(aim)
    return _pack(o, d, rng)


def tied_rays(g, n, seed, reach=REACH):
    """Case C: |d.x| == |d.z| = h exactly.  In turn: (0) origin with equal float32
    offsets from the grid's minimum corner in x and z, on a cell corner;
    (1) the same off the corners; (2) origin REACH * h from a vertical edge
    of the scene box, aimed out through it (the walls there are nearer than the
    reference's a > 0.1, so the ray leaves the grid); (3) origin
    REACH * h from a z face of the scene box, aimed out through it, and as far
    from an interior x boundary as from the grid's last z boundary, so that it
    enters an x cell at the instant it leaves the grid."""
    rng = np.random.default_rng(seed)
    mn, cell, nn = g["mn"], g["cell"], g["n"]
    ylo, yhi = float(g["smin"][1]), float(g["smax"][1])
    o, d = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    f32 = np.float32
    for i in range(n):
        kind = i % 4
        sx, sz = (f32(x) for x in rng.choice([-1.0, 1.0], size=2))
        h = f32(rng.uniform(0.3, 1.0))
        dy = f32(rng.uniform(-0.25, 0.25))
        y = f32(rng.uniform(ylo + 0.2 * (yhi - ylo), yhi - 0.2 * (yhi - ylo)))
        m = min(int(nn[0]), int(nn[2]))
        a = f32(rng.uniform(*reach)) * h
        if kind == 2:
            ox = f32(g["smax"][0]) - a if sx > 0 else f32(g["smin"][0]) + a
            oz = f32(g["smax"][2]) - a if sz > 0 else f32(g["smin"][2]) + a
            dy = f32(dy * f32(0.1))
        elif kind == 3:
            oz = f32(g["smax"][2]) - a if sz > 0 else f32(g["smin"][2]) + a
            last = f32(nn[2]) * cell[2] if sz > 0 else f32(0.0)
            off = f32(f32(mn[2] - oz) + last)  # to the last z boundary, as the walk's A + b B has it
            b = int(rng.integers(1, int(nn[0])))
            ox = f32(f32(mn[0] + f32(b) * cell[0]) - sx * sz * off)
            dy = f32(dy * f32(0.1))
        else:
            b = int(rng.integers(1, m))
            off = f32(b) * cell[0] if kind == 0 else f32(rng.uniform(0.02, 0.98) * float(cell[0]) * m)
            ox = f32(mn[0] + off)
            oz = f32(mn[2] + f32(ox - mn[0]))  # (the offset the walk computes)
        o[i], d[i] = (ox, y, oz), (sx * h, dy, sz * h)
    return _pack(o, d, rng)


def walked_grid(name, g):
    """The grid the device walks for scene `name`, from the restated one: the
    mazes' y axis is merged into one cell (grid_build.cpp; MM_INFO_GRID_CELLS_Y
    == 1 on the GPU)."""
    if not name.startswith("maze"):
        return g
    w = dict(g)
    w["n"] = np.array([g["n"][0], 1, g["n"][2]])
    w["cell"] = np.float32([g["cell"][0], np.float32(float(g["mx"][1]) - float(g["mn"][1])), g["cell"][2]])
    return w


# ---- measures ---------------------------------------------------------------------
def on_face_hits(rec):
    """Recorded queries whose hit is one of the crate's six face rects."""
    k = rec[:, 7].view(np.uint32)
    return k < 6


def grazing_starts(rec, centre, bound=2.0 ** -6):
    """Recorded queries that start at a hit point on a face rect (the query
    before them hit one) with |d . n| < bound."""
    k = rec[:, 7].view(np.uint32)
    start = bounce_starts(rec, centre)
    prev_face = np.concatenate([[False], k[:-1] < 6])
    axis = np.concatenate([[0], np.minimum(k[:-1], 5) // 2])
    dn = np.abs(rec[np.arange(len(rec)), 4 + axis])
    nrm = np.linalg.norm(rec[:, 4:7].astype(np.float64), axis=1)
    return start & prev_face & (dn < bound * nrm)


# ---- the cases' inputs (the CPU and the GPU tests use the same) ------------------------
A_CASES = [(pl, ld) for pl in sorted(A_DISTANCES) for ld in A_DISTANCES[pl]]
A_LIMITS = (2, 15, 200)
A_WINDOW_CASE = (1, 12)  # the telephoto windows of trace_tile (test_grid_stress.py says why only these)
C_SCENES = ("maze10", "maze64", "crate1")
N_RAYS = 4096 + 37


def ext():
    from mirror_maze import make_ext

    return make_ext(8, 8, 8, frame=1)


_INPUTS = {}


def b_rays(placement):
    if ("b", placement) not in _INPUTS:
        _INPUTS[("b", placement)] = face_rays(placement, N_RAYS, seed=40 + placement)
    return _INPUTS[("b", placement)]


def j_rays(placement):
    if ("j", placement) not in _INPUTS:
        _INPUTS[("j", placement)] = junction_rays(placement, 4096, seed=60 + placement)
    return _INPUTS[("j", placement)]


def c_grid(name):
    return walked_grid(name, grid_of(scene(name)))


def c_rays(name):
    if ("c", name) not in _INPUTS:
        _INPUTS[("c", name)] = tied_rays(c_grid(name), 4096, seed=50)
    return _INPUTS[("c", name)]
