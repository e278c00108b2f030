"""Shared by tests/test_gpu_trace_rays.py: the CPU reference of mm_trace_rays
(tests/rays_ref.c -- the resolve and the jitter stated over the oracle's
trace_path and tile seed), the scenes, and the 185-ray list every scene is
traced with."""
from __future__ import annotations

import ctypes as C
import functools
import re
import subprocess
import tempfile
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
REPO = HERE.parent
N_RAYS = 185            # x 8, 3, 24 spp: no multiple of 64 paths, the last chunk is ragged (64 spp: a chunk each)
SPPS = (8, 64, 3, 24)   # fused; fused, one entry per chunk; staged left to right; staged in blocks of 8
FRAME = 5
assert all((N_RAYS * s) % 64 for s in SPPS if s != 64)


@functools.lru_cache(maxsize=None)
def ref_lib() -> C.CDLL:
    """tests/rays_ref.c (which includes oracle/mm_oracle.c), compiled once per process with the oracle
    Makefile's CFLAGS."""
    mk = (REPO / "oracle" / "Makefile").read_text()
    cflags = re.search(r"^CFLAGS\s*:=\s*(.*)$", mk, flags=re.M).group(1).split()
    so = Path(tempfile.mkdtemp(prefix="rays_ref")) / "librays_ref.so"
    subprocess.run(["gcc", *cflags, "-Wno-unused-function", "-shared", "-o", str(so), str(HERE / "rays_ref.c"), "-lm"],
                   check=True)
    L = C.CDLL(str(so))
    P = C.c_void_p
    L.raysref_trace.argtypes = [P, P, C.c_int, P, C.c_uint64, P, P, P]
    L.raysref_resolve.argtypes = [P, C.c_uint64, C.c_uint32, P, P]
    L.raysref_dir.argtypes = [P, C.c_uint32, C.c_uint32, C.c_int, P]
    L.raysref_dir.restype = None
    L.oracle_primary_dir.argtypes = [P, C.c_uint32, C.c_uint32, P]
    L.oracle_primary_dir.restype = None
    return L


class Ref:
    """rays_ref.c on one scene (an oracle.Oracle holds the arrays)."""

    def __init__(self, scene):
        from oracle.oracle import Oracle

        self.L = ref_lib()
        self.o = Oracle(scene.rects, scene.nodes, scene.idx, scene.is_mirror, scene.emission)

    def trace(self, ext, rays, jitter):
        """((n, 4) float32 out, (n,) float32 var, closest-hit queries) of (n, 8) float32 records."""
        rays = np.ascontiguousarray(rays, dtype=np.float32)
        n = rays.shape[0]
        out, var, q = np.zeros((n, 4), np.float32), np.zeros(n, np.float32), C.c_uint64()
        eb = C.create_string_buffer(bytes(ext), len(bytes(ext)))
        rc = self.L.raysref_trace(C.byref(self.o.sc), eb, 1 if jitter else 0, rays.ctypes.data, n, out.ctypes.data,
                                  var.ctypes.data, C.byref(q))
        assert rc == 0, rc
        return out, var, int(q.value)


def start_dir(rec, smp, frame, jitter):
    """The direction sample `smp` of record `rec` starts with, by rays_ref.c."""
    rec = np.ascontiguousarray(rec, dtype=np.float32)
    d = np.zeros(3, np.float32)
    ref_lib().raysref_dir(rec.ctypes.data, smp, frame, 1 if jitter else 0, d.ctypes.data)
    return d


def primary_dirs(uniform, pixels):
    """oracle_primary_dir of each (x, y) of `pixels`: (n, 3) float32."""
    L = ref_lib()
    ub = C.create_string_buffer(bytes(uniform), 56)
    out = np.zeros((len(pixels), 3), np.float32)
    for k, (x, y) in enumerate(np.asarray(pixels).astype(np.int64)):
        L.oracle_primary_dir(ub, int(x), int(y), out[k].ctypes.data)
    return out


def pack(origins, dirs, keys):
    """(n, 8) float32 records on the host: mirror_maze.rays.pack_rays in numpy."""
    o, d = np.asarray(origins, np.float32), np.asarray(dirs, np.float32)
    rays = np.zeros((len(o), 8), np.float32)
    rays[:, 0:3], rays[:, 4:7] = o, d
    rays.view(np.uint32)[:, 3] = np.asarray(keys).astype(np.uint64).astype(np.uint32)
    return rays


def pixel_records(uniform, pixels):
    """The records of mm_api.h's equivalence: (cam.center, y*view_w + x, primary direction) per pixel."""
    px = np.asarray(pixels).astype(np.int64)
    centre = np.float32(list(uniform.cam.center))
    return pack(np.tile(centre, (len(px), 1)), primary_dirs(uniform, px), px[:, 1] * int(uniform.view_w) + px[:, 0])


# ---- scenes ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene(name):
    """(Scene, points inside it (m, 3) float32): "maze" the N=10 maze (cell centres at eye height), "corridor"
    aov_support.corridor() (points along its axis), "soup" the 3000-rect soup (points among the rects)."""
    import aov_support
    from mirror_maze import Scene

    rng = np.random.default_rng(77)
    if name == "maze":
        s = Scene.build(10, 0)
        ij = rng.integers(0, 10, (64, 2))
        pts = np.stack([-50.0 + 10.0 * ij[:, 0] + 5.0 + rng.uniform(-3, 3, 64), rng.uniform(-0.5, 0.5, 64),
                        -50.0 + 10.0 * ij[:, 1] + 5.0 + rng.uniform(-3, 3, 64)], axis=1)
    elif name == "corridor":
        s, _ = aov_support.corridor()
        pts = np.stack([rng.uniform(-0.9, 0.9, 64), rng.uniform(-0.9, 0.9, 64), rng.uniform(1.0, 199.0, 64)], axis=1)
    else:
        from test_gpu_random_scene import random_scene

        s = random_scene(3000, 7, False)
        pts = rng.uniform(-150, 150, (64, 3))
    return s, np.float32(pts)


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def candidates(name, seed=1):
    """(origins, dirs) of 80 rays from the scene's inside points with random unit directions: the pool the
    equal-geometry pairs are picked from."""
    _, pts = scene(name)
    rng = np.random.default_rng(1000 + seed)
    return pts[rng.integers(0, len(pts), 80)], np.float32(_unit(rng, 80))


def ray_list(name, pair_geometry, pair_keys, seed=0):
    """The scene's 185 records and the index sets of their kinds.

    pair_geometry: (7, 2, 3) float32 origins and directions for the equal-geometry pairs, pair_keys: (7, 2)
    their two keys (picked by the caller with the reference alone).  Kinds, in order: 73 rays from inside points with random unit directions; 20 from
    outside the scene's box looking in, 10 looking away; 20 starting exactly on a rect (o + a v + b u in
    float32); 10 directions of length 1e-3, 10 of length 1e3; 10 with one zero component, 10 with two; 1 with
    dz = -0.0f; 7 duplicates of records 0..6 (key included); 7 pairs of equal geometry and different keys."""
    s, pts = scene(name)
    rng = np.random.default_rng(seed)
    corners = np.concatenate([s.rects[:, 0:3], s.rects[:, 0:3] + s.rects[:, 3:6], s.rects[:, 0:3] + s.rects[:, 6:9],
                              s.rects[:, 0:3] + s.rects[:, 3:6] + s.rects[:, 6:9]])
    lo, hi = corners.min(axis=0), corners.max(axis=0)
    mid, half = (lo + hi) / 2, (hi - lo) / 2 + 1.0

    def inside(n):
        return pts[rng.integers(0, len(pts), n)]

    o, d, kind = [], [], {}

    def add(what, origins, dirs):
        kind[what] = np.arange(sum(len(x) for x in o), sum(len(x) for x in o) + len(origins))
        o.append(np.float32(origins))
        d.append(np.float32(dirs))

    add("inside", inside(73), _unit(rng, 73))
    away = _unit(rng, 30)
    far = mid + 3.0 * half * away
    add("outside_in", far[:20], -away[:20] + rng.uniform(-0.1, 0.1, (20, 3)))
    add("outside_away", far[20:], away[20:])
    k = rng.integers(0, s.n_rects, 20)
    a, b = np.float32(rng.uniform(0.1, 0.9, (2, 20, 1)))
    add("on_wall", s.rects[k, 0:3] + a * s.rects[k, 3:6] + b * s.rects[k, 6:9], _unit(rng, 20))
    add("short", inside(10), 1e-3 * _unit(rng, 10))
    add("long", inside(10), 1e3 * _unit(rng, 10))
    one = _unit(rng, 10)
    one[np.arange(10), rng.integers(0, 3, 10)] = 0.0
    add("one_zero", inside(10), one)
    two = np.zeros((10, 3))
    two[np.arange(10), rng.integers(0, 3, 10)] = rng.choice([-1.0, 1.0], 10)
    add("two_zeros", inside(10), two)
    add("minus_zero_z", inside(1), [[0.6, 0.8, -0.0]])
    add("duplicates", o[0][:7], d[0][:7])
    add("pair_a", pair_geometry[:, 0], pair_geometry[:, 1])
    add("pair_b", pair_geometry[:, 0], pair_geometry[:, 1])
    o, d = np.concatenate(o), np.concatenate(d)
    keys = rng.integers(0, 2**32, len(o), dtype=np.uint64)
    keys[:4] = (0, 1, 2**31, 2**32 - 1)
    keys[kind["duplicates"]] = keys[:7]
    keys[kind["pair_a"]], keys[kind["pair_b"]] = pair_keys[:, 0], pair_keys[:, 1]
    assert (keys[kind["pair_a"]] != keys[kind["pair_b"]]).all()
    rays = pack(o, d, keys)
    assert rays.shape == (N_RAYS, 8) and np.signbit(rays[kind["minus_zero_z"][0], 6])
    rays.setflags(write=False)
    return rays, kind
