"""Shared by tests/test_aov.py and tests/test_gpu_aov.py: the CPU reference of
mm_query_rays / mm_trace_aov (tests/aov_ref.c over the oracle) and the
corridor scene (tests/golden/aov_corridor.npz)."""
from __future__ import annotations

import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
REPO = HERE.parent
CORRIDOR = HERE / "golden" / "aov_corridor.npz"
MISS, FAILED, SURFACE, MIRROR_END, RECT = 0xFFFFFFFF, 0xFFFFFFFE, 1 << 30, 2 << 30, 0x00FFFFFF


def build_ref(tmp_dir, twin: bool = False) -> C.CDLL:
    """Compile tests/aov_ref.c (which includes oracle/mm_oracle.c) into tmp_dir
    with the oracle Makefile's CFLAGS and bind it.  twin: the build over
    oracle/grid_cpu.c -- the same entry points answered by the CPU twin of the
    certified grid search (class Twin)."""
    mk = (REPO / "oracle" / "Makefile").read_text()
    cflags = re.search(r"^CFLAGS\s*:=\s*(.*)$", mk, flags=re.M).group(1).split()
    so = Path(tmp_dir) / ("libaov_twin.so" if twin else "libaov_ref.so")
    subprocess.run(["gcc", *cflags, *(["-DAOVREF_TWIN"] if twin else []), "-Wno-unused-function", "-shared", "-o",
                    str(so), str(HERE / "aov_ref.c"), "-lm"], check=True)
    L = C.CDLL(str(so))
    P = C.c_void_p
    L.aovref_walk_ties.argtypes = [P, C.c_int, P, C.c_uint64, P, P, P]
    L.aovref_walk_ties.restype = None
    L.oracle_trace_tile.argtypes = [P, P, P] + [C.c_uint32] * 5 + [P, P]
    if twin:
        L.gridcpu_build.argtypes = [P]
        L.gridcpu_stats.argtypes = [P, C.c_int]
        L.gridcpu_stats.restype = None
    else:
        L.aovref_record.argtypes = [P, C.c_uint64]
        L.aovref_record.restype = C.c_uint64
    L.aovref_query.argtypes = [P, P, P, P, P]
    L.aovref_query_batch.argtypes = [P, P, C.c_uint64, P]
    L.aovref_pixel.argtypes = [P, P, C.c_uint32, C.c_uint32, C.c_uint32, P, P, P]
    L.aovref_tile.argtypes = [P, P] + [C.c_uint32] * 6 + [P, P, P]
    return L


class Ref:
    """aov_ref.c on one scene (an oracle.Oracle holds the arrays)."""

    def __init__(self, L, scene):
        from oracle.oracle import Oracle

        self.L = L
        self.o = Oracle(scene.rects, scene.nodes, scene.idx, scene.is_mirror, scene.emission)

    def query(self, rays):
        """(t, k) of (n, 2, 4) float32 rays."""
        rays = np.ascontiguousarray(rays, dtype=np.float32)
        n = rays.shape[0]
        hits = np.zeros((n, 2), dtype=np.uint32)
        assert self.L.aovref_query_batch(C.byref(self.o.sc), rays.ctypes.data, n, hits.ctypes.data) == 0
        return hits[:, 0].copy().view(np.float32), hits[:, 1].copy()

    def query_one(self, o, d):
        o, d = np.float32(o), np.float32(d)
        t, k = C.c_float(), C.c_uint32()
        assert self.L.aovref_query(C.byref(self.o.sc), o.ctypes.data, d.ctypes.data, C.byref(t), C.byref(k)) == 0
        return t.value, k.value

    def pixel(self, uniform, px, py, mirror_limit):
        nd, al, i = np.zeros(4, np.float32), np.zeros(4, np.float32), C.c_uint32()
        ub = C.create_string_buffer(bytes(uniform), 56)
        assert self.L.aovref_pixel(C.byref(self.o.sc), ub, px, py, mirror_limit, nd.ctypes.data, al.ctypes.data,
                                   C.byref(i)) == 0
        return nd, al, i.value

    def tile(self, uniform, mirror_limit, x0, y0, w, h, y_stride=1):
        """dict of (h, w, 4) float32 normal_depth / albedo and (h, w) uint32 id."""
        nd, al = np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32)
        ids = np.zeros((h, w), np.uint32)
        ub = C.create_string_buffer(bytes(uniform), 56)
        assert self.L.aovref_tile(C.byref(self.o.sc), ub, mirror_limit, x0, y0, w, h, y_stride, nd.ctypes.data,
                                  al.ctypes.data, ids.ctypes.data) == 0
        return {"normal_depth": nd, "albedo": al, "id": ids}

    def trace_tile(self, uniform, ext, x0, y0, w, h, y_stride=1):
        """oracle_trace_tile of this library: ((h, w, 4) float32, Stats)."""
        from oracle.oracle import Stats

        out, st = np.zeros((h, w, 4), np.float32), Stats()
        ub, eb = C.create_string_buffer(bytes(uniform), 56), C.create_string_buffer(bytes(ext), len(bytes(ext)))
        assert self.L.oracle_trace_tile(C.byref(self.o.sc), ub, eb, x0, y0, w, h, y_stride, out.ctypes.data,
                                        C.byref(st)) == 0
        return out, st

    def recorded(self, fn, cap=1 << 20):
        """(fn()'s result, the queries the reference walk answered meanwhile):
        an (n, 8) float32 array of (o.xyz, t, d.xyz, bits of k), in order; a
        path's first query starts at the camera, every later one at the
        float32 ori + t * dir of the one before."""
        rec = np.zeros((cap, 8), np.float32)
        self.L.aovref_record(rec.ctypes.data, cap)
        try:
            res = fn()
        finally:
            n = self.L.aovref_record(None, 0)
        assert n <= cap, (n, cap)
        return res, rec[:n].copy()

    def walk_ties(self, grid, flat, rays, best):
        """aovref_walk_ties: dict of the walk restatement's counts (aov_ref.c)."""
        g = np.float32(list(grid["mn"]) + list(grid["cell"]) + [float(x) for x in grid["n"]] + list(grid["mx"]))
        rays = np.ascontiguousarray(rays, dtype=np.float32)
        best = np.ascontiguousarray(best, dtype=np.float32)
        out = (C.c_uint64 * 5)()
        flags = np.zeros(rays.shape[0], np.uint8)
        self.L.aovref_walk_ties(g.ctypes.data, 1 if flat else 0, rays.ctypes.data, rays.shape[0], best.ctypes.data, out,
                                flags.ctypes.data)
        w = dict(zip(("tied_steps", "ended_at_tend", "entered_at_exit", "walked", "steps"), [int(x) for x in out]))
        w["flags"] = flags  # per ray: 1 a tied step, 2 ended at tend / left the grid, 4 entered a cell at the exit
        return w


class Twin(Ref):
    """The same entry points over oracle/grid_cpu.c (build_ref(twin=True)): the
    CPU twin of the certified grid search, with its walk fallback.  The
    library keeps one grid: making a Twin builds its scene's and zeroes the
    counts, so a Twin is used up before the next one is made."""

    def __init__(self, L, scene):
        super().__init__(L, scene)
        assert L.gridcpu_build(C.byref(self.o.sc)) == 0

    def stats(self, reset=False):
        """Queries since the build or the last reset: {"grid", "fallback", "other_scene"}."""
        out = (C.c_uint64 * 3)()
        self.L.gridcpu_stats(out, 1 if reset else 0)
        return {"grid": out[0], "fallback": out[1], "other_scene": out[2]}


def corridor():
    """(Scene, mm_uniform of its 67x48 camera): two parallel mirrors facing each
    other along z, a matte floor, a matte wall at the far end, the near end and
    the top open (tests/golden/aov_corridor.npz; its BVH is Scene.bvh's)."""
    from mirror_maze import Scene

    z = np.load(CORRIDOR)
    s = Scene(0, z["rects"], np.ascontiguousarray(z["nodes"]), z["idx"], z["is_mirror"], z["emission"],
              np.zeros((0, 0), np.uint8), 0)
    return s, uniform_of(z["camera"], 67, 48)


def make_corridor():
    """The arrays of tests/golden/aov_corridor.npz (tuned on aov_ref.c alone until
    test_aov.py's input conditions held): a corridor 2 wide, 2 high and 200 long;
    the camera near its open end, turned 1.45 rad towards the x = +1 mirror, so
    its rays zigzag down the corridor."""
    import math

    from mirror_maze import Scene

    lz, hm = 200.0, 2.0
    rects = np.float32([
        [-1, -hm / 2, 0, 0, hm, 0, 0, 0, lz, 0.9, 0.9, 0.95],   # mirror x = -1, normal +x (inwards)
        [1, -hm / 2, 0, 0, 0, lz, 0, hm, 0, 0.95, 0.9, 0.9],    # mirror x = +1, normal -x (inwards)
        [-1, hm / 2, 0, 2, 0, 0, 0, 0, lz, 0.6, 0.5, 0.4],      # floor y = +1 (y points down the image)
        [-1, -hm / 2, lz, 2, 0, 0, 0, hm, 0, 0.3, 0.6, 0.8],    # far end wall z = 200
    ])
    is_mirror = np.uint8([1, 1, 0, 0])
    emission = np.float32([[1, 1, 1, 0], [1, 1, 1, 0], [1, 1, 1, 0], [1.0, 0.8, 0.3, 2.0]])
    nodes, idx = Scene.bvh(rects)
    yaw, pitch = 1.45, 0.02
    ax, aw = math.sin(pitch / 2), math.cos(pitch / 2)  # q = q_yaw(y) * q_pitch(x), (x, y, z, w)
    by, bw = math.sin(yaw / 2), math.cos(yaw / 2)
    quat = [bw * ax, by * aw, -by * ax, bw * aw]
    camera = np.float32([0.2, 0.0, 3.0, 1.0, *quat, 2.0 * 67 / 48, 2.0])
    return {"rects": rects, "nodes": nodes, "idx": idx, "is_mirror": is_mirror, "emission": emission,
            "camera": camera}


def uniform_of(cam10, view_w, view_h):
    """mm_uniform with the (10,) float32 camera record cam10."""
    from mirror_maze import _lib

    u = _lib.mm_uniform()
    C.memmove(C.byref(u), np.ascontiguousarray(cam10, dtype=np.float32).ctypes.data, 40)
    u.view_w, u.view_h, u.chunk_w, u.time = float(view_w), float(view_h), 4, 0
    return u


def kinds(ids):
    """(miss, surface, mirror_end) boolean masks of an id buffer."""
    ids = np.asarray(ids).view(np.uint32)
    return ids == MISS, (ids != MISS) & (ids >> 30 == 1), (ids != MISS) & (ids != FAILED) & (ids >> 30 == 2)
