"""Shared by tests/test_cert_fast.py (CPU) and tests/test_gpu_cert_fast.py (GPU):
the C twin of the grid search's two certificates (tests/cert_fast_ref.c) and rays
aimed by construction at the band around the edges of a rect's reference leaf
box, where the fast certificate (mm_grid.h) must hand over to the full one.

Everything here is tuned on the twin and the reference walk (tests/aov_ref.c)
alone."""
from __future__ import annotations

import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np

from grid_stress_support import _pack, grid_of, outside

HERE = Path(__file__).resolve().parent
REPO = HERE.parent
MISS = 0xFFFFFFFF
FAST, FULL, NO_CERT = 1, 2, 0x80
MAZE_N = 10
# hit-point offsets from an edge, in floats of the edge coordinate (ulp) and in units of the margin m = 2^-20 C
ULP_STEPS = (0, 1, -1, 2, -2, 3, -3, 4, -4)
M_STEPS = (0.5, -0.5, 1.0, -1.0, 2.0, -2.0)
N_AIMED = 4096 + 37


def build_twin(tmp_dir) -> C.CDLL:
    """Compile tests/cert_fast_ref.c into tmp_dir with the oracle Makefile's CFLAGS and bind it."""
    mk = (REPO / "oracle" / "Makefile").read_text()
    cflags = re.search(r"^CFLAGS\s*:=\s*(.*)$", mk, flags=re.M).group(1).split()
    so = Path(tmp_dir) / "libcert_fast_ref.so"
    subprocess.run(["gcc", *cflags, "-shared", "-o", str(so), str(HERE / "cert_fast_ref.c"), "-lm"], check=True)
    L = C.CDLL(str(so))
    P = C.c_void_p
    L.certfast_scale.argtypes = [P]
    L.certfast_scale.restype = C.c_double
    L.certfast_build.argtypes = [P, P, P, P]
    L.certfast_build.restype = C.c_float
    L.certfast_flags.argtypes = [P, P, C.c_float, P, C.c_uint64, P]
    L.certfast_flags.restype = None
    return L


class Certs:
    """The twin on one scene: per rect its reference leaf's box, its inner window and its FAST normal axis."""

    def __init__(self, L, scene):
        from oracle.oracle import Oracle

        self.L = L
        self.rects = np.asarray(scene.rects, dtype=np.float32)
        self.o = Oracle(scene.rects, scene.nodes, scene.idx, scene.is_mirror, scene.emission)
        n = scene.n_rects
        self.box, self.win = np.zeros((n, 3, 2), np.float32), np.zeros((n, 3, 2), np.float32)
        self.axis = np.zeros(n, np.int32)
        self.C = float(L.certfast_scale(C.byref(self.o.sc)))
        self.omax = float(L.certfast_build(C.byref(self.o.sc), self.box.ctypes.data, self.win.ctypes.data,
                                           self.axis.ctypes.data))
        self.m = float(np.float32(self.C * 2.0 ** -20))

    def flags(self, queries):
        """Per answered query (n, 8) float32 (o.xyz, t, d.xyz, bits of k): FAST | FULL bits, or NO_CERT for a miss."""
        q = np.ascontiguousarray(queries, dtype=np.float32)
        out = np.zeros(len(q), np.uint8)
        self.L.certfast_flags(self.box.ctypes.data, self.win.ctypes.data, C.c_float(self.omax), q.ctypes.data, len(q),
                              out.ctypes.data)
        return out


def sufficient(certs, queries):
    """The condition mm_grid.h's proof derives from a passed fast certificate, evaluated exactly, per answered
    query: on the hit rect's normal axis k its plane lies in its leaf's range, and on both in-plane axes
    RN(B_lo - o) <= a d <= RN(B_hi - o) -- the numerators as the full certificate rounds them (float32), the
    product a d of two float32 exact in float64.  It implies that a lies between the two slab quotients on
    every axis, whatever the quotients' rounding.  False for a miss."""
    q = np.ascontiguousarray(queries, dtype=np.float32)
    k = q[:, 7].copy().view(np.uint32)
    hit = (k != MISS) & (q[:, 3] < np.float32(1e30))
    kk = np.where(hit, k, 0).astype(np.int64)
    ok = hit & (certs.axis[kk] >= 0)
    ak = np.maximum(certs.axis[kk], 0)
    rows = np.arange(len(q))
    plane = certs.rects[kk, ak]
    ok &= (certs.box[kk, ak, 0] <= plane) & (plane <= certs.box[kk, ak, 1])
    ad = q[:, 3:4].astype(np.float64) * q[:, 4:7].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        n_lo = (certs.box[kk, :, 0] - q[:, 0:3]).astype(np.float64)  # float32 subtraction: RN(B_lo - o)
        n_hi = (certs.box[kk, :, 1] - q[:, 0:3]).astype(np.float64)
    inside = (n_lo <= ad) & (ad <= n_hi)
    inside[rows, ak] = True
    return ok & inside.all(axis=1)


def naive_fast(certs, queries):
    """A control: the fast certificate without its margin -- the hit point fma(a, d, o) inside the leaf's box
    itself on the in-plane axes, origin within omax.  Not sound: test_cert_fast.py shows that the aimed rays
    catch it in breach of `sufficient`, i.e. that they would catch a margin that is too small."""
    q = np.ascontiguousarray(queries, dtype=np.float32)
    k = q[:, 7].copy().view(np.uint32)
    hit = (k != MISS) & (q[:, 3] < np.float32(1e30))
    kk = np.where(hit, k, 0).astype(np.int64)
    # (float32 a d + o in float64 is exact up to the final rounding: one fma)
    p = (q[:, 3:4].astype(np.float64) * q[:, 4:7].astype(np.float64) + q[:, 0:3].astype(np.float64)).astype(np.float32)
    inside = (p >= certs.box[kk, :, 0]) & (p <= certs.box[kk, :, 1])
    inside[np.arange(len(q)), np.maximum(certs.axis[kk], 0)] = True
    return hit & (certs.axis[kk] >= 0) & inside.all(axis=1) & (np.abs(q[:, 0:3]).max(axis=1) <= certs.omax)


def guarded(queries):
    """The queries the grid search can be asked (mm_trace.h ray_fast_ok_boxed): |d| in [2^-40, 2^40] on every
    axis, every origin coordinate 0 or at least 2^-30 in magnitude."""
    o, d = np.abs(queries[:, 0:3]), np.abs(queries[:, 4:7])
    return ((d >= 2.0 ** -40) & (d <= 2.0 ** 40)).all(axis=1) & ((o == 0) | (o >= 2.0 ** -30)).all(axis=1)


def answered(rays, t, k):
    """(n, 8) query records (aov_ref.c's layout) of (n, 2, 4) rays and their reference answers."""
    q = np.zeros((len(rays), 8), np.float32)
    q[:, 0:3], q[:, 3], q[:, 4:7] = rays[:, 0, :3], t, rays[:, 1, :3]
    q[:, 7] = np.asarray(k, np.uint32).view(np.float32)
    return q


def _step(x, ulps):
    """float32 x moved by `ulps` floats along the number line (x != 0)."""
    i = np.float32(x).view(np.int32)
    return (i + (ulps if x > 0 else -ulps)).view(np.float32)


def _candidates(scene, certs, g, n, seed):
    """Rays whose hit point lies, by construction, at a chosen offset from an edge (one ray in four: from a
    corner, both in-plane coordinates offset) of a rect with a FAST record: 0, +-1 .. +-4 floats and +-m / 2,
    +-m, +-2 m (m = 2^-20 C, the fast certificate's margin; positive = into the rect), for each of the rect's
    four edges.  The direction's component along the offset axis has magnitude 2^-j, j = 0 .. 40
    (against O(1) along the normal), or is whatever the origin gives when that is on a wall.  Origins, in
    turn: (0) 0.3 to 8 back along the direction; (1) on a wall of the scene (a point of another rect); (2) on a
    face of the grid box g (grid_stress_support.grid_of: one coordinate mn or mx to the float, or one float
    inside) -- the largest |o| grid_ray_ok admits, so the largest a ray of mm_query_rays can bring to the
    certificate; (3) beyond the box, which only a bounce ray can be (mm_path.h): one coordinate at omax = 8 C,
    the largest the fast certificate takes, to the float or one float beyond, or the origin 2^12 C away (a
    telephoto camera's bounce origins are that coarse) -- mm_query_rays answers these with the BVH walk, the C
    twin takes them as they are.  The origin is float32, so the
    computed hit point is the aimed one up to a float or two of C (of the origin, for the far ones).
    Returns (rays (n, 2, 4), target rect, origin kind)."""
    rng = np.random.default_rng(seed)
    rects = np.asarray(scene.rects, dtype=np.float64)
    r9 = rects[:, 0:9]
    corners = np.stack([r9[:, 0:3], r9[:, 0:3] + r9[:, 3:6], r9[:, 0:3] + r9[:, 6:9], r9[:, 0:3] + r9[:, 3:6] + r9[:, 6:9]])
    lo, hi = corners.min(axis=0), corners.max(axis=0)
    fast = np.flatnonzero(certs.axis >= 0)
    offsets = [("ulp", s) for s in ULP_STEPS] + [("m", s) for s in M_STEPS]
    O, D, target, kind = [], [], [], []
    for i in range(n):
        k = int(fast[i % len(fast)]) if i < len(fast) else int(rng.choice(fast))
        ak = int(certs.axis[k])
        inplane = [a for a in range(3) if a != ak]
        e = inplane[int(rng.integers(2))]    # the edge's axis ...
        end = int(rng.integers(2))           # ... and which of its two edges
        other = inplane[0] + inplane[1] - e

        def off_point(axis, which_end, what, s):
            edge = np.float32(hi[k, axis] if which_end else lo[k, axis])
            inward = -1.0 if which_end else 1.0
            if what == "ulp":
                return float(_step(edge, int(s * inward) * (1 if edge > 0 else -1))) if s and edge != 0 else float(edge)
            return float(np.float32(float(edge) + inward * s * certs.m))

        P = np.zeros(3)
        P[ak] = lo[k, ak]
        P[e] = off_point(e, end, *offsets[int(rng.integers(len(offsets)))])
        if rng.random() < 0.25:              # a corner
            P[other] = off_point(other, int(rng.integers(2)), *offsets[int(rng.integers(len(offsets)))])
        else:
            P[other] = np.float32(rng.uniform(lo[k, other], hi[k, other]))
        okind = i % 4
        d = np.zeros(3)
        d[ak] = rng.choice([-1.0, 1.0]) * rng.uniform(0.3, 1.0)
        d[e] = rng.choice([-1.0, 1.0]) * 2.0 ** -int(rng.integers(41))
        d[other] = rng.choice([-1.0, 1.0]) * rng.uniform(0.05, 1.0)
        if okind == 0:
            o = P - rng.uniform(0.3, 8.0) * d
        elif okind == 1:
            w = int(rng.choice(fast))
            o = lo[w] + rng.uniform(0.0, 1.0, 3) * (hi[w] - lo[w])
            if abs(o[ak] - P[ak]) < 0.5:     # (a wall in the target's own plane: step back instead)
                o = P - rng.uniform(0.3, 8.0) * d
            else:
                d = P - np.float32(o).astype(np.float64)
        elif okind == 2 or (okind == 3 and i % 8 < 4):
            ax = (ak, other)[int(rng.integers(2))]  # (an axis the direction is not tiny along)
            if okind == 2:
                up = int(rng.integers(2))
                face = np.float32(g["mx"][ax] if up else g["mn"][ax])
                big = float(face if rng.integers(2) else np.nextafter(face, np.float32(-np.inf if up else np.inf)))
            else:
                big = np.float32(certs.omax)
                big = big if rng.integers(2) else np.nextafter(big, np.float32(np.inf))
                big = float(big) * float(rng.choice([-1.0, 1.0]))
            s = (P[ax] - big) / d[ax]
            if s < 0:                        # (the ray has to run from the origin to the hit point)
                d[ax], s = -d[ax], -s
            o = P - s * d
            o[ax] = big
        else:
            o = P - certs.C * 2.0 ** 12 * d / np.abs(d).max()
        o32 = np.float32(o)
        o32 = np.where(np.abs(o32) < 2.0 ** -30, np.float32(0.0), o32)  # (the guards' origin range)
        if okind in (1, 2, 3):               # re-aim from the rounded origin (then a = 1, or a power of two)
            d = P - o32.astype(np.float64)
            d = d * 2.0 ** -max(0.0, np.ceil(np.log2(np.abs(d).max())))
        d32 = np.float32(d)
        d32 = np.where(np.abs(d32) < 2.0 ** -40, np.copysign(np.float32(2.0 ** -40), d32 + np.float32(0.0)), d32)
        d32 = np.where(d32 == 0, np.float32(2.0 ** -40), d32)
        O.append(o32), D.append(d32), target.append(k), kind.append(okind)
    return _pack(np.array(O), np.array(D), rng), np.array(target), np.array(kind)


def reaches(g, queries):
    """Which query records (o.xyz, t, d.xyz, k) mm_query_rays brings to the grid search, and so to its
    certificate when they hit: inside the guards and with the origin in the grid box (mm_path.h GridQuery)."""
    return guarded(queries) & ~outside(g, queries[:, 0:3])


def aimed_rays(scene, certs, ref, n=N_AIMED, seed=410):
    """n of 4 n candidates (_candidates), an equal number per origin kind: for half of a kind's quota those
    with a clear view -- the reference walk (ref: an aov_support.Ref of the scene) answers the targeted rect --,
    then the others in their order (aimed just outside the rect, or at something in the way).
    Returns (rays, target rect, origin kind, the walk's (t, k))."""
    rays, target, kind = _candidates(scene, certs, grid_of(scene), 4 * n, seed)
    t, k = ref.query(rays)
    keep = []
    for j in range(4):
        quota = n // 4 + (j < n % 4)
        of_kind = np.flatnonzero(kind == j)
        on = of_kind[k[of_kind] == target[of_kind]]
        on = on[: quota // 2]
        keep.append(np.concatenate([on, np.setdiff1d(of_kind, on)])[:quota])
    keep = np.sort(np.concatenate(keep))
    return rays[keep], target[keep], kind[keep], (t[keep], k[keep])


_MAZE = {}


def maze():
    """The N = 10 maze, built once."""
    from mirror_maze import Scene

    if "s" not in _MAZE:
        _MAZE["s"] = Scene.build(MAZE_N, 0)
    return _MAZE["s"]


# ---- bounce rays with coarse origins ----------------------------------------------
TELE_SCENE, TELE_LOG2_D, TELE_VIEW = "floor_only", 12, (96, 64)
TELE_WINDOWS = [(24, 20), (40, 30)]  # 32 x 16 each


def telephoto_gallery():
    """(Scene, mm_uniform): grid_forms_support's gallery without its ceiling (a maze form), seen from
    D = 2^12 C above it by a camera looking down into the rooms through a viewport 1.3 gallery diagonals wide.
    Its hit points ori + t * dir are rounded at ulp(D) = 2^-12 C = 4 eps: the bounce rays, which GridQuery
    takes without the box check (mm_path.h), start from such points."""
    import grid_forms_support as G
    from grid_stress_support import camera

    s = G.scene(TELE_SCENE)[0]
    g = grid_of(s)
    centre = np.array([(G.X0 + G.X1) / 2, G.Y1, (G.Z0 + G.Z1) / 2])
    f = np.array([0.05, 1.0, 0.08])
    f /= np.linalg.norm(f)
    D = 2.0 ** TELE_LOG2_D * g["C"]
    wide = 1.3 * (G.X1 - G.X0) * np.sqrt(2.0) / D
    return s, camera(centre - D * f, f, wide, wide * TELE_VIEW[1] / TELE_VIEW[0], TELE_VIEW)
