"""Shared by tests/test_guard_edges.py (CPU: what the inputs reach, and the CPU
twin against the walk) and tests/test_gpu_guard_edges.py (GPU against the walk):
rays and cameras at and beyond the per-ray guards of the fast paths
(mm_trace.h ray_fast_ok / ray_fast_ok_boxed: every |d| component in
[2^-40, 2^40], every |o| component 0 or in [2^-30, 2^60]).  A ray outside them
must take IEEE division in the reference-order walk; its RN(1/d) from
rcp_guarded is then inf, NaN or a flushed value and must never be read.

Everything here is tuned on the reference walk alone (tests/aov_ref.c)."""
from __future__ import annotations

import math

import numpy as np

import aov_support as A
import grid_stress_support as S

F32 = np.float32
DIR_LO, DIR_HI, ORG_LO = 2.0 ** -40, 2.0 ** 40, 2.0 ** -30
SCENES = ("crate1", "crate2", "maze10", "soup")
SIZES = (1, 63, 8192)
N_CLASSES = 8
VIEW = S.VIEW            # 96 x 64
WINDOW = (32, 24)        # the 32 x 16 trace_tile window: the middle of the view
CAMERA_SCENES = ("crate1", "maze10")
LIMITS = (2, 15, 200)
# The corridor chain: the row of pixels whose camera-space y is exactly 0 (py = 32 of 64)
CORRIDOR_TILE = (14, 32, 67, 1, 1)

# |d| components at and below the guard's lower edge: 2^-40 passes, as does its upper neighbour; the rest fail
TINY_DIRS = [F32(2.0 ** -40), np.nextafter(F32(2.0 ** -40), F32(0)), np.nextafter(F32(2.0 ** -40), F32(1)),
             F32(2.0 ** -41), F32(2.0 ** -45), F32(2.0 ** -100), F32(2.0 ** -126), F32(1e-40), F32(1.4e-45), F32(0.0)]
# |o| components at and below the origin guard's lower edge: 2^-30 and 0 pass
TINY_ORGS = [F32(2.0 ** -30), np.nextafter(F32(2.0 ** -30), F32(0)), F32(2.0 ** -31), F32(2.0 ** -35), F32(1e-40),
             F32(0.0)]
NON_FINITE = [F32(np.nan), F32(np.inf), F32(-np.inf)]


def box(scene):
    """(lo, hi) of every rect corner."""
    c = S.corners(scene.rects)
    return c.min(axis=(0, 1)), c.max(axis=(0, 1))


def _signed(rng, v):
    """v with either sign (-0.0 for v = 0)."""
    return F32(-v) if rng.random() < 0.5 else F32(v)


def edge_rays(scene, n, seed):
    """((n, 2, 4) float32 rays, (n,) class): eight classes in turn (i % 8).
    Origins are uniform in the scene's corner box and directions unit vectors
    unless the class says otherwise.
      0  one direction component replaced, with either sign, by one of
         TINY_DIRS: 2^-40, its two neighbours, 2^-41, 2^-45, 2^-100, 2^-126,
         two denormals, 0 (so -0.0 occurs)
      1  two direction components replaced from the same list, opposite signs
      2  the direction scaled by 2^u, u uniform in [-46, -36]
      3  the direction scaled by 2^u, u uniform in [36, 44]
      4  one origin component replaced, with either sign, by one of TINY_ORGS
      5  class 4's origin and class 0's direction
      6  one component of o or d set to NaN, +inf or -inf
      7  one origin component +-2^u, u uniform in [58, 64], the direction aimed
         back at a point of the box and normalised: one component +-1, the
         others near 2^-55"""
    rng = np.random.default_rng(seed)
    lo, hi = box(scene)
    rays = np.zeros((n, 2, 4), F32)
    rays[:, :, 3] = rng.normal(size=(n, 2))  # the w components are ignored
    cls = np.arange(n) % N_CLASSES
    for i in range(n):
        o = rng.uniform(lo, hi).astype(F32)
        d = rng.normal(size=3)
        d = (d / np.linalg.norm(d)).astype(F32)
        k = int(cls[i])
        if k in (0, 5):
            d[int(rng.integers(3))] = _signed(rng, TINY_DIRS[int(rng.integers(len(TINY_DIRS)))])
        if k == 1:
            a, b = rng.choice(3, size=2, replace=False)
            sg = F32(rng.choice([-1.0, 1.0]))
            d[a] = sg * TINY_DIRS[int(rng.integers(len(TINY_DIRS)))]
            d[b] = -sg * TINY_DIRS[int(rng.integers(len(TINY_DIRS)))]
        if k == 2:
            d = (d.astype(np.float64) * 2.0 ** rng.uniform(-46, -36)).astype(F32)
        if k == 3:
            d = (d.astype(np.float64) * 2.0 ** rng.uniform(36, 44)).astype(F32)
        if k in (4, 5):
            o[int(rng.integers(3))] = _signed(rng, TINY_ORGS[int(rng.integers(len(TINY_ORGS)))])
        if k == 6:
            (o if rng.random() < 0.5 else d)[int(rng.integers(3))] = NON_FINITE[int(rng.integers(3))]
        if k == 7:
            a = int(rng.integers(3))
            o64 = o.astype(np.float64)
            o64[a] = float(rng.choice([-1.0, 1.0])) * 2.0 ** rng.uniform(58, 64)
            o = o64.astype(F32)
            aim = rng.uniform(lo, hi) - o.astype(np.float64)
            d = (aim / np.linalg.norm(aim)).astype(F32)
        rays[i, 0, :3], rays[i, 1, :3] = o, d
    return rays, cls


_RAYS = {}


def rays_of(name, n):
    """edge_rays of scene `name`, made once (read-only)."""
    if (name, n) not in _RAYS:
        rays, cls = edge_rays(S.scene(name), n, seed=700 + n)
        rays.setflags(write=False)
        cls.setflags(write=False)
        _RAYS[(name, n)] = (rays, cls)
    return _RAYS[(name, n)]


def dir_outside(d):
    """Which (n, 3) directions have a component outside [2^-40, 2^40] (NaN counts)."""
    a = np.abs(np.asarray(d, dtype=np.float64))
    return ~((a >= DIR_LO) & (a <= DIR_HI)).all(axis=-1)


def org_below(o):
    """Which (n, 3) origins have a nonzero component below 2^-30."""
    a = np.abs(np.asarray(o, dtype=np.float64))
    return ((a > 0) & (a < ORG_LO)).any(axis=-1)


def centre_of(name):
    """A camera centre inside scene `name`, off its lattice."""
    if name == "crate1":
        return np.array([1.3, 2.1, 0.7])
    lo, hi = box(S.scene(name))
    return (lo + hi) / 2 + np.array([0.13, 0.0, 0.21])


def _uniform(centre, focal, quat, vw, vh):
    return A.uniform_of(F32([*centre, focal, *quat, vw, vh]), *VIEW)


def edge_cameras(name):
    """{camera name: mm_uniform at a 96 x 64 view} for scene `name`.
      tiny-focal     focal 2^-45, identity quaternion, viewport 1.6 x 1.2: a
                     primary has |d.z| = 2^-45 / |p| (below 2^-40 but for the
                     nine pixels around the view axis), and trace_tile's
                     jitter leaves z alone
      tiny-viewport  viewport 2^-44 on both axes, focal 1: |d.x|, |d.y| <= 2^-45
      huge-focal     focal 2^45: primary_dir's rsq gets 2^90 (rsq_ieee)
      tiny-centre    centre (2^-35, -1e-40, -0.0), looking along (0.3, 0.1, 1)
    For the corridor (aov_support.corridor), its camera's centre and viewport
    with focal 2^-45, and the row py = 32 (CORRIDOR_TILE), whose camera-space y
    is exactly 0, so that d.y = 0 through every reflection:
      corridor-tiny-focal  its yaw (aov_support.make_corridor's 1.45) with
                     pitch 0: the pixel on the view axis, px = 48, has p =
                     (0, 0, 2^-45) -- rsq_ieee again -- and zigzags down the
                     corridor between the two mirrors past 200 mirror hits
      corridor-across      the identity quaternion: the camera's x axis, where
                     every tiny-focal primary points, is the mirrors' normal;
                     d = (+-1, 0, 2^-45 / |x|) crosses from mirror to mirror
                     without advancing, a tiny nonzero d.z in every one of the
                     200 queries of each chain."""
    ident = [0.0, 0.0, 0.0, 1.0]
    if name == "corridor":
        _, u = A.corridor()
        c, vp = list(u.cam.center), list(u.cam.viewport)
        yaw = 1.45
        return {"corridor-tiny-focal": _uniform(c, 2.0 ** -45, [0.0, math.sin(yaw / 2), 0.0, math.cos(yaw / 2)], *vp),
                "corridor-across": _uniform(c, 2.0 ** -45, ident, *vp)}
    c = centre_of(name)
    return {
        "tiny-focal": _uniform(c, 2.0 ** -45, ident, 1.6, 1.2),
        "tiny-viewport": _uniform(c, 1.0, ident, 2.0 ** -44, 2.0 ** -44),
        "huge-focal": _uniform(c, 2.0 ** 45, ident, 1.6, 1.2),
        "tiny-centre": _uniform([2.0 ** -35, -1e-40, -0.0], 1.0, S.look_quat([0.3, 0.1, 1.0]), 1.6, 1.2),
    }


def cam10(u):
    """The (10,) float32 camera record of a uniform."""
    return np.frombuffer(bytes(u.cam), dtype=F32).copy()


def scaled(scene, factor):
    """`scene` with every rect coordinate times `factor` (a power of two), its
    BVH rebuilt by Scene.bvh."""
    from mirror_maze import Scene

    rects = scene.rects.copy()
    rects[:, 0:9] *= F32(factor)
    nodes, idx = Scene.bvh(rects)
    return Scene(0, rects, nodes, idx, scene.is_mirror, scene.emission, np.zeros((0, 0), np.uint8), 0)


assert math.isclose(float(TINY_DIRS[0]), DIR_LO) and float(TINY_DIRS[1]) < DIR_LO < float(TINY_DIRS[2])
