"""Rays at and beyond the fast paths' per-ray guards, host side (no GPU).

tests/test_gpu_guard_edges.py compares the GPU with the reference walk on the
inputs of tests/guard_edge_support.py; a green result there is void if the
inputs never reach what they were made for.  This file states on the reference
walk alone (tests/aov_ref.c, which records its queries) that the rays of each
class hit something, that the cameras' queries lie outside the guards, and it
runs the same inputs through the CPU twin of the grid search (oracle/grid_cpu.c)
against the walk, bit for bit."""
from __future__ import annotations

import numpy as np
import pytest

import aov_support as A
import grid_stress_support as S
import guard_edge_support as G


@pytest.fixture(scope="module")
def ref_lib(tmp_path_factory):
    return A.build_ref(tmp_path_factory.mktemp("aov_ref"))


@pytest.fixture(scope="module")
def twin_lib(tmp_path_factory):
    return A.build_ref(tmp_path_factory.mktemp("aov_twin"), twin=True)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_tile(a, b):
    return all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in a)


def _tile_records(ref, u, limit=15, tile=S.B_TILE):
    x0, y0, w, h, ys = tile
    return ref.recorded(lambda: ref.tile(u, limit, x0, y0, w, h, ys))


# ---- the inputs are what their descriptions say ------------------------------------
def test_edge_rays_hold_every_listed_value_with_either_sign():
    rays, cls = G.rays_of("crate1", 8192)
    d0 = rays[cls == 0, 1, :3]
    for v in G.TINY_DIRS:
        for sign in (False, True):
            m = (np.abs(d0) == v) & (np.signbit(d0) == sign)
            assert m.any(), (float(v), sign)  # (v = 0 with the sign bit set: -0.0)
    o4 = rays[cls == 4, 0, :3]
    for v in G.TINY_ORGS:
        for sign in (False, True):
            assert ((np.abs(o4) == v) & (np.signbit(o4) == sign)).any(), (float(v), sign)
    d1 = rays[cls == 1, 1, :3]
    tiny = np.isin(np.abs(d1), np.float32(G.TINY_DIRS))
    assert (tiny.sum(axis=1) >= 2).all()
    n2, n3 = (np.linalg.norm(rays[cls == c, 1, :3].astype(np.float64), axis=1) for c in (2, 3))
    assert n2.min() < 2.0 ** -45 and n2.max() > 2.0 ** -37 and n3.min() < 2.0 ** 37 and n3.max() > 2.0 ** 43
    r6 = rays[cls == 6][:, :, :3].reshape(-1, 6)
    assert ((~np.isfinite(r6)).sum(axis=1) == 1).all()
    assert np.isnan(r6[:, :3]).any() and np.isnan(r6[:, 3:]).any() and np.isposinf(r6).any() and np.isneginf(r6).any()
    o7, d7 = rays[cls == 7, 0, :3].astype(np.float64), rays[cls == 7, 1, :3].astype(np.float64)
    big = np.abs(o7).max(axis=1)
    assert big.min() >= 2.0 ** 58 and big.max() > 2.0 ** 63 and (big > 2.0 ** 60).any() and (big < 2.0 ** 60).any()
    small = np.sort(np.abs(d7), axis=1)
    assert (small[:, 2] == 1.0).all() and small[:, 1].max() < 2.0 ** -50
    # classes 0, 1, 5 and 7 are mostly outside the direction guard, 4 is inside it and outside the origin's
    out = {c: float(G.dir_outside(rays[cls == c, 1, :3]).mean()) for c in range(8)}
    assert min(out[c] for c in (0, 1, 2, 5)) > 0.75 and out[7] == 1.0 and out[4] == 0.0, out
    assert 0.3 < out[3] < 0.7, out  # (the upper edge 2^40 lies inside class 3's range)
    assert G.org_below(o4).mean() > 0.5


@pytest.mark.parametrize("name", G.SCENES)
def test_a_third_of_each_finite_class_hits_and_the_long_and_non_finite_rays_miss(ref_lib, name):
    """At least one third of the rays of each of classes 0, 1, 2, 4, 5 and 7 hit
    a rect on the reference walk.  Classes 3 and 6 return (1e30, MISS) for every
    ray, as a fact about the reference: a direction of length >= 2^36 divides
    every hit distance a = dot(o - ori, n) / dot(d, n) by that length, and the
    scenes are under 2^9 across, so the reference's `a > 0.1f` rejects every
    hit (it rejects every hit of a direction longer than 10 scene diameters);
    a NaN or infinite operand makes a, d1 or d2 NaN or infinite, which fails
    one of the ordered compares of ray_rect_intersect.  Both classes are
    still compared on the GPU: they exercise the guard's upper edge and its
    handling of non-finite values."""
    rays, cls = G.rays_of(name, 8192)
    t, k = A.Ref(ref_lib, S.scene(name)).query(rays)
    share = {c: float((k[cls == c] != A.MISS).mean()) for c in range(G.N_CLASSES)}
    print(f"{name}: share of each class that hits (threshold 1/3 for 0, 1, 2, 4, 5, 7; 0 for 3, 6):",
          {c: round(v, 3) for c, v in share.items()})
    for c in (0, 1, 2, 4, 5, 7):
        assert share[c] >= 1 / 3, (name, c, share)
    for c in (3, 6):
        m = cls == c
        assert (k[m] == A.MISS).all() and (_bits(t[m]) == _bits(np.float32(1e30))).all(), (name, c)


@pytest.mark.parametrize("name", G.CAMERA_SCENES)
def test_cameras_put_every_aov_query_outside_the_guards(ref_lib, name):
    """Over S.B_TILE at mirror limit 15: every reference query of tiny-focal,
    tiny-viewport and huge-focal has a direction component outside
    [2^-40, 2^40]; every query of tiny-centre has a nonzero origin component
    below 2^-30; tiny-focal's tile holds misses and surfaces."""
    ref = A.Ref(ref_lib, S.scene(name))
    cams = G.edge_cameras(name)
    for cn in ("tiny-focal", "tiny-viewport", "huge-focal"):
        t, rec = _tile_records(ref, cams[cn])
        out = int(G.dir_outside(rec[:, 4:7]).sum())
        print(f"{name} {cn}: {out} of {len(rec)} queries outside the direction guard (threshold: all)")
        assert len(rec) >= 335 and out == len(rec), (name, cn)
        if cn == "tiny-focal":
            miss, surf, _ = A.kinds(t["id"])
            print(f"{name} tiny-focal: {int(miss.sum())} misses, {int(surf.sum())} surfaces (threshold: some of both)")
            assert miss.any() and surf.any()
    t, rec = _tile_records(ref, cams["tiny-centre"])
    low = int(G.org_below(rec[:, 0:3]).sum())
    print(f"{name} tiny-centre: {low} of {len(rec)} queries with a nonzero |o| component below 2^-30 (threshold: all)")
    assert len(rec) >= 335 and low == len(rec)
    assert np.signbit(np.float32(list(cams["tiny-centre"].cam.center))[1:]).all()  # -1e-40 and -0.0 are in the record


@pytest.mark.parametrize("name", G.CAMERA_SCENES)
def test_tiny_focal_window_of_the_path_kernel_holds_a_sixth_outside_the_guard(ref_lib, name):
    """trace_tile's jitter adds to x and y only, so every primary of the
    tiny-focal camera keeps its |d.z| = 2^-45 / |p|, below 2^-40 for every
    pixel but the nine around the view axis (|p| < 2^-5), which share their
    waves with the others; the diffuse bounces after it are ordinary."""
    ref = A.Ref(ref_lib, S.scene(name))
    u = G.edge_cameras(name)["tiny-focal"]
    (_, st), rec = ref.recorded(lambda: ref.trace_tile(u, S.ext(), *G.WINDOW, 32, 16))
    out = int(G.dir_outside(rec[:, 4:7]).sum())
    print(f"{name} tiny-focal window: {out} of {len(rec)} queries outside the direction guard (threshold 1/6)")
    assert st.rays == len(rec) and out * 6 >= len(rec)
    first = (rec[:, 0:3] == np.float32(list(u.cam.center))).all(axis=1)
    outside = int(G.dir_outside(rec[first, 4:7]).sum())  # of the 8 spp primaries of every pixel
    assert first.sum() == 32 * 16 * 8 and (32 * 16 - 9) * 8 <= outside < 32 * 16 * 8, outside


def test_corridor_chains_stay_outside_the_guard_to_the_mirror_limit(ref_lib):
    """The corridor's camera with pitch 0 and focal 2^-45, row py = 32 (camera-
    space y exactly 0, so d.y = 0 through every reflection): the pixel on the
    view axis, px = 48, zigzags between the two mirrors to MIRROR_END at limit
    200, and every query of the row -- the first of each pixel and up to 199
    hit-origin continuations -- has a direction outside the guard.  The same
    with the camera turned to face along the corridor (corridor-across): the
    row's rays cross from mirror to mirror with d.y = 0 and, for nine in ten,
    0 < |d.z| < 2^-40, a tiny nonzero component kept through every reflection."""
    s, _ = A.corridor()
    ref = A.Ref(ref_lib, s)
    cams = G.edge_cameras("corridor")
    x0 = G.CORRIDOR_TILE[0]
    for cn, u in cams.items():
        t, rec = _tile_records(ref, u, 200, G.CORRIDOR_TILE)
        _, _, end = A.kinds(t["id"])
        out = int(G.dir_outside(rec[:, 4:7]).sum())
        print(f"{cn}: {int(end.sum())} MIRROR_END pixels, {out} of {len(rec)} queries outside the guard (threshold: all)")
        assert out == len(rec)
        if cn == "corridor-tiny-focal":
            assert end[0, 48 - x0] and t["albedo"][0, 48 - x0, 3] == 199.0 and len(rec) >= 67 + 199
        else:
            assert end.sum() >= 60 and len(rec) >= 60 * 200
            dz = np.abs(rec[:, 6])  # (the pixel on the view axis looks straight down the corridor: one query)
            assert (dz > 0).all() and (dz == 1.0).sum() == 1 and (dz < 2.0 ** -40).mean() > 0.9


# ---- the scaled-up crate ---------------------------------------------------------------
def _one_leaf(s):
    """`s` with its BVH replaced by one leaf holding every rect (the root's box
    is never tested): the walk then is ray_rect_intersect over all rects."""
    from mirror_maze import Scene
    from mirror_maze.scene import NODE_DTYPE

    nodes = np.zeros(1, NODE_DTYPE)
    nodes["count"] = len(s.rects)
    return Scene(0, s.rects, nodes, np.arange(len(s.rects), dtype=np.uint32), s.is_mirror, s.emission, s.grid, 0)


def test_reference_drops_rects_whose_normal_overflows(ref_lib):
    """DESIGN.md §Numerics, "Large rects": ray_rect_intersect normalises
    cross(v, u), and from |v| |u| >= 2^64 on dot(n, n) is inf, its rsqrt 0 and the
    normal 0 (NaN once the cross product itself overflows): nc = 0 or NaN, and
    no ray hits the rect.  crate1's faces are 128 wide, so at scale 2^24 every
    answer is the unit crate's scaled, at 2^25 five of the six faces are gone
    and at 2^26 all six.  Neither Scene.bvh nor the walk is the stage that
    loses them: a BVH of one leaf holding every rect (ray_rect_intersect over
    all of them, no box test at all) answers the same bits at every scale."""
    base = S.scene("crate1")
    rng = np.random.default_rng(3)
    n = 2048
    o = rng.uniform(-60, 60, (n, 3))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    answers = {}
    for e in (0, 24, 25, 26, 30):
        s = G.scaled(base, 2.0 ** e)
        rays = np.zeros((n, 2, 4), np.float32)
        rays[:, 0, :3], rays[:, 1, :3] = np.float32(o) * np.float32(2.0 ** e), d
        t, k = A.Ref(ref_lib, s).query(rays)
        t1, k1 = A.Ref(ref_lib, _one_leaf(s)).query(rays)
        assert np.array_equal(_bits(t), _bits(t1)) and np.array_equal(k, k1), e
        v, u = s.rects[:, 3:6].astype(np.float64), s.rects[:, 6:9].astype(np.float64)
        lost = np.linalg.norm(v, axis=1) * np.linalg.norm(u, axis=1) >= 2.0 ** 64  # (axis-aligned, perpendicular edges)
        answers[e] = (t, k, lost)
        print(f"crate1 x 2^{e}: {int((k != A.MISS).sum())} of {n} rays hit, {int(lost.sum())} rects with dot(n, n) = inf")
        assert not lost[k[k != A.MISS]].any()
    t0, k0, _ = answers[0]
    t24, k24, lost24 = answers[24]
    hit = k0 != A.MISS
    assert not lost24.any() and hit.sum() > 1500
    assert np.array_equal(k24[hit], k0[hit]) and np.array_equal(_bits(t24[hit]), _bits(t0[hit] * np.float32(2.0 ** 24)))
    assert list(np.flatnonzero(answers[25][2])) == [0, 2, 3, 4, 5]  # (face 1 covers half of its face: 2^32 x 2^31)
    assert list(np.flatnonzero(answers[26][2])) == [0, 1, 2, 3, 4, 5]
    assert 0 < (answers[26][1] != A.MISS).sum() < (answers[25][1] != A.MISS).sum() < hit.sum()
    assert answers[30][2].all() and (answers[30][1] == A.MISS).all()


# ---- the CPU twin against the walk ---------------------------------------------------
def test_twin_equals_the_walk_on_rays_tiles_and_windows(ref_lib, twin_lib):
    """Every ray class at the three sizes, every camera's AOV tile at the three
    mirror limits and every camera's path window (Oracle.from_scene(s,
    method="grid")) through oracle/grid_cpu.c: bit-equal to the walk.  The share
    of each class the twin's search (not its fallback) answered is printed and
    nothing is asserted about it: the twin divides in IEEE and applies no
    origin guard, so it answers class 4 from the grid where the GPU must fall
    back, and the upper half of class 3.
    One grid per library at a time: each scene is finished before the next."""
    from oracle.oracle import Oracle

    shares = {}
    for name in G.SCENES:
        s = S.scene(name)
        ref, twin = A.Ref(ref_lib, s), A.Twin(twin_lib, s)
        for n in G.SIZES:
            rays, cls = G.rays_of(name, n)
            t0, k0 = ref.query(rays)
            for c in range(min(n, G.N_CLASSES)):
                twin.stats(reset=True)
                t1, k1 = twin.query(rays[cls == c])
                assert np.array_equal(_bits(t0[cls == c]), _bits(t1)) and np.array_equal(k0[cls == c], k1), (name, n, c)
                if n == G.SIZES[-1]:
                    st = twin.stats()
                    shares[f"{name} class {c}"] = round(st["grid"] / (st["grid"] + st["fallback"]), 3)
        if name in G.CAMERA_SCENES:
            walk, grid = Oracle.from_scene(s), Oracle.from_scene(s, method="grid")
            for cn, u in G.edge_cameras(name).items():
                for limit in G.LIMITS:
                    assert _same_tile(ref.tile(u, limit, *S.B_TILE), twin.tile(u, limit, *S.B_TILE)), (name, cn, limit)
                (a, sa), (b, sb) = (o.trace_tile(u, S.ext(), *G.WINDOW, 32, 16) for o in (walk, grid))
                assert np.array_equal(_bits(a), _bits(b)) and (sa.rays, sa.paths) == (sb.rays, sb.paths), (name, cn)
    s, _ = A.corridor()
    ref, twin = A.Ref(ref_lib, s), A.Twin(twin_lib, s)
    for cn, u in G.edge_cameras("corridor").items():
        assert _same_tile(ref.tile(u, 200, *G.CORRIDOR_TILE), twin.tile(u, 200, *G.CORRIDOR_TILE)), cn
    print("share of each class's rays the twin's search answered:", shares)
