"""The certified grid search where its eps argument is thin, host side (no GPU).

tests/test_gpu_grid_stress.py compares the GPU with the reference walk on the
inputs of tests/grid_stress_support.py; a green result there is void if the
inputs never reach the condition they were made for.  This file states each
condition on the reference walk alone (tests/aov_ref.c: the walk records its
queries, and a float32 restatement of the cell walk's crossing times), and runs
the same inputs through the CPU twin of the search (oracle/grid_cpu.c) against
the walk, bit for bit.

The twin always checks its box (grid_cpu.c grid_search), so for case A it says
nothing about the check the GPU skips for bounce rays (mm_path.h GridQuery):
a bounce origin outside the box is a fallback there.  Only the GPU tests see
the clamped start cell."""
from __future__ import annotations

import numpy as np
import pytest

import aov_support as A
import grid_stress_support as S


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


def _share(st):
    n = st["grid"] + st["fallback"]
    assert st["other_scene"] == 0 and n > 0, st
    return st["grid"] / n


# ---- the scenes -------------------------------------------------------------------
def test_crate_has_a_rect_on_every_box_face_and_a_lattice_inside():
    for pl in S.PLACEMENTS:
        s = S.scene(f"crate{pl}")
        c = S.corners(s.rects)                        # (4, n, 3)
        lo, hi = c.min(axis=(0, 1)), c.max(axis=(0, 1))
        assert len(s.rects) == 50 and list(s.is_mirror[:2]) == [1, 1] and not s.is_mirror[2:].any()
        assert s.emission[2, 3] > 0 and not s.emission[3:, 3].any()
        for f, (axis, side) in enumerate([(0, -1), (0, 1), (1, -1), (1, 1), (2, -1), (2, 1)]):
            assert (c[:, f, axis] == (hi if side > 0 else lo)[axis]).all(), (pl, f)  # the face rect lies in the box face
        # the two mirrors face each other: normals (cross(v, u)) +x on the -x face, -x on the +x face
        n0, n1 = (np.cross(s.rects[k, 3:6].astype(np.float64), s.rects[k, 6:9].astype(np.float64)) for k in (0, 1))
        assert n0[0] > 0 and n1[0] < 0
        # the +x face rect covers half of its face: the opening
        assert np.prod(np.ptp(c[:, 1], axis=0)[1:]) * 2 == np.prod((hi - lo)[1:])
        inner = c[:, 6:]
        touching = ((inner == lo) | (inner == hi)).any(axis=(0, 2)).sum()
        assert touching >= 8, touching                # several touch a face
        # several continue a neighbour in its plane: same plane, one shared edge
        shared = 0
        for i in range(6, 46):
            for j in range(i + 1, 46):  # (the last four are the junctions)
                pts_i, pts_j = {tuple(p) for p in c[:, i]}, {tuple(p) for p in c[:, j]}
                flat_i = np.flatnonzero(np.ptp(c[:, i], axis=0) == 0)
                flat_j = np.flatnonzero(np.ptp(c[:, j], axis=0) == 0)
                if len(pts_i & pts_j) == 2 and list(flat_i) == list(flat_j) and c[0, i, flat_i[0]] == c[0, j, flat_j[0]]:
                    shared += 1
        assert shared >= 6, shared
        assert S.grid_of(s)["C"] / (hi - lo).max() == {1: 0.5, 2: 0.5, 3: 64.0}[pl]


def test_cell_sweep_puts_the_lattice_on_and_off_the_cell_boundaries():
    """MM_OPT_GRID_CELL 100: 16 cells of 8 + eps / 8, every lattice plane within
    eps of a cell boundary; 130 and 70: 12 and 23 cells, most planes well inside
    a cell."""
    s = S.scene("crate1")
    planes = np.arange(-56.0, 57.0, S.PITCH)
    for pct, n, on in zip(S.CELLS, (16, 12, 23), (True, False, False)):
        g = S.grid_of(s, pct)
        assert list(g["n"]) == [n] * 3
        b = float(g["mn"][0]) + np.arange(n + 1) * float(g["cell"][0])
        dist = np.abs(planes[:, None] - b[None, :]).min(axis=1)
        assert (dist <= g["eps"]).all() if on else (dist > 0.5).sum() >= len(planes) // 2, (pct, dist)


# ---- case A -----------------------------------------------------------------------
@pytest.mark.parametrize("pl,ld", S.A_CASES)
def test_case_a_a_quarter_of_the_bounce_origins_lie_outside_the_box(ref_lib, pl, ld):
    """Per compared tile (each mirror limit): of the float32 ori + t * dir the
    reference chain continues from, at least one quarter lie outside the grid
    box (the rect corners widened by eps, restated from grid_build.cpp).  At
    2^20 C (placement 1) some lie more than half a cell outside the box of the
    finest grid the GPU test sweeps (MM_OPT_GRID_CELL 70: cells of 5.6; the hit
    points are 4 apart, cells of 8 would need two steps); at 2^16 C (placement
    3) some do at every cell size."""
    s = S.scene(f"crate{pl}")
    ref = A.Ref(ref_lib, s)
    u = S.telephoto(pl, ld)
    centre = list(u.cam.center)
    x0, y0, w, h, ys = S.A_TILE
    for limit in S.A_LIMITS:
        t, rec = ref.recorded(lambda: ref.tile(u, limit, x0, y0, w, h, ys))
        starts = rec[S.bounce_starts(rec, centre), 0:3]
        shares = {}
        for pct in S.CELLS:
            g = S.grid_of(s, pct)
            out = S.outside(g, starts)
            far = S.outside(g, starts, 0.5 * float(g["cell"].min()))
            shares[pct] = (int(out.sum()), len(starts), int(far.sum()))
            assert len(starts) >= 20 and out.mean() >= 0.25, (pl, ld, limit, pct, shares)
        print(f"case A crate{pl} D=2^{ld}C limit {limit}: outside, bounce origins, > half a cell outside:", shares)
        if ld == 20:
            assert shares[70][2] > 0, shares
        if ld == 16:
            assert all(v[2] > 0 for v in shares.values()), shares
        kinds = A.kinds(t["id"])
        assert kinds[0].any() and kinds[1].any()  # misses and surfaces are both compared


def test_case_a_telephoto_windows_of_trace_tile_hold_some_off_box_origins(ref_lib):
    """trace_tile jitters every primary direction by up to 0.001, two crate
    widths at 2^12 C from placement 1 and far more at every other distance, so
    a telephoto window's samples land all over the crate's surroundings: at
    2^12 C about one path in eight hits the crate, at 2^16 C one in 4000, beyond
    none, and from placement 3 (C = 8192) none at any distance.  Placement 1's
    faces lie on the hit points' float grid (telephoto's docstring), so the
    share of off-box origins stays below one quarter there, and the paths that
    enter the crate add seven accurate origins each.  The windows are therefore
    no part of case A's condition; they are compared on the GPU because they are
    the only way the path kernels see an off-box origin at all, and this states
    what they hold: some in every window."""
    pl, ld = S.A_WINDOW_CASE
    s = S.scene(f"crate{pl}")
    ref, g = A.Ref(ref_lib, s), S.grid_of(s)
    u = S.telephoto(pl, ld)
    for (x0, y0) in S.A_WINDOWS:
        (_, st), rec = ref.recorded(lambda: ref.trace_tile(u, S.ext(), x0, y0, 32, 16))
        b = S.bounce_starts(rec, list(u.cam.center))
        out = S.outside(g, rec[b, 0:3])
        print(f"telephoto window {x0},{y0}: {st.rays} rays, {int(b.sum())} bounce origins, {int(out.sum())} outside")
        assert st.rays == len(rec) and b.sum() >= 400 and out.sum() >= 20


# ---- case B -----------------------------------------------------------------------
def _b_records(ref, pl):
    recs = []
    for which in (0, 1):
        u = S.grazing(pl, which)
        c = list(u.cam.center)
        for (x0, y0) in S.B_WINDOWS:
            _, rec = ref.recorded(lambda: ref.trace_tile(u, S.ext(), x0, y0, 32, 16))
            recs.append((rec, c))
        x0, y0, w, h, ys = S.B_TILE
        _, rec = ref.recorded(lambda: ref.tile(u, 15, x0, y0, w, h, ys))
        recs.append((rec, c))
    return recs


@pytest.mark.parametrize("pl", S.PLACEMENTS)
def test_case_b_face_hits_and_grazing_bounces(ref_lib, pl):
    """At least 500 reference hits land on the crate's face rects, and at least
    200 bounce or mirror-continuation rays start on one with |d . n| < 2^-6."""
    s = S.scene(f"crate{pl}")
    ref = A.Ref(ref_lib, s)
    face = graze = 0
    for rec, c in _b_records(ref, pl):
        face += int(S.on_face_hits(rec).sum())
        graze += int(S.grazing_starts(rec, c).sum())
        assert not S.outside(S.grid_of(s), rec[:, 0:3]).any()  # (these cameras are of order C: case A's effect is absent)
    t, k = ref.query(S.b_rays(pl))
    ray_face = int((k < 6).sum())
    print(f"case B crate{pl}: face hits {face} (cameras) + {ray_face} (rays), grazing starts {graze}")
    assert face >= 500 and ray_face >= 500 and graze >= 200
    per_kind = [int((k[i::3] != A.MISS).sum()) for i in range(3)]
    assert per_kind[0] > 100 and per_kind[1] > 1000 and per_kind[2] == 0, per_kind  # (a ray within a face hits nothing)


@pytest.mark.parametrize("pl", S.PLACEMENTS)
def test_case_b_junction_rays_meet_two_rects_within_rounding_of_their_line(ref_lib, pl):
    """Of 4096 rays aimed at the lines where two rects cross (the first line in
    two cell-boundary planes), at least 2000 hit one of the pair within 1e-4
    (of a 128-wide crate) of the line, and each of the four rects is the
    answer at least 200 times: which of two hits an ulp apart is the closer is
    decided by bits, on both sides of the cell boundary."""
    s = S.scene(f"crate{pl}")
    rays = S.j_rays(pl)
    t, k = A.Ref(ref_lib, s).query(rays)
    sc, c = S.crate_scale(pl), S.crate_centre(pl)
    p = rays[:, 0, :3].astype(np.float64) + t.astype(np.float64)[:, None] * rays[:, 1, :3].astype(np.float64)
    near = np.zeros(len(rays), bool)
    for j, ((ax, a), (bx, b)) in enumerate(S.JUNCTIONS):
        m = np.arange(len(rays)) % len(S.JUNCTIONS) == j
        on_line = (np.abs(p[:, ax] - (c[ax] + a) * sc) < 1e-4 * sc) & (np.abs(p[:, bx] - (c[bx] + b) * sc) < 1e-4 * sc)
        near |= m & on_line & ((k == 46 + 2 * j) | (k == 47 + 2 * j))
    counts = [int((near & (k == r)).sum()) for r in range(46, 50)]
    print(f"case B crate{pl}: junction rays near their line {int(near.sum())}, per rect {counts}")
    assert near.sum() >= 2000 and min(counts) >= 200, (int(near.sum()), counts)
    g = S.grid_of(s)
    if pl in (1, 2):  # x = 0 and z = 0 are boundary 8 of 16, to the last bit
        assert float(g["mn"][0]) + 8 * float(g["cell"][0]) == 0.0 and float(g["mn"][2]) + 8 * float(g["cell"][2]) == 0.0


# ---- case C -----------------------------------------------------------------------
@pytest.mark.parametrize("name", S.C_SCENES)
def test_case_c_tied_crossing_times(ref_lib, name):
    """On the restated walk (aov_ref.c aovref_walk_ties: the two fmas of
    mm_grid.h grid_search in float32): at least 1000 steps with tx == tz, at
    least 100 rays whose last step time equals tend (the 3-D walk: that leave
    the grid), at least a third of the rays hit something -- and at least 16
    rays enter a cell at the very instant they leave the grid, the cell the maze
    forms skip and the 3-D walk tests."""
    s = S.scene(name)
    g = S.c_grid(name)
    rays = S.c_rays(name)
    assert (np.abs(rays[:, 1, 0]) == np.abs(rays[:, 1, 2])).all()
    on_corner = ((rays[0::4, 0, 0] - g["mn"][0]) / g["cell"][0])
    assert np.abs(on_corner - np.round(on_corner)).max() < 1e-5   # kind 0 starts on cell corners: a quarter ...
    off = rays[:, 0, 0] - g["mn"][0] == rays[:, 0, 2] - g["mn"][2]
    assert off[0::4].all() and off[1::4].all()                    # ... and half have equal float32 offsets
    ref = A.Ref(ref_lib, s)
    t, k = ref.query(rays)
    w = ref.walk_ties(g, name.startswith("maze"), rays.reshape(-1, 8), t)
    print(f"case C {name}:", {a: b for a, b in w.items() if a != "flags"}, "hits", int((k != A.MISS).sum()))
    assert w["walked"] == len(rays)
    assert w["tied_steps"] >= 1000 and w["ended_at_tend"] >= 100 and w["entered_at_exit"] >= 16
    assert (k != A.MISS).sum() * 3 >= len(rays)
    assert (k[2::4] == A.MISS).all() and (k[3::4] == A.MISS).all()  # the outbound kinds leave the grid


def test_mazes_and_crate_have_square_grids():
    """Case C needs equal cells and minimum corners in x and z."""
    for name in S.C_SCENES:
        g = S.c_grid(name)
        assert g["mn"][0] == g["mn"][2] and g["cell"][0] == g["cell"][2] and g["n"][0] == g["n"][2], name


# ---- the CPU twin against the walk ---------------------------------------------------
def _d_rays(name, n):
    from test_gpu_aov import _rays

    return _rays(S.scene(name), n, seed=100 + n)


def test_twin_equals_the_walk_on_every_family(ref_lib, twin_lib):
    """The same rays, tiles and windows through oracle/grid_cpu.c (its query
    entry through tests/aov_ref.c's twin build, its windows through
    Oracle.from_scene(s, method="grid")): bit-equal to the walk, and the search
    -- not its fallback -- answers at least half of each case's queries.
    Expected fallbacks, share stated and only asserted below 1: case A (the
    primaries start outside the box, and so do most of the bounce rays: the
    twin checks its box for both).  D's eight ray kinds are taken one by one:
    five of them lie outside the search's domain by construction.
    One grid per library at a time: each case is finished before the next."""
    from oracle.oracle import Oracle

    def same_rays(ref, twin, rays):
        (t0, k0), (t1, k1) = ref.query(rays), twin.query(rays)
        return np.array_equal(_bits(t0), _bits(t1)) and np.array_equal(k0, k1)

    shares = {}
    for pl, ld in S.A_CASES:                                        # A: tiles
        s = S.scene(f"crate{pl}")
        ref, twin = A.Ref(ref_lib, s), A.Twin(twin_lib, s)
        u = S.telephoto(pl, ld)
        for limit in S.A_LIMITS:
            assert _same_tile(ref.tile(u, limit, *S.A_TILE), twin.tile(u, limit, *S.A_TILE)), (pl, ld, limit)
        shares[f"A crate{pl} 2^{ld}"] = _share(twin.stats())
        assert shares[f"A crate{pl} 2^{ld}"] < 1.0
    pl, ld = S.A_WINDOW_CASE                                        # A: windows
    s = S.scene(f"crate{pl}")
    walk, grid = Oracle.from_scene(s), Oracle.from_scene(s, method="grid")
    Oracle.grid_stats(reset=True)
    u = S.telephoto(pl, ld)
    for (x0, y0) in S.A_WINDOWS:
        (a, sa), (b, sb) = walk.trace_tile(u, S.ext(), x0, y0, 32, 16), grid.trace_tile(u, S.ext(), x0, y0, 32, 16)
        assert np.array_equal(_bits(a), _bits(b)) and (sa.rays, sa.paths) == (sb.rays, sb.paths)
    shares["A windows"] = _share(Oracle.grid_stats())
    assert shares["A windows"] < 1.0
    for pl in S.PLACEMENTS:                                         # B
        s = S.scene(f"crate{pl}")
        ref, twin = A.Ref(ref_lib, s), A.Twin(twin_lib, s)
        walk, grid = Oracle.from_scene(s), Oracle.from_scene(s, method="grid")
        Oracle.grid_stats(reset=True)
        for which in (0, 1):
            u = S.grazing(pl, which)
            for (x0, y0) in S.B_WINDOWS:
                (a, sa), (b, sb) = (o.trace_tile(u, S.ext(), x0, y0, 32, 16) for o in (walk, grid))
                assert np.array_equal(_bits(a), _bits(b)) and (sa.rays, sa.paths) == (sb.rays, sb.paths)
            assert _same_tile(ref.tile(u, 15, *S.B_TILE), twin.tile(u, 15, *S.B_TILE)), (pl, which)
        shares[f"B crate{pl} windows"] = _share(Oracle.grid_stats())
        shares[f"B crate{pl} tiles"] = _share(twin.stats(reset=True))
        assert same_rays(ref, twin, S.b_rays(pl)), pl
        shares[f"B crate{pl} rays"] = _share(twin.stats(reset=True))
        assert same_rays(ref, twin, S.j_rays(pl)), pl
        shares[f"B crate{pl} junction rays"] = _share(twin.stats())
        assert min(shares[f"B crate{pl} {x}"] for x in ("windows", "tiles", "rays", "junction rays")) >= 0.5, shares
    for name in S.C_SCENES:                                         # C
        s = S.scene(name)
        ref, twin = A.Ref(ref_lib, s), A.Twin(twin_lib, s)
        assert same_rays(ref, twin, S.c_rays(name)), name
        shares[f"C {name}"] = _share(twin.stats())
        assert shares[f"C {name}"] >= 0.5, shares
    for name in ("soup", "lattice"):                                # D
        s = S.scene(name)
        ref, twin = A.Ref(ref_lib, s), A.Twin(twin_lib, s)
        for n in (1, 63, 64, S.N_RAYS):
            assert same_rays(ref, twin, _d_rays(name, n)), (name, n)
        # Five of the eight kinds are outside the search's domain by construction (origin outside the box: 1, 2;
        # a zero direction component: 4, 5, 7): the walk answers all of them, on the GPU as here.  The half is
        # asked of the three kinds the search can answer.
        rays = _d_rays(name, S.N_RAYS)
        for kind in range(8):
            twin.stats(reset=True)
            twin.query(rays[kind::8])
            shares[f"D {name} kind {kind}"] = _share(twin.stats())
        assert all(shares[f"D {name} kind {k}"] == 0.0 for k in (1, 2, 4, 5, 7)), shares
        assert all(shares[f"D {name} kind {k}"] >= 0.5 for k in (0, 3, 6)), shares
    print("share of queries the twin's search answered:", {k: round(v, 3) for k, v in shares.items()})
