"""The maze forms' grid build on hand-built scenes, host side (no GPU).

grid_build.cpp and rect_compact.cpp decide, per scene, whether the grid takes the maze forms (16-byte
records + the threshold class table, the x / z walk, the slab shortcut, face ranges) and write their data.
The project's own mazes take one side of each decision; tests/grid_forms_support.py's gallery variants take
the other sides.  This file

  * builds every variant with tests/grid_forms/grid_forms_host.cpp (stand-alone, compiled plain and with the
    address and undefined-behaviour sanitizers) and asserts the branch it was made for (FACTS);
  * decodes the image the host program built: list entries, class offsets, and every compact record's
    thresholds, read through the class table, against the same rect's 32-byte record;
  * states, on the reference walk alone (aov_support.Ref), what the three ray families of
    tests/test_gpu_grid_forms.py reach, and prints the figures (pytest -s).
"""
from __future__ import annotations

import numpy as np
import pytest

import aov_support as A
import grid_forms_support as G


@pytest.fixture(scope="module", params=list(G.HOST_BUILDS))
def host(request, tmp_path_factory):
    tmp = tmp_path_factory.mktemp(f"grid_forms_{request.param}")
    exe = G.build_host(tmp, request.param)
    return lambda name, **kw: G.host_facts(exe, name, tmp, **kw)


@pytest.fixture(scope="module")
def host_raw(tmp_path_factory):
    """The plain build, on any rect array."""
    tmp = tmp_path_factory.mktemp("grid_forms_raw")
    exe = G.build_host(tmp)
    return lambda rects, **kw: G.run_host(exe, rects, tmp, **kw)


@pytest.fixture(scope="module")
def ref_lib(tmp_path_factory):
    return A.build_ref(tmp_path_factory.mktemp("aov_ref"))


_REFS = {}


def _ref(ref_lib, name):
    if name not in _REFS:
        _REFS[name] = A.Ref(ref_lib, G.scene(name)[0])
    return _REFS[name]


# ---- build facts ------------------------------------------------------------------
@pytest.mark.parametrize("name", G.SCENES)
def test_every_scene_takes_its_branch(host, name):
    f = host(name)
    print(name, {k: f[k] for k in ("n", "cells", "n_glob", "glob_axes", "slab", "flat_ok", "wide", "n_class", "n_slow",
                                   "longest", "bit63")})
    G.check_facts(name, f)
    assert f["n"] <= 200
    assert f["flat_ok"] == 0 or (f["bit63"] == 0 and 0 < f["n_class"] <= 64)  # the maze walk decodes no whole-list cell
    assert f["flat_ok"] == 1 or f["n_class"] == 0
    if f["slab"]:  # the pair sorted by y, although the floor (the higher y) comes first in the rect array
        assert f["slab_y"] == [G.Y0, G.Y1] and f["glob"] == [1, 0], f
    if name == "classes65":  # one class more than classes64, and nothing else in the way of the maze forms
        assert host("classes64")["n_class"] == 64 and f["n_glob"] == 2 and f["slab"] == 1
    if name == "dense_cells":  # the same rects as base, whose lists fit face ranges at the default cell size
        b = host("base")
        assert (b["wide"], b["flat_ok"]) == (1, 1) and b["longest"] <= 7 and f["cells"][0] < b["cells"][0]


def test_scenes_hold_what_their_names_say():
    rects, mirror, emission, info = G.build_rects("base")
    walls = info["conv"] >= 0
    for axis in (0, 2):  # all eight conventions per wall direction, both normal signs among them
        m = walls & (info["axis"] == axis)
        assert sorted(set(info["conv"][m])) == list(range(8))
        n = np.cross(rects[m, 3:6].astype(np.float64), rects[m, 6:9].astype(np.float64))[:, axis]
        assert (n > 0).any() and (n < 0).any()
    n_walls = len(set(info["wall"][walls]))
    assert 0.2 <= len(set(info["wall"][walls & (mirror == 1)])) / n_walls <= 0.3  # about every fourth wall a mirror
    assert (emission[:, 3] > 0).sum() == 1
    heights = np.abs(rects[walls, 3:9].reshape(-1, 2, 3)[:, :, 1]).max(axis=1)
    assert (heights == G.HEIGHT).any() and (heights == G.WINDOW[0]).any() and (heights == 1.75).any()
    # classes64 and classes65 differ in one wall's length
    a, b = G.build_rects("classes64")[0], G.build_rects("classes65")[0]
    diff = np.flatnonzero((a != b).any(axis=1))
    assert len(diff) == 1 and info["conv"][diff[0]] >= 0 and heights[diff[0] - info["n_planes"]] == G.HEIGHT
    # twin_floor: two coincident y-normal rects
    t = G.build_rects("twin_floor")[0]
    lo, hi = G._extent(t)
    assert (lo[0] == lo[1]).all() and (hi[0] == hi[1]).all() and lo[0, 1] == hi[0, 1] == G.TWIN_Y * G.TWIN_SCALE


# ---- the image ----------------------------------------------------------------------
def _words(image, off, n):
    return np.frombuffer(image, dtype=np.uint32, count=n, offset=off)


@pytest.mark.parametrize("name", G.FLAT)
def test_flat_image_lists_classes_and_thresholds(host, host_raw, name):
    """A flat image's list entries name rect k as 8 k; every record's class lies in the table; and the
    four thresholds a compact record reads through the class table are the folded thresholds of the same
    rect's 32-byte record (after the y_first swap of a z-normal record's in-plane pair) -- a wrong class
    index or a missed swap shows here.  The 32-byte records come from the same rects with one tilted rect
    appended (a SLOW record: no maze form; a rect's record does not depend on the other rects)."""
    f, image = host(name, dump=True)
    n = f["n"]
    assert f["flat_ok"] == 1 and len(image) == f["bytes"]
    entries = np.frombuffer(image, dtype=np.uint16, count=f["n_list"], offset=f["off_list"])
    assert (entries % 8 == 0).all() and (entries // 8 < n).all()
    assert f["off_data"] == f["off_class"] and f["off_recs"] == f["off_class"] + 16 * 64
    rec = _words(image, f["off_recs"], 4 * n).reshape(n, 4)
    meta = rec[:, 3]
    assert ((meta & 0x3F0) < 16 * f["n_class"]).all()
    assert (meta & ~np.uint32(0x3F0 | (3 << 20) | (3 << 30)) == 0).all()
    table = _words(image, f["off_class"], 4 * f["n_class"]).reshape(-1, 4)
    assert len({tuple(r) for r in table}) == f["n_class"]  # no class twice
    assert sorted(set((meta & 0x3F0) >> 4)) == list(range(f["n_class"]))  # and none unused

    rects = G.build_rects(name)[0]
    tilted = np.float32([[G.X0 + 14.0, G.Y0, G.Z0 + 12.0, 0.0, G.HEIGHT, 0.0, 0.5, 0.0, 6.0, 0.5, 0.5, 0.5]])
    g, wide_image = host_raw(np.concatenate([rects, tilted]), cell=G.CELL.get(name, 100), dump=True)
    assert g["flat_ok"] == 0 and g["n_slow"] == 1 and g["off_class"] == 0
    big = _words(wide_image, g["off_recs"], 8 * (n + 1)).reshape(n + 1, 8)[:n]
    assert (big[:, 7] & 0xFFFFF == np.arange(n)).all()
    axis, kind = (big[:, 7] >> 20) & 3, big[:, 7] >> 30
    assert (kind == 0).all() and ((meta >> 20) & 3 == axis).all() and (meta >> 30 == kind).all()
    z = axis == 2
    assert z.any() and (axis == 0).any()
    want_o = np.where(z[:, None], big[:, [0, 2, 1]], big[:, [0, 1, 2]])
    want_t = np.where(z[:, None], big[:, [5, 6, 3, 4]], big[:, [3, 4, 5, 6]])
    assert np.array_equal(rec[:, 0:3], want_o)
    got_t = table[(meta & 0x3F0) >> 4]
    bad = np.flatnonzero((got_t != want_t).any(axis=1))
    assert len(bad) == 0, (name, bad[:8], axis[bad[:8]])
    # both fold signs and both swap values reached the records: thresholds of either sign on either pair
    t = want_t.view(np.float32)
    assert (t[:, 0] < -1).any() and (t[:, 1] > 1).any() and (t[:, 2] < -1).any() and (t[:, 3] > 1).any()


# ---- the rays' input conditions -----------------------------------------------------
@pytest.mark.parametrize("name", G.FLAT)
def test_edge_rays_take_both_sides_of_every_threshold(ref_lib, name):
    """Family 1, per (wall direction, convention) pair and for the y-normal rects: among the rays that
    cross the targeted rect's plane within 4 floats of the targeted edge, the reference answers the
    targeted rect for at least 10 % and something else for at least 10 %."""
    s, info = G.scene(name)
    ref = _ref(ref_lib, name)
    rays, target, e_axis, e_coord, group = G.rays(name, "edge", ref)
    assert len(rays) == G.N_RAYS
    _, k = ref.query(rays)
    near = G.near_edge(rays, s.rects, target, e_axis, e_coord)
    lo, hi = G._extent(s.rects)
    o = rays[:, 0, :3]
    outside = ((o < lo.min(axis=0)) | (o > hi.max(axis=0))).any(axis=1)
    assert outside.sum() >= 200 and (~outside).sum() >= 200, (name, outside.sum())  # both occur in numbers
    for g, (a, c) in enumerate(G.edge_groups(info)):
        m = (group == g) & near
        hit = float((k[m] == target[m]).mean())
        print(f"{name} edge rays, {'xyz'[a]}-normal convention {c}: {int((group == g).sum())} rays, {int(m.sum())} "
              f"within 4 ulp, hit share {hit:.2f}, miss share {1 - hit:.2f}")
        assert m.sum() >= 80, (name, a, c, int(m.sum()))
        assert hit >= 0.10 and 1.0 - hit >= 0.10, (name, a, c, hit)


def test_slab_rays_reach_both_planes_and_pass_them(ref_lib):
    """Family 2 on base: at least 200 reference answers on each plane, at least 200 wall or miss answers
    from origins within one float of a plane, and waves of both kinds: every lane skipping a plane, and not."""
    rays, on_plane = G.rays("base", "slab")
    assert len(rays) == G.N_RAYS
    _, k = _ref(ref_lib, "base").query(rays)
    floor, ceiling, passed = int((k == 0).sum()), int((k == 1).sum()), int(((k >= 2) & on_plane).sum())
    ballots = G.slab_ballots(rays)
    dy = rays[:, 1, 1]
    print(f"slab rays: floor {floor}, ceiling {ceiling}, wall or miss from a plane {passed}; waves with the "
          f"shortcut {int(ballots.sum())} of {len(ballots)}")
    assert floor >= 200 and ceiling >= 200 and passed >= 200
    assert ballots.sum() >= 10 and (~ballots).sum() >= 10
    assert (dy > 0).any() and (dy < 0).any() and (dy == 0).sum() > 50 and (np.abs(dy) == 2.0 ** -20).sum() > 50
    oy = rays[:, 0, 1]
    for plane in (np.float32(G.Y0), np.float32(G.Y1)):
        for y in (plane, np.nextafter(plane, np.float32(np.inf)), np.nextafter(plane, np.float32(-np.inf))):
            assert (oy == y).sum() > 50, (plane, y)


def test_general_rays_tie_on_the_twin_floor(ref_lib):
    """Family 3 on twin_floor: a floor rect is the reference's answer -- a tie of the two coincident
    floors, which the search hands to the fallback walk -- for at least 30 % of the rays.

    The eight ray kinds are test_gpu_aov.py's as they are: two of them (aimed away from the scene; moving
    within a face of the scene box) never meet a plane, nor does a ray with d_y = 0, and half of the
    random directions point away from a single plane, so the share has little room above 0.30.  Measured,
    with the floors at the gallery's bottom: 0.197 (the gallery's own floor size), 0.225 (two thirds of the
    walls removed), 0.231 (walls 0.5 high), 0.249 (floors reaching 60 beyond the gallery), 0.276 (480
    beyond); as a deck at mid height, which rays from outside meet from either side: 0.282 (60 beyond),
    0.298 (160 beyond), and with the scene scaled by 4 (fewer unnormalised rays within a <= 0.1): 0.307,
    which is what the scene keeps (grid_forms_support.PLAZA, TWIN_Y, TWIN_SCALE)."""
    _, info = G.scene("twin_floor")
    rays, = G.rays("twin_floor", "general")
    _, k = _ref(ref_lib, "twin_floor").query(rays)
    share = float((k < info["n_planes"]).mean())
    print(f"twin_floor general rays: floor share {share:.3f}, miss share {float((k == A.MISS).mean()):.3f}")
    assert info["n_planes"] == 2
    assert share >= 0.30, share


@pytest.mark.parametrize("name", G.SCENES)
def test_general_rays_hit_and_miss(ref_lib, name):
    rays, = G.rays(name, "general")
    assert len(rays) == G.N_RAYS
    _, k = _ref(ref_lib, name).query(rays)
    assert (k != A.MISS).sum() > 500 and (k == A.MISS).sum() > 500, name
