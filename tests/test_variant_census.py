"""CPU side of the variant census (tests/variant_census_support.py): the launch policy plans the variant each
case names, the table covers every cell the build holds, nothing the policy reaches on the maze ladder and the
soups is missing from it, and the ringed cases' windows keep paths alive long enough to be parked.  No GPU: the
plan harness (tests/launch_plan/launch_plan_test.cpp) is the library's own mm_plan.cpp, grid_build.cpp and
scene.cpp under a main(), and mm_variant_built is host code."""
from __future__ import annotations

import pytest

import variant_census_support as vc
from variant_census_support import CASES, MM_OPT_DEFER, MM_OPT_GRID_WIDE, MM_OPT_LDS_NODES, RINGS, UNREACHED


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    """plan(scene key, options, entry, w, h) -> the harness's JSON, answered once per distinct question."""
    tmp = tmp_path_factory.mktemp("variant_census")
    exe = vc.build_harness(tmp)
    seen = {}

    def run(key, opts, entry="tile", w=32, h=16):
        q = (key, tuple(sorted(opts.items())), entry, w, h)
        if q not in seen:
            seen[q] = vc.plan(exe, key, opts, tmp, entry, w, h)
        return seen[q]

    run.tmp = tmp
    return run


def test_rect_file_input_under_sanitizers(harness, tmp_path):
    """The harness's rect-file path (a soup under its own BVH) built with the address and undefined-behaviour
    sanitizers answers as the plain build does."""
    exe = vc.build_harness(tmp_path, "sanitized")
    for key, opts in ((vc.FINE, {vc.MM_OPT_GRID_CELL: 200}), (vc.LATTICE, {})):
        assert vc.plan(exe, key, opts, tmp_path) == harness(key, opts)


def test_variant_built_matches_the_instance_lists():
    """mm_variant_built: 20 (mode, form) pairs, 17 of them with ring kinds 1 and 2; nothing outside the lists."""
    from mirror_maze import lib

    cells = vc.built_cells()
    assert len({(m, f) for m, f, _ in cells}) == 20
    assert len({(m, f) for m, f, r in cells if r == 2}) == 17
    assert {(m, f) for m, f, r in cells if r == 1} == {(m, f) for m, f, r in cells if r == 2}
    assert {(m, f) for m, f, r in cells if r == 0} - {(m, f) for m, f, r in cells if r == 2} == {(0, 5), (1, 5), (3, 5)}
    fn = lib().mm_variant_built
    for m, f, r in ((11, 17, 3), (11, 17, -1), (2, 5, 0), (11, 16, 0), (14, 11, 0), (3, 5, 1), (12, 13, 0), (-1, -1, 0)):
        assert fn(m, f, r) == 0, (m, f, r)


@pytest.mark.parametrize("case", CASES, ids=vc.case_id)
def test_planned_variant(harness, case):
    """The policy, given the case's scene, options and call shape, chooses the case's (mode, form) -- and its
    ring kind: grid_lds_cap decides it for the static-grid placements 11 / 14; for the dynamic placements the
    harness is given the static LDS figures of variant_census_support.STATIC_LDS."""
    _, _, w, h = vc.window(case)
    tile_like = case.entry in ("tile", "frames", "cameras")
    j = harness(case.scene, case.opts, case.entry if tile_like else "tile", w, h)
    mode, form, ring = vc.planned(j)
    assert (mode, form) == case.expect[:2], (j["facts"], j["placement"])
    if tile_like:
        assert ring == case.expect[2], (j["facts"], j["plan"])
        assert j["plan"]["defer"] == (ring != 0)
    else:  # a list launch never runs the rings (plan_pixels)
        assert case.expect[2] == 0 and not vc.forced(case)
    # the ring kind follows the staged bytes as the table's comments say
    if vc.forced(case):
        staged = j["placement"]["staged"]
        if mode in vc.STATIC_GRID_MODES:
            want = 2 if staged <= vc.GRID_CAP[2] else 1 if staged <= vc.GRID_CAP[1] else 0
        else:
            want = next((k for k in (2, 1) if staged + vc.STATIC_LDS[k] <= vc.LDS_PER_BLOCK), 0)
        assert case.expect[2] == want, (staged, case.expect)


def test_table_is_complete():
    """Built cells == cells the table expects + UNREACHED, and per built pair the entry kinds the issue names."""
    built = vc.built_cells()
    expected = {c.expect for c in CASES}
    assert expected.isdisjoint(UNREACHED), expected & set(UNREACHED)
    assert expected | set(UNREACHED) == built, (sorted(built - expected - set(UNREACHED)),
                                                sorted((expected | set(UNREACHED)) - built))
    assert all(r != 0 for _, _, r in UNREACHED) and all(why for why in UNREACHED.values())
    pairs = {(m, f) for m, f, _ in built}
    for pair in sorted(pairs):
        ring0 = [c for c in CASES if c.expect == (*pair, 0) and not vc.forced(c)]
        for entry in ("tile", "cameras", "pixels", "pixel_lists"):
            assert any(c.entry == entry for c in ring0), (pair, entry)
        assert any(c.stats for c in ring0), pair
        if (*pair, 2) in built:  # a deferral pair
            assert any(c.entry == "cameras" and c.expect[:2] == pair and c.expect[2] != 0 for c in CASES), pair
    assert len({vc.case_id(c) for c in CASES}) == len(CASES)
    assert all(c.entry in vc.ENTRIES for c in CASES)
    assert all(c.scene[0] != "maze" or c.scene[1] <= vc.GPU_MAZE_MAX for c in CASES)


SWEEP_OPTIONS = {"default": {}, "lds=0": {MM_OPT_LDS_NODES: 0}, "grid_wide=0": {MM_OPT_GRID_WIDE: 0}, "rings": RINGS}


def _soup_sites():
    """The table's soups with the grid options their cases upload them with."""
    sites = {(c.scene, tuple(sorted((k, v) for k, v in c.opts.items() if k == vc.MM_OPT_GRID_CELL)))
             for c in CASES if c.scene[0] == "soup"}
    return sorted(sites)


def test_reachability_sweep(harness):
    """Every (mode, form) the policy reaches on the maze ladder and the table's soups -- under default options,
    MM_OPT_LDS_NODES 0, MM_OPT_GRID_WIDE 0 and forced deferral -- and for the static-grid placements every
    ring kind, is a cell of the table; and no UNREACHED cell is reached (dynamic placements: with the
    STATIC_LDS figures)."""
    expected = {c.expect for c in CASES}
    sites = [(vc.maze(n), ()) for n in vc.MAZE_LADDER] + _soup_sites()
    reached = set()
    for key, grid_opts in sites:
        for name, opts in SWEEP_OPTIONS.items():
            j = harness(key, {**dict(grid_opts), **opts}, "cameras" if name == "rings" else "tile", 64, 32)
            mode, form, ring = vc.planned(j)
            assert (mode, form) in {e[:2] for e in expected}, (key, name, mode, form)
            if mode in vc.STATIC_GRID_MODES:
                assert (mode, form, ring) in expected, (key, name, mode, form, ring)
            assert (mode, form, ring) not in UNREACHED, (key, name)
            assert (ring != 0) <= (MM_OPT_DEFER in opts)
            reached.add((mode, form, ring))
    # the ladder's rows: (mode, form) of the auto plan, ring kind when deferral is forced
    for n, want in ((32, (11, 17, 2)), (36, (11, 17, 1)), (40, (11, 17, 1)), (44, (11, 17, 0)), (48, (14, 15, 2)),
                    (56, (14, 15, 1)), (64, (14, 15, 1)), (72, (12, 15, 2)), (80, (12, 15, 1)), (96, (12, 15, 1)),
                    (112, (12, 11, 1)), (128, (12, 11, 1)), (160, (12, 11, 1)), (200, (12, 11, 0))):
        assert vc.planned(harness(vc.maze(n), RINGS, "cameras", 64, 32)) == want, n
    assert len(reached) >= 30, sorted(reached)


RINGED = sorted({(c.scene, cam, frame, vc.window(c)) for c in CASES if c.expect[2] != 0 for cam, frame in vc.frames_of(c)})


@pytest.mark.parametrize("key,cam,frame,win", RINGED,
                         ids=[f"{vc.scene_id(k)}-cam{c}-frame{f}" for k, c, f, _ in RINGED])
def test_ringed_windows_keep_paths_alive(key, cam, frame, win):
    """A ringed case proves something only where paths live long enough to be parked: by the oracle alone, each
    frame of each ringed case traces at least 3 rays per path on its window (C3 itself: about 8)."""
    ref, rays, paths = vc.reference(key, cam, frame, *win)
    assert paths == win[2] * win[3] * vc.SPP
    assert rays >= vc.MIN_RAYS_PER_PATH * paths, (rays / paths)
    assert ref[..., :3].mean() > 0.0
