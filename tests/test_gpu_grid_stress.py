"""The certified grid search on the GPU where its eps argument is thin, against
the reference walk (Oracle.trace_tile, aov_support.Ref): every comparison is on
bits, zero differing elements, no case excluded.  The inputs and what they
reach are tests/grid_stress_support.py's and tests/test_grid_stress.py's (the
input conditions are asserted there, on the reference alone).

  A  bounce rays that start outside the grid box, whose box check GridQuery
     skips (mm_path.h): the walk then starts from a clamped cell
  B  hits on the scene box's faces and grazing bounces off them, 3-D walk
  C  tied crossing times, rays leaving through a vertical box edge, and cells
     entered at the instant the ray leaves the grid (the maze forms skip them)
  D  is test_gpu_aov.py's test_query_rays_bit_exact on soup and lattice"""
from __future__ import annotations

import numpy as np
import pytest

import aov_support as A
import grid_stress_support as S

pytestmark = pytest.mark.gpu

RINGS = {"rings": {S.MM_OPT_DEFER: 32, S.MM_OPT_DEFER_MIN: 0}, "no-rings": {S.MM_OPT_DEFER: 0}}
GRID_GLOBAL = {S.MM_OPT_TRAVERSAL: 11, S.MM_OPT_LDS_NODES: 0}   # "trav11-lds0"
BVH_LI = {S.MM_OPT_TRAVERSAL: 5, S.MM_OPT_LDS_NODES: 1}         # "trav5-lds1"


@pytest.fixture(scope="module")
def ref_lib(tmp_path_factory):
    return A.build_ref(tmp_path_factory.mktemp("aov_ref"))


_CACHE = {}


def _cached(key, fn):
    """A reference value, computed once and shared read-only."""
    if key not in _CACHE:
        v = fn()
        for a in (v.values() if isinstance(v, dict) else v if isinstance(v, tuple) else (v,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CACHE[key] = v
    return _CACHE[key]


def _ref(ref_lib, name):
    return _cached(("ref", name), lambda: A.Ref(ref_lib, S.scene(name)))


def _oracle(name):
    from oracle.oracle import Oracle

    return _cached(("oracle", name), lambda: Oracle.from_scene(S.scene(name)))


def _renderer(name, opts, cell=None):
    """A Renderer with scene `name` uploaded; opts: {option: value} or "reference"."""
    from mirror_maze import MM_PIPE_REFERENCE, Renderer

    r = Renderer(0)
    if opts == "reference":
        r.set_pipeline(MM_PIPE_REFERENCE)
    else:
        for k, v in opts.items():
            r.set_option(k, v)
    if cell is not None:
        r.set_option(S.MM_OPT_GRID_CELL, cell)
    r.upload_scene(S.scene(name))
    return r


def _check_grid(r, name, cell=100):
    """The grid exists and has the cells the CPU conditions were stated on
    (grid_stress_support.grid_of; the mazes' y merged into one cell)."""
    assert r.scene_info(S.MM_INFO_GRID_OK) == 1.0, name
    g = S.walked_grid(name, S.grid_of(S.scene(name), cell))
    got = [int(r.scene_info(k)) for k in (S.MM_INFO_GRID_CELLS_X, S.MM_INFO_GRID_CELLS_Y, S.MM_INFO_GRID_CELLS_Z)]
    assert got == [int(x) for x in g["n"]], (name, cell, got)


def _form(r, name):
    """(walk, cell words) of the uploaded grid: MM_INFO_GRID_FLAT is grid_build.cpp's
    flat_ok, the maze forms (one cell along y follows); FACES: 64-bit cell words."""
    maze = r.scene_info(S.MM_INFO_GRID_FLAT) == 1.0
    assert not maze or r.scene_info(S.MM_INFO_GRID_CELLS_Y) == 1.0, name
    return ("maze" if maze else "3-D", "wide" if r.scene_info(S.MM_INFO_GRID_FACES) == 1.0 else "plain")


def _bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint32)


def _tile_diffs(got, ref):
    return {k: int((_bits(got[k])[0] != _bits(ref[k])).sum()) for k in got}


def _aov(r, u, limit, tile):
    x0, y0, w, h, ys = tile
    return r.trace_aov(u, None, limit, x0=x0, y0=y0, w=w, h=h, y_stride=ys)


def _check_window(r, name, u, x0, y0, tag):
    ref, rst = _cached(("win", name, bytes(u), x0, y0),
                       lambda: _oracle(name).trace_tile(u, S.ext(), x0, y0, 32, 16))
    got, st = r.trace_tile(u, S.ext(), x0, y0, 32, 16, stats=True)
    bad = int((_bits(got) != _bits(ref)).sum())
    assert bad == 0, (tag, x0, y0, bad)
    assert (st.rays, st.paths) == (rst.rays, rst.paths), (tag, x0, y0)


def _check_rays(r, ref, name, key, rays, tag):
    t_ref, k_ref = _cached(("rays", name, key), lambda: ref.query(rays))
    t, k = r.query_rays(rays)
    bad = (_bits(t) != t_ref.view(np.uint32)) | (_bits(k) != k_ref)
    assert not bad.any(), (tag, int(bad.sum()), np.flatnonzero(bad)[:8])


# ---- A ----------------------------------------------------------------------------
@pytest.mark.parametrize("policy", ["auto", "trav11-lds0", "reference", "trav5-lds1"])
@pytest.mark.parametrize("pl,ld", S.A_CASES)
def test_a_aov_chains_from_off_box_origins(gpu, ref_lib, pl, ld, policy):
    """mm_trace_aov through a telephoto camera at 2^ld C: a quarter and more of
    the chains' bounce rays start outside the grid box (up to all of them, and
    up to four cells outside), unchecked (k_trace_aov passes mh != 0 as
    hit_origin).  The grid policies at the three cell sizes; the reference walk
    and BVH form 5 are the control that the scene is well-posed."""
    name = f"crate{pl}"
    u = S.telephoto(pl, ld)
    opts = {"auto": {}, "trav11-lds0": GRID_GLOBAL, "reference": "reference", "trav5-lds1": BVH_LI}[policy]
    for cell in S.CELLS if policy in ("auto", "trav11-lds0") else (None,):
        r = _renderer(name, opts, cell)
        if cell is not None:
            _check_grid(r, name, cell)
            assert _form(r, name)[0] == "3-D"
        for limit in S.A_LIMITS:
            ref = _cached(("tile", name, ld, limit), lambda: _ref(ref_lib, name).tile(u, limit, *S.A_TILE))
            d = _tile_diffs(_aov(r, u, limit, S.A_TILE), ref)
            assert not any(d.values()), (name, ld, policy, cell, limit, d)
        r.sync()
        r.close()


@pytest.mark.parametrize("rings", sorted(RINGS))
def test_a_telephoto_windows_of_the_path_kernel(gpu, rings):
    """mm_trace_tile at 8 spp, 8 / 8 bounces through the telephoto camera at
    2^12 C from placement 1, tail rings on and off: 50 to 80 bounce rays per
    window start outside the grid box (test_grid_stress.py says why no window
    holds a quarter).  Pixels and (rays, paths) against the oracle."""
    pl, ld = S.A_WINDOW_CASE
    name = f"crate{pl}"
    u = S.telephoto(pl, ld)
    for cell in S.CELLS:
        r = _renderer(name, RINGS[rings], cell)
        _check_grid(r, name, cell)
        for (x0, y0) in S.A_WINDOWS:
            _check_window(r, name, u, x0, y0, (rings, cell))
        r.sync()
        r.close()


# ---- B ----------------------------------------------------------------------------
@pytest.mark.parametrize("pl", S.PLACEMENTS)
def test_b_box_face_hits_and_grazing_bounces(gpu, ref_lib, pl):
    """Cameras 2^-3 of a cell from the -x mirror looking along it, in the three
    placements and at the three cell sizes: two windows of mm_trace_tile and one
    tile of mm_trace_aov each, and 4096 + 37 rays that start on a face rect
    within 2^-10 rad of it, on a box edge or corner, or on a face and exactly
    within it; and 4096 rays aimed at the lines where two rects cross in
    cell-boundary planes (two hits an ulp apart on either side of a boundary)."""
    name = f"crate{pl}"
    ref = _ref(ref_lib, name)
    for cell in S.CELLS:
        r = _renderer(name, {}, cell)
        _check_grid(r, name, cell)
        assert _form(r, name)[0] == "3-D"
        for which in (0, 1):
            u = S.grazing(pl, which)
            for (x0, y0) in S.B_WINDOWS:
                _check_window(r, name, u, x0, y0, (pl, cell, which))
            tile = _cached(("btile", name, which), lambda: ref.tile(u, 15, *S.B_TILE))
            d = _tile_diffs(_aov(r, u, 15, S.B_TILE), tile)
            assert not any(d.values()), (pl, cell, which, d)
        _check_rays(r, ref, name, "b", S.b_rays(pl), (pl, cell))
        _check_rays(r, ref, name, "j", S.j_rays(pl), (pl, cell, "junctions"))
        r.sync()
        r.close()


# ---- C ----------------------------------------------------------------------------
@pytest.mark.parametrize("policy", ["auto", "reference"])
@pytest.mark.parametrize("name", S.C_SCENES)
def test_c_tied_crossing_times(gpu, ref_lib, name, policy):
    """4096 rays with |d.x| == |d.z|: from cell corners and with equal offsets
    (tx == tz on every step), out through a vertical box edge, and into a cell
    at the instant of leaving the grid."""
    r = _renderer(name, {} if policy == "auto" else "reference")
    _check_grid(r, name)
    assert _form(r, name)[0] == ("maze" if name.startswith("maze") else "3-D")
    _check_rays(r, _ref(ref_lib, name), name, "c", S.c_rays(name), (name, policy))
    r.sync()
    r.close()


# ---- forms ------------------------------------------------------------------------
def test_every_grid_form_runs_the_tied_rays_and_a_window(gpu, ref_lib):
    """The 3-D walk and the maze form, each with wide (64-bit, per-face ranges)
    and plain cell words: case C's rays through mm_query_rays and one window
    through mm_trace_tile (the LDS placements) on each, and the set of forms
    seen is all four."""
    from mirror_maze import default_uniform

    seen = set()
    for name, wide in [("crate1", 1), ("crate1", 0), ("maze10", 1), ("maze10", 0), ("maze64", 1), ("soup", 0)]:
        r = _renderer(name, {S.MM_OPT_GRID_WIDE: wide})
        assert r.scene_info(S.MM_INFO_GRID_OK) == 1.0
        seen.add(_form(r, name))
        if name in S.C_SCENES:
            _check_rays(r, _ref(ref_lib, name), name, "c", S.c_rays(name), (name, wide))
        u = S.grazing(1, 0) if name == "crate1" else default_uniform(*S.VIEW, 0)
        _check_window(r, name, u, 40, 30, (name, wide))
        r.sync()
        r.close()
    assert seen == {("3-D", "wide"), ("3-D", "plain"), ("maze", "wide"), ("maze", "plain")}, seen
