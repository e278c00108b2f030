"""The maze forms of the certified grid search on the GPU, on scenes that take each side of the host
build's decisions (tests/grid_forms_support.py; tests/test_grid_forms.py asserts the branches and the rays'
input conditions on the CPU): every comparison is on bits against the reference walk (aov_support.Ref,
Oracle.trace_tile), zero differing elements, no case excluded.  The form that ran is read from the
MM_INFO_GRID_* keys of the uploaded scene, which must equal the host program's facts for the same rects."""
from __future__ import annotations

import numpy as np
import pytest

import aov_support as A
import grid_forms_support as G
from test_gpu_aov import TILES

pytestmark = pytest.mark.gpu

POLICIES = {"auto": {}, "trav11-lds0": {G.MM_OPT_TRAVERSAL: 11, G.MM_OPT_LDS_NODES: 0},
            "trav7-lds1": {G.MM_OPT_TRAVERSAL: 7, G.MM_OPT_LDS_NODES: 1}, "reference": "reference"}
RINGS = {"fused": {}, "rings": {G.MM_OPT_DEFER: 32, G.MM_OPT_DEFER_MIN: 0}}
LEAN = {name: "n_slow_min" not in G.FACTS[name] for name in G.SCENES}  # (tilted has a SLOW record)
AOV_SCENES = ("base", "shelf4", "twin_floor", "classes64", "classes65", "dense_cells")
WINDOW_SCENES = ("base", "classes64", "dense_cells", "twin_floor", "tilted")
LIMITS = (2, 15, 200)


@pytest.fixture(scope="module")
def ref_lib(tmp_path_factory):
    return A.build_ref(tmp_path_factory.mktemp("aov_ref"))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("grid_forms_host")
    exe = G.build_host(tmp)
    return lambda name: G.host_facts(exe, name, tmp)


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
    return _cached(("ref", name), lambda: A.Ref(ref_lib, G.scene(name)[0]))


def _oracle(name):
    from oracle.oracle import Oracle

    return _cached(("oracle", name), lambda: Oracle.from_scene(G.scene(name)[0]))


def _renderer(name, opts):
    """A Renderer with scene `name` uploaded at its MM_OPT_GRID_CELL; opts: {option: value} or "reference"."""
    from mirror_maze import MM_PIPE_REFERENCE, Renderer

    r = Renderer(0)
    if opts == "reference":
        r.set_pipeline(MM_PIPE_REFERENCE)
    else:
        for k, v in opts.items():
            r.set_option(k, v)
    if name in G.CELL:
        r.set_option(G.MM_OPT_GRID_CELL, G.CELL[name])
    r.upload_scene(G.scene(name)[0])
    return r


def _info(r):
    """The uploaded grid's facts, under the host program's names."""
    i = lambda k: int(r.scene_info(k))  # noqa: E731
    return {"ok": i(G.MM_INFO_GRID_OK), "cells": [i(G.MM_INFO_GRID_CELLS_X), i(G.MM_INFO_GRID_CELLS_Y), i(G.MM_INFO_GRID_CELLS_Z)],
            "n_glob": i(G.MM_INFO_GRID_GLOBAL), "wide": i(G.MM_INFO_GRID_FACES), "flat_ok": i(G.MM_INFO_GRID_FLAT),
            "slab": i(G.MM_INFO_GRID_SLAB), "n_class": i(G.MM_INFO_GRID_CLASSES)}


def _check_form(r, name):
    """The form the scene was made for is the one uploaded (FACTS, on the info keys)."""
    f = _info(r)
    G.check_facts(name, f)
    assert int(r.scene_info(G.MM_INFO_LEAN)) == int(LEAN[name]), name
    return f


def _bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint32)


def _check_rays(r, ref, ref_name, key, rays, tag):
    t_ref, k_ref = _cached(("rays", ref_name, key), lambda: ref.query(rays))
    t, k = r.query_rays(np.array(rays))  # (a copy: the shared rays are read-only)
    bad = (_bits(t) != t_ref.view(np.uint32)) | (_bits(k) != k_ref)
    assert not bad.any(), (tag, key, int(bad.sum()), np.flatnonzero(bad)[:8])
    return t_ref, k_ref


def _family(name, family, ref_lib):
    return G.rays(name, family, _ref(ref_lib, name))[0]


def _check_window(r, name, u, x0, y0, frame, tag):
    from mirror_maze import make_ext

    e = make_ext(8, 8, 8, frame=frame)
    ref, rst = _cached(("win", name, bytes(u), x0, y0, frame), lambda: _oracle(name).trace_tile(u, e, x0, y0, 32, 16))
    got, st = r.trace_tile(u, e, x0, y0, 32, 16, stats=True)
    bad = int((_bits(got) != _bits(ref)).sum())
    assert bad == 0, (tag, x0, y0, frame, bad)
    assert (st.rays, st.paths) == (rst.rays, rst.paths), (tag, x0, y0, frame)


# ---- upload facts -------------------------------------------------------------------
@pytest.mark.parametrize("name", G.SCENES)
def test_uploaded_grid_is_the_host_programs(gpu, host, name):
    """Cells, global rects, cell words, maze form, slab pair and classes of the uploaded scene equal the
    host program's for the same rects: test_grid_forms.py's conditions describe the grid the GPU walks."""
    r = _renderer(name, {})
    f = _check_form(r, name)
    h = host(name)
    assert f == {k: h[k] for k in f}, (name, f, h)
    r.close()


# ---- query rays -----------------------------------------------------------------------
@pytest.mark.parametrize("policy", sorted(POLICIES))
@pytest.mark.parametrize("name", G.SCENES)
def test_query_rays_bit_exact(gpu, ref_lib, name, policy):
    """The three ray families -- edges and corners of the rects from both sides of every folded threshold,
    origins on and around the slab planes, and the eight general kinds -- under every query policy the
    scene allows; under auto a traced window shows that the grid search is what ran."""
    from mirror_maze import MMError, _lib

    r = _renderer(name, POLICIES[policy])
    _check_form(r, name)
    if policy == "trav7-lds1" and not LEAN[name]:
        with pytest.raises(MMError) as e:
            r.query_rays(np.array(_family(name, "slab", ref_lib)))
        assert e.value.code == _lib.MM_ERR_UNSUPPORTED
        r.close()
        return
    ref = _ref(ref_lib, name)
    for family in G.FAMILIES:
        _check_rays(r, ref, name, family, _family(name, family, ref_lib), (name, policy))
    if policy == "auto":
        _check_window(r, name, G.cameras(G.WINDOW_VIEW)["inside"], *G.WINDOWS[0], 1, (name, policy))
        assert r.scene_info(G.MM_INFO_LAST_FORM) == 11.0
    r.sync()
    r.close()


# ---- AOV chains ------------------------------------------------------------------------
@pytest.mark.parametrize("name", AOV_SCENES)
def test_aov_chains_bit_exact(gpu, ref_lib, name):
    """mm_trace_aov at mirror limits 2, 15 and 200 on test_gpu_aov.py's three ragged tiles, from a camera in
    a room looking along a mirror and from one above the gallery looking down into it."""
    r = _renderer(name, {})
    _check_form(r, name)
    ref = _ref(ref_lib, name)
    seen = set()
    for cam, u in G.cameras().items():
        for tile in TILES:
            x0, y0, w, h, ys = tile
            for limit in LIMITS:
                want = _cached(("tile", name, cam, tile, limit), lambda: ref.tile(u, limit, x0, y0, w, h, ys))
                got = r.trace_aov(u, None, limit, x0=x0, y0=y0, w=w, h=h, y_stride=ys)
                d = {k: int((_bits(got[k])[0] != _bits(want[k])).sum()) for k in got}
                assert not any(d.values()), (name, cam, tile, limit, d)
                seen |= {int(x) for x in np.unique(np.minimum(want["id"] >> 30, 3))}
    assert 1 in seen, seen  # surfaces were compared
    r.sync()
    r.close()


# ---- path windows -----------------------------------------------------------------------
@pytest.mark.parametrize("rings", sorted(RINGS))
@pytest.mark.parametrize("name", WINDOW_SCENES)
def test_path_windows_bit_exact(gpu, name, rings):
    """mm_trace_tile at 8 spp, 8 / 8 bounces, two frames, with the fused resolve and with the tail rings
    forced on: pixels and (rays, paths) against the oracle."""
    from mirror_maze import MM_INFO_LAST_DEFER

    r = _renderer(name, RINGS[rings])
    _check_form(r, name)
    u = G.cameras(G.WINDOW_VIEW)["inside"]
    for frame in (1, 2):
        for (x0, y0) in G.WINDOWS:
            _check_window(r, name, u, x0, y0, frame, (name, rings))
    assert r.scene_info(G.MM_INFO_LAST_FORM) == 11.0
    assert r.scene_info(MM_INFO_LAST_DEFER) == (1.0 if rings == "rings" else 0.0)
    r.sync()
    r.close()


# ---- transitions ------------------------------------------------------------------------
def _pair(ref_lib, a, b, key, flipped):
    """Scenes a and b on the same rays (a's three families) and the same window, each against its own
    reference; the info key `key` flips 1 -> 0 from a to b.  Returns the two references' ray answers."""
    rays = np.concatenate([_family(a, f, ref_lib) for f in G.FAMILIES])
    u = G.cameras(G.WINDOW_VIEW)["inside"]
    answers, facts = [], []
    for name in (a, b):
        r = _renderer(name, {})
        facts.append(_check_form(r, name))
        answers.append(_check_rays(r, _ref(ref_lib, name), name, ("pair", a), rays, (a, b, name)))
        _check_window(r, name, u, *G.WINDOWS[1], 1, (a, b, name))
        assert r.scene_info(G.MM_INFO_LAST_FORM) == 11.0
        r.sync()
        r.close()
    assert (facts[0][key], facts[1][key]) == (1, 0), facts
    for k in flipped:
        assert facts[0][k] == facts[1][k], (k, facts)
    return rays, answers


def test_one_class_more_leaves_the_maze_forms(gpu, ref_lib):
    """classes64 (64 threshold classes: the maze forms) against classes65 (one wall shorter, 65 classes: the
    3-D walk with 32-byte records): only rays that touch that wall may answer differently."""
    rays, ((t0, k0), (t1, k1)) = _pair(ref_lib, "classes64", "classes65", "flat_ok", ("wide", "slab", "n_glob", "cells"))
    a, b = G.build_rects("classes64")[0], G.build_rects("classes65")[0]
    wall, = np.flatnonzero((a != b).any(axis=1))
    differ = (t0.view(np.uint32) != t1.view(np.uint32)) | (k0 != k1)
    assert differ.any() and ((k0[differ] == wall) | (k1[differ] == wall)).all(), (int(differ.sum()), wall)


def test_long_lists_leave_the_face_ranges(gpu, ref_lib):
    """base (face ranges) against dense_cells (the same rects in cells with lists of more than 7 entries:
    plain cell words), both maze forms: the same answers for every ray."""
    rays, ((t0, k0), (t1, k1)) = _pair(ref_lib, "base", "dense_cells", "wide", ("flat_ok", "slab", "n_glob", "n_class"))
    assert np.array_equal(t0.view(np.uint32), t1.view(np.uint32)) and np.array_equal(k0, k1)
