"""Closest-hit answers on the GPU for rays at and beyond the fast paths' per-ray
guards (mm_trace.h ray_fast_ok / ray_fast_ok_boxed), against tests/aov_ref.c:
every comparison is on bits, zero differing elements, no case excluded.  A ray
outside the guards takes IEEE division in the reference-order walk; its
RN(1/d) (make_ray computes rcp_guarded for every ray) is inf, NaN or a flushed
value there, and one read of it in any grid or BVH form shows here as a wrong
cell walk or a wrong slab test.  The inputs are tests/guard_edge_support.py's;
what they reach is asserted on the reference alone in tests/test_guard_edges.py."""
from __future__ import annotations

import numpy as np
import pytest

import aov_support as A
import grid_stress_support as S
import guard_edge_support as G
from test_gpu_aov import POLICIES, _renderer, _unsupported
from test_gpu_grid_stress import RINGS

pytestmark = pytest.mark.gpu

RAY_POLICIES = ("auto", "trav11-lds0", "trav7-lds1", "trav5-lds0", "reference")
NAMES = ("normal_depth", "albedo", "id")
# the path kernels' query forms: the grid search with tail rings on and off, and the BVH loop forms 5 and 7
PATH_FORMS = dict(RINGS)
PATH_FORMS["bvh5"] = {S.MM_OPT_TRAVERSAL: 5, S.MM_OPT_LDS_NODES: 1}
PATH_FORMS["bvh7"] = {S.MM_OPT_TRAVERSAL: 7, S.MM_OPT_LDS_NODES: 1}
MM_INFO_LEAN = 8


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


def _scene(name):
    return A.corridor()[0] if name == "corridor" else S.scene(name)


def _ref(ref_lib, name):
    return _cached(("ref", name), lambda: A.Ref(ref_lib, _scene(name)))


def _bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint32)


def _finite_rays(name, n):
    """The first n rays of classes 0-5 and 7 of a seeded edge_rays set."""
    def make():
        rays, cls = G.edge_rays(S.scene(name), n + n // 7 + 8, seed=900 + n)
        keep = np.flatnonzero(cls != 6)[:n]
        assert len(keep) == n
        return np.ascontiguousarray(rays[keep]), cls[keep].copy()

    return _cached(("finite", name, n), make)


def _check_rays(r, ref_lib, name, key, rays, tag):
    t_ref, k_ref = _cached(("hits", name, key), lambda: _ref(ref_lib, name).query(rays))
    t, k = r.query_rays(np.array(rays))  # (a writable copy: the shared inputs are read-only)
    assert t.shape == (len(rays),) and k.shape == (len(rays),)
    bad = (_bits(t) != t_ref.view(np.uint32)) | (_bits(k) != k_ref)
    assert not bad.any(), (tag, int(bad.sum()), np.flatnonzero(bad)[:8], rays[np.flatnonzero(bad)[:4]])
    return k_ref


def _expect_unsupported(r, call):
    from mirror_maze import MMError, _lib

    with pytest.raises(MMError) as e:
        call()
    assert e.value.code == _lib.MM_ERR_UNSUPPORTED
    r.close()


def _aov(r, u, limit, tile, cameras=None):
    x0, y0, w, h, ys = tile
    return r.trace_aov(u, cameras, limit, x0=x0, y0=y0, w=w, h=h, y_stride=ys)


def _ref_tile(ref_lib, name, u, limit, tile):
    return _cached(("tile", name, bytes(u), limit, tile), lambda: _ref(ref_lib, name).tile(u, limit, *tile))


def _tile_diffs(got, ref, frame=0):
    return {k: int((_bits(got[k])[frame] != _bits(ref[k])).sum()) for k in got}


def _ext(frame):
    from mirror_maze import make_ext

    return make_ext(8, 8, 8, frame=frame)  # (S.ext() is frame 1)


def _ref_window(ref_lib, name, u, frame=1):
    def run():
        out, st = _ref(ref_lib, name).trace_tile(u, _ext(frame), *G.WINDOW, 32, 16)
        return out, (st.rays, st.paths)

    return _cached(("win", name, bytes(u), frame), run)


# ---- rays ---------------------------------------------------------------------------
@pytest.mark.parametrize("policy", RAY_POLICIES)
@pytest.mark.parametrize("name", G.SCENES)
def test_finite_edge_rays_bit_exact(gpu, ref_lib, name, policy):
    """Classes 0-5 and 7 of guard_edge_support.edge_rays: 1, 63 and 8192 rays.
    maze10 runs the flat (maze) grid forms, soup the SLOW records, the crates
    the 3-D walk."""
    s = S.scene(name)
    r = _renderer(s, POLICIES[policy])
    if _unsupported(r, POLICIES[policy]):
        _expect_unsupported(r, lambda: r.query_rays(np.array(_finite_rays(name, 63)[0])))
        return
    for n in G.SIZES:
        rays, cls = _finite_rays(name, n)
        k_ref = _check_rays(r, ref_lib, name, ("finite", n), rays, (name, policy, n))
    assert (k_ref != A.MISS).sum() > 2000 and (k_ref == A.MISS).sum() > 1000  # both answers were compared
    r.sync()
    r.close()


@pytest.mark.parametrize("opts", [{S.MM_OPT_GRID_CELL: 70}, {S.MM_OPT_GRID_CELL: 100}, {S.MM_OPT_GRID_CELL: 130},
                                  {S.MM_OPT_GRID_WIDE: 0}], ids=["cell70", "cell100", "cell130", "plain"])
def test_finite_edge_rays_on_the_crate_at_every_cell_size_and_word_form(gpu, ref_lib, opts):
    """crate1 with the lattice on and off the cell boundaries and with plain
    cell words: the 3-D walk's wide form (MM_OPT_GRID_CELL 100, the default)
    and its plain form (MM_OPT_GRID_WIDE 0; the 23^3 cells of MM_OPT_GRID_CELL 70
    get plain words as well) in front of the same 8192 rays."""
    r = _renderer(S.scene("crate1"), opts)
    assert r.scene_info(S.MM_INFO_GRID_OK) == 1.0 and r.scene_info(S.MM_INFO_GRID_FLAT) == 0.0
    if S.MM_OPT_GRID_WIDE in opts or opts.get(S.MM_OPT_GRID_CELL) == 100:
        assert r.scene_info(S.MM_INFO_GRID_FACES) == (0.0 if S.MM_OPT_GRID_WIDE in opts else 1.0)
    n = G.SIZES[-1]
    _check_rays(r, ref_lib, "crate1", ("finite", n), _finite_rays("crate1", n)[0], opts)
    r.sync()
    r.close()


@pytest.mark.parametrize("name", G.SCENES)
def test_non_finite_rays_bit_exact(gpu, ref_lib, name):
    """Class 6: one component of o or d is NaN, +inf or -inf; every policy
    returns the reference's (1e30, MISS).  Why each query terminates:
      the guard refuses a non-finite direction: as unsigned integers the bits of |NaN| and |inf| lie above 2^40's in ray_fast_ok_boxed (test_gpu_arith.py's ray_guard row covers every pattern), and dir_ok's ordered compares fail in ray_fast_ok;
      a NaN or infinite origin fails grid_ray_ok, six positive compares o >= mn, o <= mx against a finite box (mm_query_rays passes hit_origin = false: the box is always checked), and org_ok's, so no grid walk and no Markstein quotient sees such a ray;
      the fallback walk (traverse_li<false>, traverse<false>, traverse_reference) visits each node at most once: a node is entered from the root or from its parent's step only, pushed at most once and popped once, whatever the slab tests return, so it ends after at most 2P - 1 visits (aabb_pairs returns tmin or 1e30, never NaN: a NaN fails its `tmax >= tmin`)."""
    rays_all, cls = G.rays_of(name, G.SIZES[-1])
    rays = np.ascontiguousarray(rays_all[cls == 6])
    assert len(rays) == 1024 and not np.isfinite(rays[:, :, :3]).all(axis=(1, 2)).any()
    s = S.scene(name)
    for policy in RAY_POLICIES:
        r = _renderer(s, POLICIES[policy])
        if _unsupported(r, POLICIES[policy]):
            r.close()
            continue
        for n in (1, 63, len(rays)):
            k_ref = _check_rays(r, ref_lib, name, ("nonfinite", n), rays[:n], (name, policy, n))
            assert (k_ref == A.MISS).all()
        r.sync()
        r.close()


@pytest.mark.parametrize("e", [24, 25])
def test_scaled_crate_rays_bit_exact(gpu, ref_lib, e):
    """crate1 scaled by 2^24 (every rect answers) and by 2^25, where five of the
    six faces have dot(n, n) = inf, a zero normal and never answer
    ("Large rects"; test_guard_edges.py): k_prep_rects
    computes n with the reference's operations, so the answers agree."""
    s = _cached(("scaled", e), lambda: G.scaled(S.scene("crate1"), 2.0 ** e))
    rng = np.random.default_rng(3)
    n = 2048 + 37
    d = rng.normal(size=(n, 3))
    rays = np.zeros((n, 2, 4), np.float32)
    rays[:, 0, :3] = np.float32(rng.uniform(-60, 60, (n, 3))) * np.float32(2.0 ** e)
    rays[:, 1, :3] = d / np.linalg.norm(d, axis=1)[:, None]
    t_ref, k_ref = A.Ref(ref_lib, s).query(rays)
    assert (k_ref != A.MISS).sum() > 300 and ((k_ref < 6).sum() > 1000) == (e == 24)
    for policy in ("auto", "trav5-lds0", "reference"):
        r = _renderer(s, POLICIES[policy])
        t, k = r.query_rays(rays)
        bad = (_bits(t) != t_ref.view(np.uint32)) | (_bits(k) != k_ref)
        assert not bad.any(), (e, policy, int(bad.sum()), np.flatnonzero(bad)[:8])
        r.sync()
        r.close()


# ---- AOV ----------------------------------------------------------------------------
@pytest.mark.parametrize("policy", RAY_POLICIES)
@pytest.mark.parametrize("name", G.CAMERA_SCENES)
def test_aov_through_the_edge_cameras_bit_exact(gpu, ref_lib, name, policy):
    """mm_trace_aov over S.B_TILE through tiny-focal, tiny-viewport, huge-focal
    (every query outside the direction guard; huge-focal's primary_dir takes
    rsq_ieee) and tiny-centre (every query outside the origin guard)."""
    r = _renderer(S.scene(name), POLICIES[policy])
    assert not _unsupported(r, POLICIES[policy]), (name, policy)  # both scenes have a grid and lean records
    for cn, u in G.edge_cameras(name).items():
        for limit in G.LIMITS:
            d = _tile_diffs(_aov(r, u, limit, S.B_TILE), _ref_tile(ref_lib, name, u, limit, S.B_TILE))
            assert not any(d.values()), (name, policy, cn, limit, d)
    r.sync()
    r.close()


@pytest.mark.parametrize("policy", RAY_POLICIES)
def test_aov_corridor_chains_outside_the_guard_bit_exact(gpu, ref_lib, policy):
    """The corridor's row py = 32 at mirror limit 200: chains of up to 199
    hit-origin continuation rays (GridQuery skips their box check) with d.y = 0
    and, through corridor-across, a tiny d.z kept by every reflection."""
    s, _ = A.corridor()
    r = _renderer(s, POLICIES[policy])
    if _unsupported(r, POLICIES[policy]):
        u = G.edge_cameras("corridor")["corridor-tiny-focal"]
        _expect_unsupported(r, lambda: _aov(r, u, 200, G.CORRIDOR_TILE))
        return
    for cn, u in G.edge_cameras("corridor").items():
        ref = _ref_tile(ref_lib, "corridor", u, 200, G.CORRIDOR_TILE)
        assert A.kinds(ref["id"])[2].any() and ref["albedo"][..., 3].max() == 199.0
        d = _tile_diffs(_aov(r, u, 200, G.CORRIDOR_TILE), ref)
        assert not any(d.values()), (policy, cn, d)
    r.sync()
    r.close()


# ---- path kernels -----------------------------------------------------------------------
@pytest.mark.parametrize("form", sorted(PATH_FORMS))
@pytest.mark.parametrize("name", G.CAMERA_SCENES)
def test_path_windows_through_the_edge_cameras_bit_exact(gpu, ref_lib, name, form):
    """mm_trace_tile, a 32 x 16 window at 8 spp, 8 / 8 bounces: pixels and
    (rays, paths) against the reference's trace_tile.  Through tiny-focal the
    waves hold primaries outside the guard next to ordinary bounce rays."""
    r = _renderer(S.scene(name), PATH_FORMS[form])
    assert r.scene_info(S.MM_INFO_GRID_OK) == 1.0 and r.scene_info(MM_INFO_LEAN) == 1.0
    for cn, u in G.edge_cameras(name).items():
        ref, counts = _ref_window(ref_lib, name, u)
        got, st = r.trace_tile(u, S.ext(), *G.WINDOW, 32, 16, stats=True)
        bad = int((_bits(got) != _bits(ref)).sum())
        assert bad == 0 and (st.rays, st.paths) == counts, (name, form, cn, bad, (st.rays, st.paths), counts)
    r.sync()
    r.close()


# ---- camera sequence ------------------------------------------------------------------
@pytest.mark.parametrize("name", G.CAMERA_SCENES)
def test_edge_cameras_as_one_sequence_equal_single_calls_and_the_reference(gpu, ref_lib, name):
    """The four cameras and the default one as one mm_trace_tile_cameras launch
    and one mm_trace_aov sequence: the camera records -- a denormal and a -0.0
    among their floats -- come through scalar loads there (frame_camera)."""
    from mirror_maze import default_uniform
    from test_gpu_camera_sequence import _with_cam

    cams = dict(G.edge_cameras(name))
    cams["default"] = default_uniform(*G.VIEW, 0)
    u = cams["default"]
    rows = np.stack([G.cam10(c) for c in cams.values()])
    assert (rows.view(np.uint32) == 0x80000000).any() and (np.abs(rows[rows != 0]) < 2.0 ** -126).any()
    r = _renderer(S.scene(name), {})
    seq, st = r.trace_tile_cameras(u, rows, S.ext(), *G.WINDOW, 32, 16, stats=True)
    aov = _aov(r, u, 15, S.B_TILE, cameras=rows)
    assert seq.shape == (5, 16, 32, 4) and aov["id"].shape == (5, 5, 67)
    rays = 0
    for f, (cn, c) in enumerate(cams.items()):
        uf = _with_cam(u, rows[f])
        assert bytes(uf.cam) == bytes(c.cam)
        ref, counts = _ref_window(ref_lib, name, uf, frame=1 + f)  # (frame f of a sequence draws with RNG frame ext.frame + f)
        rays += counts[0]
        assert int((_bits(seq[f]) != _bits(ref)).sum()) == 0, (name, cn)
        one, _ = r.trace_tile(uf, _ext(1 + f), *G.WINDOW, 32, 16)
        assert np.array_equal(_bits(one), _bits(seq[f])), (name, cn)
        d = _tile_diffs(aov, _ref_tile(ref_lib, name, uf, 15, S.B_TILE), f)
        assert not any(d.values()), (name, cn, d)
        one = _aov(r, uf, 15, S.B_TILE)
        assert all(np.array_equal(_bits(one[k])[0], _bits(aov[k])[f]) for k in NAMES), (name, cn)
    assert st.rays == rays and st.paths == 5 * 32 * 16 * 8
    r.sync()
    r.close()
