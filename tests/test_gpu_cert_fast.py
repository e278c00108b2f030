"""The grid search with its fast certificate (mm_grid.h) on the GPU, bit for bit against the reference walk, where
the fast certificate and the full one meet: the rays aimed at the band around the rects' edges
(tests/cert_fast_support.py) through mm_query_rays, and path windows through the wave-persistent kernel with
the tail rings on and off.  mm_query_rays asks the grid search only for rays inside the guards whose origin
lies in the grid box (mm_path.h GridQuery); the others -- a quarter of the aimed set by construction, origins
beyond the box -- it answers with the BVH walk, and they are compared all the same.  The shares below and in
tests/test_cert_fast.py are counted over the rays that do reach the certificate on the device."""
from __future__ import annotations

import numpy as np
import pytest

import aov_support as A
import cert_fast_support as S
import grid_forms_support as G

pytestmark = pytest.mark.gpu

VIEW = (640, 480)
WINDOWS = [(288, 224), (96, 416)]  # 64 x 32 each: the horizon down the corridors, the floor in front of the camera
DEFER = {"off": {G.MM_OPT_DEFER: 0}, "on": {G.MM_OPT_DEFER: 32, G.MM_OPT_DEFER_MIN: 0}}


@pytest.fixture(scope="module")
def ref_lib(tmp_path_factory):
    return A.build_ref(tmp_path_factory.mktemp("aov_ref"))


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return S.build_twin(tmp_path_factory.mktemp("cert_fast_ref"))


def _bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint32)


def _renderer(opts):
    from mirror_maze import Renderer

    r = Renderer(0)
    for k, v in opts.items():
        r.set_option(k, v)
    r.upload_scene(S.maze())
    assert int(r.scene_info(G.MM_INFO_GRID_OK)) == 1 and int(r.scene_info(G.MM_INFO_GRID_FLAT)) == 1
    return r


def test_aimed_rays_bit_exact(gpu, ref_lib, twin):
    """4133 aimed rays on the N = 10 maze: (t, k) of mm_query_rays equal the walk's on every ray, under the
    default policy (the grid search) and with the grid read from global memory.  Of them 2325 reach the
    certificate on the device (origin in the grid box, answered; 483 of those from the grid box's faces, the
    largest |o| grid_ray_ok admits), 36 % on the full certificate and 64 % on the fast one (the C twin's
    verdicts, asserted here as in tests/test_cert_fast.py)."""
    s = S.maze()
    ref = A.Ref(ref_lib, s)
    c = S.Certs(twin, s)
    rays, _, kind, (t_ref, k_ref) = S.aimed_rays(s, c, ref)
    q = S.answered(rays, t_ref, k_ref)
    fl = c.flags(q)
    reach = (fl != S.NO_CERT) & S.reaches(S.grid_of(s), q)
    fast = reach & (fl & S.FAST != 0)
    assert reach.sum() >= 2000 and 0.25 * reach.sum() <= fast.sum() <= 0.75 * reach.sum(), (int(reach.sum()), int(fast.sum()))
    assert 0 < (fast & (kind == 2)).sum() < (reach & (kind == 2)).sum()
    for opts in ({}, {G.MM_OPT_TRAVERSAL: 11, G.MM_OPT_LDS_NODES: 0}):
        r = _renderer(opts)
        t, k = r.query_rays(np.array(rays))
        bad = (_bits(t) != t_ref.view(np.uint32)) | (_bits(k) != k_ref)
        assert not bad.any(), (opts, int(bad.sum()), np.flatnonzero(bad)[:8])
        r.sync()
        r.close()


@pytest.mark.parametrize("defer", sorted(DEFER))
def test_path_windows_bit_exact(gpu, defer):
    """Two 64 x 32 windows of a 640 x 480 frame of the N = 10 maze at 8 spp, 8 / 8 bounces through the
    wave-persistent kernel, with deferral to the tail rings off and forced on: pixels and (rays, paths) against
    the oracle, 0 ulp."""
    from mirror_maze import MM_INFO_LAST_DEFER, default_uniform, make_ext
    from oracle.oracle import Oracle

    o = Oracle.from_scene(S.maze())
    r = _renderer(DEFER[defer])
    u, e = default_uniform(*VIEW, 0), make_ext(8, 8, 8, frame=1)
    for (x0, y0) in WINDOWS:
        want, wst = o.trace_tile(u, e, x0, y0, 64, 32)
        got, st = r.trace_tile(u, e, x0, y0, 64, 32, stats=True)
        bad = int((_bits(got) != _bits(want)).sum())
        assert bad == 0, (defer, x0, y0, bad)
        assert (st.rays, st.paths) == (wst.rays, wst.paths), (defer, x0, y0)
    assert r.scene_info(G.MM_INFO_LAST_FORM) == 11.0
    assert r.scene_info(MM_INFO_LAST_DEFER) == (1.0 if defer == "on" else 0.0)
    r.sync()
    r.close()


@pytest.mark.parametrize("defer", sorted(DEFER))
def test_telephoto_windows_bit_exact(gpu, defer):
    """Bounce rays from coarse origins (cert_fast_support.telephoto_gallery: hit points rounded at 2^-12 C; GridQuery
    takes them without the box check): two 32 x 16 windows at 8 spp, 8 / 8 bounces against the oracle, 0 ulp.
    tests/test_cert_fast.py states what these queries are on the CPU."""
    from mirror_maze import Renderer, make_ext
    from oracle.oracle import Oracle

    s, u = S.telephoto_gallery()
    o = Oracle.from_scene(s)
    r = Renderer(0)
    for k, v in DEFER[defer].items():
        r.set_option(k, v)
    r.upload_scene(s)
    assert int(r.scene_info(G.MM_INFO_GRID_OK)) == 1 and int(r.scene_info(G.MM_INFO_GRID_FLAT)) == 1
    e = make_ext(8, 8, 8, frame=1)
    for (x0, y0) in S.TELE_WINDOWS:
        want, wst = o.trace_tile(u, e, x0, y0, 32, 16)
        got, st = r.trace_tile(u, e, x0, y0, 32, 16, stats=True)
        bad = int((_bits(got) != _bits(want)).sum())
        assert bad == 0, (defer, x0, y0, bad)
        assert (st.rays, st.paths) == (wst.rays, wst.paths), (defer, x0, y0)
    assert r.scene_info(G.MM_INFO_LAST_FORM) == 11.0
    r.sync()
    r.close()
