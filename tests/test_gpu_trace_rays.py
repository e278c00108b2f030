"""Ray lists (mm_trace_rays, Renderer.trace_rays): entry e of a launch is the
mean of ext.spp paths along the caller's ray e, and must equal tests/rays_ref.c
-- the resolve and the jitter of include/mm_api.h over the oracle's trace_path
and tile seed -- on float bits, with zero differing elements.  The references
are computed once per module (tests/rays_support.py) and left unchanged."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

import rays_support as rs

pytestmark = pytest.mark.gpu

MM_OPT_FUSE_RESOLVE = 12
LIMITS = {"maze": (8, 8), "corridor15": (8, 15), "corridor200": (8, 200), "soup": (8, 8)}
# MM_OPT_* sets the soup is traced with: the grid search with its index in LDS, BVH loop form 5 with everything
# through L1/L2, the grid search all-global (tests/test_gpu_trace_pixels.py test_rect_soup)
SOUP_OPTS = {"auto-grid": {}, "bvh-li": {7: 5}, "grid-global": {7: 11, 1: 0}}


def _bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _diff(got, ref):
    return int((_bits(got) != _bits(ref)).sum())


def _ext(case, spp, flags=0):
    from mirror_maze import make_ext

    b, m = LIMITS[case]
    return make_ext(spp, b, m, frame=rs.FRAME, flags=flags)


def _renderer(scene, opts=None, pipe=0):
    from mirror_maze import Renderer

    r = Renderer(0)
    r.set_pipeline(pipe)
    for k, v in (opts or {}).items():
        r.set_option(k, v)
    if scene is not None:
        r.upload_scene(scene)
    return r


@functools.lru_cache(maxsize=None)
def _case(case):
    """(Scene, records (185, 8), kinds, {(spp, jitter): (out, var, queries)}) of a case, read-only.  The seven
    equal-geometry pairs are the first candidates (rays_support.candidates) whose two keys give different
    reference values at every spp and in both jitter modes: picked with the reference alone."""
    name = "corridor" if case.startswith("corridor") else case
    s, _ = rs.scene(name)
    ref = rs.Ref(s)
    co, cd = rs.candidates(name)
    rng = np.random.default_rng(9)
    ka, kb = rng.integers(0, 2**32, (2, len(co)), dtype=np.uint64)
    differ = np.ones(len(co), bool)
    for spp in rs.SPPS:
        for jitter in (False, True):
            a = ref.trace(_ext(case, spp), rs.pack(co, cd, ka), jitter)[0]
            b = ref.trace(_ext(case, spp), rs.pack(co, cd, kb), jitter)[0]
            differ &= (_bits(a) != _bits(b)).any(axis=1)
    pick = np.flatnonzero(differ)[:7]
    assert len(pick) == 7, (case, int(differ.sum()))
    rays, kind = rs.ray_list(name, np.stack([co[pick], cd[pick]], axis=1),
                             np.stack([ka[pick], kb[pick]], axis=1))
    # the record with dz = -0.0f starts its paths along -0.0f without the jitter and along +0.0f with it
    # (-0.0f + 0.0f), in the reference the results are compared with
    rec = rays[kind["minus_zero_z"][0]]
    plain, jittered = rs.start_dir(rec, 0, rs.FRAME, False), rs.start_dir(rec, 0, rs.FRAME, True)
    assert np.signbit(plain[2]) and np.array_equal(_bits(plain), _bits(rec[4:7]))
    assert jittered[2] == 0.0 and not np.signbit(jittered[2]) and jittered[0] != rec[4] and jittered[1] != rec[5]
    refs = {}
    for spp in rs.SPPS:
        for jitter in (False, True):
            out, var, q = ref.trace(_ext(case, spp), rays, jitter)
            out.setflags(write=False)
            var.setflags(write=False)
            refs[(spp, jitter)] = (out, var, q)
    return s, rays, kind, refs


def _routes():
    from mirror_maze import MM_PIPE_REFERENCE

    return {"fused": ({}, 0), "unfused": ({MM_OPT_FUSE_RESOLVE: 0}, 0), "reference": ({}, MM_PIPE_REFERENCE)}


CASES = [("maze", "auto"), ("corridor15", "auto"), ("corridor200", "auto")] + [("soup", k) for k in SOUP_OPTS]


@pytest.mark.parametrize("route", ["fused", "unfused", "reference"])
@pytest.mark.parametrize("case,form", CASES, ids=[f"{c}-{f}" for c, f in CASES])
def test_against_the_oracle(gpu, case, form, route):
    """1. The 185 rays of every kind (rays_support.ray_list) at spp 8 and 64 (fused resolve), 3 and 24 (staged),
    with and without MM_RAYS_JITTER, through MM_OPT_FUSE_RESOLVE 1 and 0 and MM_PIPE_REFERENCE; stats (rays and
    paths exact) on half of the calls, so both the counting and the plain instances run every resolve.

    Equal geometry with different keys: two such rays coincide whenever neither path's value depends on a random
    number -- a ray that leaves the scene unhit, or ends on a dark surface, gives (0, 0, 0) under every key; of
    rays_support.candidates' 80 random rays 13 coincide in the maze, 44 and 43 in the corridor (limits 15 and
    200) and 33 in the soup, at one spp or jitter mode at least.  Among rays whose
    values do depend on the stream a coincidence needs all 96 bits of two means of different samples to agree,
    which no share can be promised for but none was seen.  The seven pairs used are those for which the
    reference alone gives different values at every spp and in both jitter modes (_case)."""
    from mirror_maze import MM_INFO_LAST_DEFER

    s, rays, kind, refs = _case(case)
    opts, pipe = _routes()[route]
    r = _renderer(s, {**SOUP_OPTS.get(form, {}), **opts}, pipe)
    import torch

    dev_rays = torch.from_numpy(np.array(rays)).cuda()
    for spp in rs.SPPS:
        for jitter in (False, True):
            want, _, queries = refs[(spp, jitter)]
            stats = (spp in (8, 3)) != jitter
            got, st = r.trace_rays(_ext(case, spp), dev_rays, jitter=jitter, stats=stats)
            got = got.cpu().numpy()
            bad = _diff(got, want)
            print(f"{case} {form} {route} spp {spp} jitter {jitter}: differing words {bad}")
            assert got.shape == (rs.N_RAYS, 4) and bad == 0, (case, form, route, spp, jitter, bad)
            if stats:
                assert (st.rays, st.paths) == (queries, rs.N_RAYS * spp)
            assert r.scene_info(MM_INFO_LAST_DEFER) == 0
            # duplicate records: equal results; equal geometry under another key: different ones
            assert np.array_equal(_bits(got[kind["duplicates"]]), _bits(got[:7]))
            assert (_bits(got[kind["pair_a"]]) != _bits(got[kind["pair_b"]])).any(axis=1).all()
    r.close()


@pytest.mark.parametrize("n", [1, 64])
def test_short_lists(gpu, n):
    """n_rays of 1 and of 64 (one chunk at 1 spp... eight at 8): the list's first entries, whose values do not
    depend on the list's length."""
    import torch

    s, rays, _, refs = _case("maze")
    r = _renderer(s)
    dev_rays = torch.from_numpy(np.array(rays[:n])).cuda()
    for spp in rs.SPPS:
        got, st = r.trace_rays(_ext("maze", spp), dev_rays, jitter=True, stats=True)
        assert got.shape == (n, 4) and _diff(got, refs[(spp, True)][0][:n]) == 0, (n, spp)
        assert st.paths == n * spp
    r.close()


@pytest.mark.parametrize("route", ["fused", "unfused", "reference"])
def test_flags(gpu, route):
    """MM_EXT_RGBA8 is quantize() of the float result; MM_EXT_ACCUMULATE into a buffer of 7.0 gives 7 + the
    value and alpha 8 -- at spp 8 and 3, so through the fused store and the resolve kernels' (unfused,
    reference: the kernels' at both)."""
    import torch

    from mirror_maze import MM_EXT_ACCUMULATE

    s, rays, _, refs = _case("maze")
    opts, pipe = _routes()[route]
    r = _renderer(s, opts, pipe)
    dev_rays = torch.from_numpy(np.array(rays)).cuda()
    for spp in (8, 3):
        want = refs[(spp, False)][0]
        u8, _ = r.trace_rays(_ext("maze", spp), dev_rays, rgba8=True)
        assert u8.dtype == torch.uint8 and u8.shape == (rs.N_RAYS, 4)
        assert torch.equal(u8, r.quantize(torch.from_numpy(np.array(want)).cuda()))
        assert int(u8[:, :3].max()) > 0 and int(u8[:, 3].min()) == 255
        acc = torch.full((rs.N_RAYS, 4), 7.0, device="cuda")
        r.trace_rays(_ext("maze", spp, MM_EXT_ACCUMULATE), dev_rays, out=acc)
        assert _diff(acc, np.float32(7.0) + want) == 0 and (acc[:, 3] == 8.0).all()
    r.close()


# ---- 2. every built variant -------------------------------------------------------
def _pairs():
    import variant_census_support as vc

    return sorted(vc.PAIR_SITES)


@pytest.mark.parametrize("pair", _pairs(), ids=lambda p: f"m{p[0]}f{p[1]}")
def test_every_built_variant(gpu, pair):
    """2. One 185-ray, 8-spp list through every built (LDS mode, form) pair's ray-list instance, on the scene
    and options the variant census runs the pair with: the primary rays of the census window's first 185
    pixels under the scene's camera 0, keyed by pixel, with the jitter.  The launch runs the pair, ring 0."""
    import torch

    import variant_census_support as vc
    from mirror_maze import MM_INFO_LAST_DEFER, MM_INFO_LAST_KERNEL_FORM, MM_INFO_LAST_LDS_MODE, MM_INFO_LAST_RING

    key, opts = vc.PAIR_SITES[pair]
    u = vc.uniform(key, 0)
    x0, y0 = vc.ORIGIN
    px = np.stack([x0 + np.arange(rs.N_RAYS) % 32, y0 + np.arange(rs.N_RAYS) // 32], axis=1)
    rays = rs.pixel_records(u, px)
    want, _, queries = rs.Ref(vc.scene(key)).trace(vc.ext(), rays, True)
    r = _renderer(None, opts)
    r.upload_scene(vc.scene(key))
    got, st = r.trace_rays(vc.ext(), torch.from_numpy(rays).cuda(), jitter=True, stats=pair[1] % 2 == 1)
    r.sync()
    ran = (r.scene_info(MM_INFO_LAST_LDS_MODE), r.scene_info(MM_INFO_LAST_KERNEL_FORM), r.scene_info(MM_INFO_LAST_RING))
    defer = r.scene_info(MM_INFO_LAST_DEFER)
    r.close()
    bad = _diff(got, want)
    print(f"m{pair[0]}f{pair[1]}: ran {ran} defer {defer} differing words {bad}")
    assert bad == 0
    if st is not None:
        assert (st.rays, st.paths) == (queries, rs.N_RAYS * vc.SPP)
    assert ran == (float(pair[0]), float(pair[1]), 0.0) and defer == 0


# ---- 3. equivalence with the pixel list -----------------------------------------------
@pytest.mark.parametrize("spp", [8, 24])
@pytest.mark.parametrize("name", ["maze", "corridor"])
def test_primary_rays_equal_the_pixel_list(gpu, name, spp):
    """3. 185 scattered pixels of a view, 20 of them twice, none outside it: the records (cam.center,
    y*view_w + x, oracle_primary_dir) with the jitter give trace_pixels' out and trace_pixels_var's var."""
    import torch

    import aov_support
    from mirror_maze import default_uniform, make_ext

    s, _ = rs.scene(name)
    u = aov_support.corridor()[1] if name == "corridor" else default_uniform(320, 180, 0)
    W, H = int(u.view_w), int(u.view_h)
    rng = np.random.default_rng(3)
    px = np.stack([rng.integers(0, W, 165), rng.integers(0, H, 165)], axis=1)
    px = np.concatenate([px, px[rng.permutation(165)[:20]]])[rng.permutation(185)]
    assert len(px) == rs.N_RAYS and len({(int(x), int(y)) for x, y in px}) < 185
    rays = torch.from_numpy(rs.pixel_records(u, px)).cuda()
    e = make_ext(spp, 8, 15, frame=rs.FRAME)
    r = _renderer(s)
    want, _ = r.trace_pixels(u, e, px.astype(np.uint32))
    want_out, want_var, _ = r.trace_pixels_var(u, e, px.astype(np.uint32))
    got, _ = r.trace_rays(e, rays, jitter=True)
    got_out, got_var, _ = r.trace_rays(e, rays, jitter=True, var=True)
    assert _diff(got, want) == 0 and _diff(got_out, want_out) == 0 and _diff(got_var, want_var) == 0
    assert float(want[:, :3].max()) > 0 and _diff(got, got_out) == 0
    # without the jitter the directions differ, and so do the results
    plain, _ = r.trace_rays(e, rays, jitter=False)
    assert _diff(plain, want) > 0
    r.close()


# ---- 4. variance ----------------------------------------------------------------------
@pytest.mark.parametrize("route", ["fused", "reference"])
@pytest.mark.parametrize("spp", [8, 3])
def test_variance(gpu, spp, route):
    """4. var_dev against tests/rays_ref.c at spp 8 (blocks of 8) and 3 (left to right); out with var_dev is
    out without it."""
    import torch

    s, rays, _, refs = _case("maze")
    opts, pipe = _routes()[route]
    r = _renderer(s, opts, pipe)
    dev_rays = torch.from_numpy(np.array(rays)).cuda()
    for jitter in (False, True):
        want, want_var, queries = refs[(spp, jitter)]
        out, var, st = r.trace_rays(_ext("maze", spp), dev_rays, jitter=jitter, var=True, stats=True)
        assert var.shape == (rs.N_RAYS,) and _diff(out, want) == 0 and _diff(var, want_var) == 0
        assert float(var.max()) > 0 and (st.rays, st.paths) == (queries, rs.N_RAYS * spp)
        mine = torch.full((rs.N_RAYS,), -1.0, device="cuda")
        out2, var2, _ = r.trace_rays(_ext("maze", spp), dev_rays, jitter=jitter, var=mine)
        assert var2 is mine and _diff(mine, want_var) == 0 and _diff(out2, want) == 0
    r.close()


# ---- 5. errors ------------------------------------------------------------------------
def test_arguments(gpu):
    """5. Every MM_ERR_INVALID condition through the C entry point and as MMError from Renderer.trace_rays;
    n_rays = 0 takes no call number; no scene; MM_PIPE_WAVEFRONT.  (No scene whose traversal stack overflows
    can be uploaded -- mm_upload_scene refuses a BVH deeper than the stack, tests/test_gpu_parity.py -- so
    MM_ERR_STACK has no case here.)  Then a valid call still matches the reference."""
    import torch

    from mirror_maze import MM_PIPE_WAVEFRONT, MMError, lib, make_ext
    from mirror_maze._lib import (MM_ERR_INVALID, MM_ERR_NO_SCENE, MM_ERR_UNSUPPORTED, MM_EXT_ACCUMULATE, MM_EXT_RGBA8,
                                  MM_OK, MM_RAYS_JITTER)

    s, rays, _, refs = _case("maze")
    r = _renderer(s)
    dev_rays = torch.from_numpy(np.array(rays)).cuda()
    out = torch.zeros((186, 4), dtype=torch.float32, device="cuda")
    var = torch.zeros((186,), dtype=torch.float32, device="cuda")
    e = _ext("maze", 8)
    P = C.c_void_p

    def raw(ext=e, flags=0, src=dev_rays.data_ptr(), n=185, dst=out.data_ptr(), v=None, ctx=None):
        return lib().mm_trace_rays(ctx or r._ctx, C.byref(ext) if ext is not None else None, flags, P(src), n, P(dst),
                                   P(v), None)

    assert lib().mm_trace_rays(None, C.byref(e), 0, P(dev_rays.data_ptr()), 185, P(out.data_ptr()), None,
                               None) == MM_ERR_INVALID
    for kw in (dict(ext=None), dict(src=None), dict(dst=None)):
        assert raw(**kw) == MM_ERR_INVALID, kw
    assert raw(src=dev_rays.data_ptr() + 4) == MM_ERR_INVALID
    assert raw(dst=out.data_ptr() + 4) == MM_ERR_INVALID
    assert raw(ext=make_ext(8, 8, 8, flags=MM_EXT_RGBA8), dst=out.data_ptr() + 2) == MM_ERR_INVALID
    for flags in (2, 3, 0x80000000):
        assert raw(flags=flags) == MM_ERR_INVALID
    for bad in (make_ext(0, 8, 8), make_ext(4097, 8, 8), make_ext(8, 32768, 8), make_ext(8, 8, 32768),
                make_ext(8, 8, 8, flags=MM_EXT_RGBA8 | MM_EXT_ACCUMULATE)):
        assert raw(ext=bad) == MM_ERR_INVALID, bytes(bad)
    # the variance buffer's conditions
    assert raw(ext=make_ext(1, 8, 8), v=var.data_ptr()) == MM_ERR_INVALID
    assert raw(ext=make_ext(8, 8, 8, flags=MM_EXT_ACCUMULATE), v=var.data_ptr()) == MM_ERR_INVALID
    assert raw(v=var.data_ptr() + 2) == MM_ERR_INVALID
    assert raw(v=out.data_ptr() + 16) == MM_ERR_INVALID
    # the 32-bit queue and the 2^29 staged paths (nothing is read)
    assert raw(ext=make_ext(4096, 8, 8), n=2**20) == MM_ERR_INVALID
    assert raw(ext=make_ext(1, 8, 8), n=2**32 - 2**24) == MM_ERR_INVALID
    assert raw(ext=make_ext(1, 8, 8), n=2**40) == MM_ERR_INVALID
    assert raw(ext=make_ext(3, 8, 8), n=2**29 // 3 + 1) == MM_ERR_INVALID
    assert raw(n=2**26 + 1, v=var.data_ptr()) == MM_ERR_INVALID
    r.set_option(MM_OPT_FUSE_RESOLVE, 0)
    assert raw(n=2**26 + 1) == MM_ERR_INVALID
    r.set_option(MM_OPT_FUSE_RESOLVE, 1)
    assert r.last_call() == 0
    # ... and as the binding's exception
    for bad in (make_ext(0, 8, 8), make_ext(8, 8, 8, flags=MM_EXT_ACCUMULATE)):
        with pytest.raises(MMError) as ei:
            r.trace_rays(bad, dev_rays, var=True)
        assert ei.value.code == MM_ERR_INVALID and "mm_trace_rays" in str(ei.value)
    with pytest.raises(ValueError):
        r.trace_rays(e, dev_rays.view(-1, 2, 4))
    with pytest.raises(ValueError):
        r.trace_rays(e, dev_rays, var=torch.zeros((184,), device="cuda"))
    # nothing to do: MM_OK, no call number
    assert raw(n=0) == MM_OK and raw(n=0, src=None, dst=None, ext=None, flags=0x80) == MM_OK
    empty, st = r.trace_rays(e, dev_rays[:0], stats=True)
    assert empty.shape == (0, 4) and r.last_call() == 0
    bare = _renderer(None)
    assert raw(ctx=bare._ctx) == MM_ERR_NO_SCENE
    bare.close()
    wave = _renderer(s, pipe=MM_PIPE_WAVEFRONT)
    assert raw(ctx=wave._ctx) == MM_ERR_UNSUPPORTED
    wave.close()
    got, _ = r.trace_rays(e, dev_rays, jitter=True)
    assert _diff(got, refs[(8, True)][0]) == 0 and r.last_call() == 1
    assert raw(flags=MM_RAYS_JITTER) == MM_OK and r.last_call() == 2
    r.sync()
    assert _diff(out[:185], refs[(8, True)][0]) == 0
    r.close()


# ---- 6. helpers -----------------------------------------------------------------------
def test_ray_helpers(gpu):
    """6. pack_rays writes the key's bits; equirect_rays and ortho_rays return the documented shape, unit
    directions and keys y*w + x; a 64 x 32 panorama of the N=10 maze equals the reference on the rays the
    helper produced."""
    import torch

    from mirror_maze import default_uniform, equirect_rays, ortho_rays, pack_rays

    keys = torch.tensor([0, 1, 2**31, 2**32 - 1, 0x3F800000], dtype=torch.int64)
    rec = pack_rays(torch.arange(15, dtype=torch.float32).reshape(5, 3), torch.ones(5, 3), keys)
    assert rec.shape == (5, 8) and rec.dtype == torch.float32
    assert (rec.view(torch.int32)[:, 3].to(torch.int64) & 0xFFFFFFFF).tolist() == keys.tolist()
    assert rec[4, 3] == 1.0 and rec[:, 0:3].flatten().tolist() == list(range(15)) and (rec[:, 4:7] == 1).all()
    assert (rec[:, 7] == 0).all()

    u = default_uniform(320, 180, 0)
    centre, quat = list(u.cam.center), list(u.cam.quat)
    w, h = 64, 32
    pano = equirect_rays(centre, quat, w, h)
    orth = ortho_rays([-50.0, -1.0, -50.0], [100.0, 0.0, 0.0], [0.0, 0.0, 100.0], [0.0, 2.0, 0.0], w, h)
    for rays in (pano, orth):
        assert rays.shape == (w * h, 8) and rays.is_cuda and rays.dtype == torch.float32
        assert torch.allclose(rays[:, 4:7].norm(dim=1), torch.ones(w * h, device="cuda"), atol=1e-6)
        assert rays.view(torch.int32)[:, 3].tolist() == list(range(w * h))  # key y*w + x, row-major
    assert (pano[:, 0:3].cpu() == torch.tensor(centre)).all()
    # the panorama's middle looks where the pinhole's middle looks, its columns go round once
    mid = pano[(h // 2) * w + w // 2, 4:7].cpu().numpy()
    fwd = rs.primary_dirs(u, [[160, 90]])[0]
    assert float(np.dot(mid, fwd / np.linalg.norm(fwd))) > 0.99
    assert float(pano[(h // 2) * w, 4:7].cpu().numpy() @ mid) < -0.95
    assert (orth[:, 4:7].cpu() == torch.tensor([0.0, 1.0, 0.0])).all()
    assert torch.allclose(orth[0, 0:3].cpu(), torch.tensor([-50.0 + 50.0 / w, -1.0, -50.0 + 50.0 / h]))

    s, _ = rs.scene("maze")
    e = _ext("maze", 8)
    want, _, queries = rs.Ref(s).trace(e, pano.cpu().numpy(), False)
    r = _renderer(s)
    got, st = r.trace_rays(e, pano, stats=True)
    assert _diff(got, want) == 0 and (st.rays, st.paths) == (queries, w * h * 8)
    assert int((got[:, :3].sum(dim=1) > 0).sum()) > 0
    r.close()
