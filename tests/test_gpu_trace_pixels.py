"""Pixel lists (mm_trace_pixels, Renderer.trace_pixels): entry e of a launch is
the pixel (x, y) the list names, and must equal, on float bits with zero
differing entries, that pixel of the tile trace with the same uniform and ext
-- the CPU oracle's (oracle_tile) in the first test, Renderer.trace_tile's of
the auto pipeline elsewhere.  References are traced once per module and
gathered in list order."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from conftest import oracle_tile

pytestmark = pytest.mark.gpu

MM_INFO_LAST_FORM, MM_INFO_LAST_LDS_MODE, MM_INFO_LAST_DEFER = 11, 12, 14
VIEW = (320, 180)
WINDOW = (11, 7, 37, 5)  # x0, y0, w, h: 185 pixels
RINGS = {21: 32, 22: 0}  # tail rings on launches of any size: a list launch must not take them


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _diff(got, ref):
    return int((_bits(got) != _bits(ref)).any(axis=-1).sum())


_SCENES = {}


def _scene(n):
    from mirror_maze import Scene

    if n not in _SCENES:
        _SCENES[n] = Scene.build(n, 0)
    return _SCENES[n]


def _renderer(scene, opts=None, pipe=0):
    from mirror_maze import Renderer

    r = Renderer(0)
    r.set_pipeline(pipe)
    for k, v in (opts or {}).items():
        r.set_option(k, v)
    if scene is not None:
        r.upload_scene(scene)
    return r


def _window_list(seed=0):
    """A seeded permutation of the window's 185 pixels, (n, 2) uint32."""
    x0, y0, w, h = WINDOW
    xy = np.stack(np.meshgrid(np.arange(x0, x0 + w), np.arange(y0, y0 + h)), axis=-1).reshape(-1, 2)
    return np.ascontiguousarray(np.random.default_rng(seed).permutation(xy).astype(np.uint32))


def _gather(tile, x0, y0, pixels):
    """Rows of the (h, w, 4) tile at (x0, y0) in list order."""
    p = np.asarray(pixels).astype(np.int64)
    return np.asarray(tile)[p[:, 1] - y0, p[:, 0] - x0]


def _tile_ref(r, u, e, pixels):
    """trace_tile's value of every list entry: the list's bounding box traced
    once and gathered, or (a few pixels far apart in a large view) one 1 x 1
    tile per distinct pixel."""
    p = np.asarray(pixels).astype(np.int64)
    x0, y0 = int(p[:, 0].min()), int(p[:, 1].min())
    w, h = int(p[:, 0].max()) - x0 + 1, int(p[:, 1].max()) - y0 + 1
    if w * h * e.spp <= 1 << 23:
        tile, _ = r.trace_tile(u, e, x0, y0, w, h)
        return _gather(tile.cpu().numpy(), x0, y0, p)
    one = {}
    for x, y in {(int(x), int(y)) for x, y in p}:
        one[(x, y)] = r.trace_tile(u, e, x, y, 1, 1)[0].cpu().numpy()[0, 0]
    return np.stack([one[(int(x), int(y))] for x, y in p])


@pytest.fixture(scope="module")
def case1(gpu):
    """The N=32 maze at 320x180, the 37x5 window at (11, 7), 8 spp, 8/8 bounces,
    frame 5: the oracle's tile and ray count, read-only."""
    from mirror_maze import default_uniform, make_ext
    from oracle.oracle import Oracle

    s = _scene(32)
    u = default_uniform(*VIEW, 0)
    e = make_ext(8, 8, 8, frame=5)
    ref, rays = oracle_tile(Oracle.from_scene(s), u, e, *WINDOW)
    ref.setflags(write=False)
    return s, u, e, ref, rays


def _check_case1(r, case1):
    _, u, e, ref, rays = case1
    px = _window_list()
    got, st = r.trace_pixels(u, e, px, stats=True)
    assert got.shape == (185, 4)
    assert _diff(got.cpu().numpy(), _gather(ref, WINDOW[0], WINDOW[1], px)) == 0
    assert st.rays == rays and st.paths == 1480


def test_ragged_list_against_the_oracle(case1):
    """1. 185 pixels x 8 spp = 1480 paths: 24 chunks, the last padded."""
    assert (185 * 8) % 64 != 0 and -(-185 * 8 // 64) == 24
    r = _renderer(case1[0])
    _check_case1(r, case1)
    assert r.scene_info(MM_INFO_LAST_DEFER) == 0
    r.close()


def test_duplicates_and_scatter(case1):
    """2. The four view corners, 60 seeded pixels anywhere in the view and 20 of
    them again, against the full frame gathered."""
    s, u, e, _, _ = case1
    rng = np.random.default_rng(2)
    W, H = VIEW
    anywhere = np.stack([rng.integers(0, W, 60), rng.integers(0, H, 60)], axis=1)
    px = np.concatenate([[[0, 0], [W - 1, 0], [0, H - 1], [W - 1, H - 1]], anywhere, anywhere[rng.permutation(60)[:20]]])
    px = np.ascontiguousarray(px.astype(np.uint32))
    r = _renderer(s)
    frame, _ = r.trace_tile(u, e, 0, 0, W, H)
    want = _gather(frame.cpu().numpy(), 0, 0, px)
    got, st = r.trace_pixels(u, e, px, stats=True)
    got = got.cpu().numpy()
    assert _diff(got, want) == 0 and st.paths == len(px) * 8
    # equal entries, equal results; distinct pixels are not all equal
    first = {}
    for k, (x, y) in enumerate(px):
        assert got[k].tobytes() == got[first.setdefault((int(x), int(y)), k)].tobytes()
    assert len(first) < len(px) and len({g.tobytes() for g in got}) > 30
    r.close()


@pytest.mark.parametrize("spp,opts", [(1, {}), (3, {}), (3, RINGS), (24, {}), (24, RINGS), (64, {}), (4096, {})],
                         ids=["1", "3", "3-rings-requested", "24", "24-rings-requested", "64", "4096"])
def test_every_resolve(case1, spp, opts):
    """3. spp 1 (64 pixels per wave), 3 (staged, left to right), 24 (staged,
    blocks of 8), 64 (one pixel per wave), 4096 (the largest: 64 waves per
    pixel, staged), at 1, 7 and 185 entries.  With the tail rings requested the
    result is the same and the launch runs without them."""
    from mirror_maze import make_ext

    s, u = case1[0], case1[1]
    e = make_ext(spp, 8, 8, frame=9)
    px = _window_list(seed=spp)
    if spp == 4096:
        px = px[:7]
    ref_r = _renderer(s)
    want = _tile_ref(ref_r, u, e, px)
    ref_r.close()
    r = _renderer(s, opts)
    for n in (1, 7, 185):
        if n > len(px):
            continue
        got, st = r.trace_pixels(u, e, px[:n], stats=True)
        assert _diff(got.cpu().numpy(), want[:n]) == 0, (spp, n)
        assert st.paths == n * spp
        assert r.scene_info(MM_INFO_LAST_DEFER) == 0
    r.close()


def _scattered(view, n, seed):
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(np.stack([rng.integers(0, view[0], n), rng.integers(0, view[1], n)], axis=1)
                                .astype(np.uint32))


@pytest.mark.parametrize("case", ["form5", "form7", "no-lds", "reference"])
def test_query_methods_and_placements_on_the_maze(case1, case):
    """4a. MM_OPT_TRAVERSAL 5 and 7, MM_OPT_LDS_NODES 0 and MM_PIPE_REFERENCE
    on the N=32 maze, against the auto pipeline's trace_tile."""
    from mirror_maze import MM_PIPE_REFERENCE

    s, u, e = case1[:3]
    opts, pipe, form, modes = {"form5": ({7: 5}, 0, 5, (3,)), "form7": ({7: 7}, 0, 7, (3,)),
                               "no-lds": ({1: 0}, 0, 11, (13,)),
                               "reference": ({}, MM_PIPE_REFERENCE, None, None)}[case]
    px = _window_list(seed=4)
    auto = _renderer(s)
    want = _tile_ref(auto, u, e, px)
    auto.close()
    r = _renderer(s, opts, pipe)
    got, st = r.trace_pixels(u, e, px, stats=True)
    assert _diff(got.cpu().numpy(), want) == 0
    assert st.paths == 1480 and st.rays == case1[4]
    if form is not None:
        assert r.scene_info(MM_INFO_LAST_FORM) == form and r.scene_info(MM_INFO_LAST_LDS_MODE) in modes
    r.close()


def test_n64_scene_records_in_lds_boxes_through_cache(gpu):
    """4b. The N=64 maze (placement 14), 3840x2160, 40 scattered pixels, 64 spp,
    16/16 bounces."""
    from mirror_maze import default_uniform, make_ext

    s = _scene(64)
    u = default_uniform(3840, 2160, 0)
    e = make_ext(64, 16, 16, frame=7)
    px = _scattered((3840, 2160), 40, seed=64)
    r = _renderer(s)
    want = _tile_ref(r, u, e, px)
    got, _ = r.trace_pixels(u, e, px)
    assert _diff(got.cpu().numpy(), want) == 0
    assert r.scene_info(MM_INFO_LAST_LDS_MODE) == 14
    r.close()


@pytest.mark.parametrize("case", ["auto-grid", "bvh-li", "grid-global"])
def test_rect_soup(gpu, case):
    """4c. A 3000-rect soup (tests/test_gpu_random_scene.py's): its BVH nodes
    exceed LDS, so form 5 reads nodes and records through L1/L2 (placement 0);
    the grid search with its index in LDS, and all-global."""
    from mirror_maze import default_uniform, make_ext
    from test_gpu_random_scene import random_scene

    opts, form, modes = {"auto-grid": ({}, 11, (11, 12)), "bvh-li": ({7: 5}, 5, (0,)),
                         "grid-global": ({7: 11, 1: 0}, 11, (13,))}[case]
    s = random_scene(3000, 7, False)
    u = default_uniform(1920, 1080, 0)
    e = make_ext(8, 8, 8, frame=3)
    px = _scattered((1920, 1080), 40, seed=3000)
    auto = _renderer(s)
    want = _tile_ref(auto, u, e, px)
    auto.close()
    r = _renderer(s, opts)
    got, _ = r.trace_pixels(u, e, px)
    assert _diff(got.cpu().numpy(), want) == 0
    assert r.scene_info(MM_INFO_LAST_FORM) == form and r.scene_info(MM_INFO_LAST_LDS_MODE) in modes
    r.close()


def test_flags(case1):
    """5. RGBA8 is quantize() of the float result; two MM_EXT_ACCUMULATE calls
    with frames 3 and 4 give the sum of the two plain results and alpha 2."""
    import torch

    from mirror_maze import MM_EXT_ACCUMULATE, make_ext

    s, u, e = case1[:3]
    px = _window_list(seed=5)
    r = _renderer(s)
    f32, _ = r.trace_pixels(u, e, px)
    u8, _ = r.trace_pixels(u, e, px, rgba8=True)
    assert u8.dtype == torch.uint8 and u8.shape == (185, 4)
    assert torch.equal(u8, r.quantize(f32)) and int(u8[:, :3].max()) > 0 and int(u8[:, 3].min()) == 255
    plain = [r.trace_pixels(u, make_ext(8, 8, 8, frame=f), px)[0].cpu().numpy() for f in (3, 4)]
    acc = torch.zeros((185, 4), dtype=torch.float32, device="cuda")
    for f in (3, 4):
        r.trace_pixels(u, make_ext(8, 8, 8, frame=f, flags=MM_EXT_ACCUMULATE), px, out=acc)
    want = (np.zeros_like(plain[0]) + plain[0]) + plain[1]
    assert np.array_equal(_bits(acc.cpu().numpy()), _bits(want))
    assert (want[:, 3] == 2.0).all() and not np.array_equal(plain[0], plain[1])
    r.close()


OUTSIDE = [(VIEW[0], 0), (0, VIEW[1]), (2**31, 2**31)]


@pytest.mark.parametrize("case", ["fused-8", "staged-3", "staged-24", "unfused-2", "unfused-8", "reference-8"])
def test_entries_outside_the_view(case1, case):
    """6. (view_w, 0), (0, view_h) and (2^31, 2^31) between valid entries: zero
    (untouched with MM_EXT_ACCUMULATE, 0 in RGBA8), not counted, and the valid
    entries are what they are without them -- through the fused resolve and
    each resolve kernel."""
    import torch

    from mirror_maze import MM_EXT_ACCUMULATE, MM_PIPE_REFERENCE, make_ext

    spp = int(case.split("-")[1])
    opts = {12: 0} if case.startswith("unfused") else {}
    s, u = case1[0], case1[1]
    e = make_ext(spp, 8, 8, frame=6)
    valid = _window_list(seed=6)[:70]
    # outside entries first, last, and at chunk-interior positions
    where = [0, 9, 40]
    px = valid.astype(np.int64)
    for k, o in zip(where, OUTSIDE):
        px = np.insert(px, k, o, axis=0)
    px = np.concatenate([px, [OUTSIDE[2]]])
    px = np.ascontiguousarray(px.astype(np.uint32))
    out_idx = np.array([k for k, p in enumerate(px) if p[0] >= VIEW[0] or p[1] >= VIEW[1]])
    in_idx = np.setdiff1d(np.arange(len(px)), out_idx)
    assert len(out_idx) == 4 and len(in_idx) == 70
    r = _renderer(s, opts, MM_PIPE_REFERENCE if case.startswith("reference") else 0)
    alone, st0 = r.trace_pixels(u, e, valid, stats=True)
    got, st = r.trace_pixels(u, e, px, out=torch.full((len(px), 4), 7.0, device="cuda"), stats=True)
    got = got.cpu().numpy()
    assert (_bits(got[out_idx]) == 0).all()
    assert _diff(got[in_idx], alone.cpu().numpy()) == 0
    assert (st.paths, st.rays) == (st0.paths, st0.rays) == (70 * spp, st0.rays)
    u8, _ = r.trace_pixels(u, e, px, out=torch.full((len(px), 4), 9, dtype=torch.uint8, device="cuda"))
    u8 = u8.cpu().numpy()
    assert (u8[out_idx] == 0).all() and np.array_equal(u8[in_idx], r.quantize(alone).cpu().numpy())
    acc = torch.full((len(px), 4), 7.0, device="cuda")
    r.trace_pixels(u, make_ext(spp, 8, 8, frame=6, flags=MM_EXT_ACCUMULATE), px, out=acc)
    acc = acc.cpu().numpy()
    assert (acc[out_idx] == 7.0).all()
    want = np.float32(7.0) + alone.cpu().numpy()
    assert np.array_equal(_bits(acc[in_idx]), _bits(want))
    r.close()


def test_arguments(case1):
    """7. Every refusal, n_pixels = 0, no scene; then a valid call still
    matches the oracle."""
    import torch

    from mirror_maze import lib, make_ext
    from mirror_maze._lib import (MM_ERR_INVALID, MM_ERR_NO_SCENE, MM_EXT_ACCUMULATE, MM_EXT_RGBA8, MM_OK,
                                  mm_uniform)

    s, u, e = case1[:3]
    r = _renderer(s)
    px = torch.from_numpy(_window_list().view(np.int32)).cuda()
    out = torch.zeros((186, 4), dtype=torch.float32, device="cuda")
    P = C.c_void_p

    def raw(uni=u, ext=e, pixels=px.data_ptr(), n=185, dst=out.data_ptr(), ctx=None):
        return lib().mm_trace_pixels(ctx or r._ctx, C.byref(uni) if uni is not None else None,
                                     C.byref(ext) if ext is not None else None, P(pixels), n, P(dst), None)

    assert lib().mm_trace_pixels(None, C.byref(u), C.byref(e), P(px.data_ptr()), 185, P(out.data_ptr()),
                                 None) == MM_ERR_INVALID
    for kw in (dict(uni=None), dict(ext=None), dict(pixels=None), dict(dst=None)):
        assert raw(**kw) == MM_ERR_INVALID, kw
    assert raw(pixels=px.data_ptr() + 4) == MM_ERR_INVALID
    assert raw(dst=out.data_ptr() + 4) == MM_ERR_INVALID
    assert raw(ext=make_ext(8, 8, 8, flags=MM_EXT_RGBA8), dst=out.data_ptr() + 2) == MM_ERR_INVALID
    assert raw(ext=make_ext(8, 8, 8, flags=MM_EXT_RGBA8), dst=out.data_ptr() + 4, n=1) == MM_OK  # 4-byte pixels
    n_ok = 1
    for bad in (make_ext(0, 8, 8), make_ext(4097, 8, 8), make_ext(8, 32768, 8), make_ext(8, 8, 32768),
                make_ext(8, 8, 8, flags=MM_EXT_RGBA8 | MM_EXT_ACCUMULATE)):
        assert raw(ext=bad) == MM_ERR_INVALID, bytes(bad)
    bad_view = mm_uniform.from_buffer_copy(u)
    bad_view.view_w = 0.0
    assert raw(uni=bad_view) == MM_ERR_INVALID
    # the 32-bit queue: chunks padded to 64, less the 2^24 the last claims may overshoot (nothing is read)
    assert raw(ext=make_ext(4096, 8, 8), n=2**20) == MM_ERR_INVALID
    assert raw(ext=make_ext(1, 8, 8), n=2**32 - 2**24) == MM_ERR_INVALID
    assert raw(ext=make_ext(1, 8, 8), n=2**40) == MM_ERR_INVALID
    # staged samples: 2^29 paths
    assert raw(ext=make_ext(3, 8, 8), n=2**29 // 3 + 1) == MM_ERR_INVALID
    r.set_option(12, 0)
    assert raw(ext=make_ext(8, 8, 8), n=2**26 + 1) == MM_ERR_INVALID
    r.set_option(12, 1)
    assert r.last_call() == n_ok
    assert raw(n=0) == MM_OK and raw(n=0, pixels=None, dst=None) == MM_OK
    assert r.last_call() == n_ok  # no call number taken
    r.sync()
    empty, st = r.trace_pixels(u, e, np.zeros((0, 2), np.uint32), stats=True)
    assert empty.shape == (0, 4) and r.last_call() == n_ok
    bare = _renderer(None)
    assert raw(ctx=bare._ctx) == MM_ERR_NO_SCENE
    bare.close()
    _check_case1(r, case1)
    assert r.last_call() == n_ok + 1
    r.close()
