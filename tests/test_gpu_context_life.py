"""What one context carries from call to call: the work-queue words, the staged samples, the tail records, the
stats and error words, the scene buffers and the facts derived from them -- across streams, scene swaps and
failed calls.  The other GPU tests build a fresh Renderer, upload one scene, stay on one stream and look at
each result before the next call; here one context is kept, moved between two streams with no sync in between
(the library orders its launches: mm_api.h, "One context, several streams"), given one scene after another, and
used again after calls that failed or were refused.

Every comparison is on all 32 bits.  Outputs that a skipped launch would leave untouched are pre-filled with
NaN, allocated and synchronised before the streams are used.  The oracle's references are computed once per
module; a 64 x 32 tile's reference is the top-left corner of the same frame's 128 x 64 reference (a pixel's
value depends on its own (pixel, sample, frame) only).

128 x 64 x 8 spp is 1024 chunks: blocks with several waves, the smallest shape at which the rings can go wrong
(tests/test_gpu_predraw.py)."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import aov_support as A
from conftest import GOLDEN, oracle_tile

pytestmark = pytest.mark.gpu

MM_OPT_DEFER, MM_OPT_DEFER_MIN, MM_OPT_FAULT_INJECT, MM_OPT_GRID_CELL = 21, 22, 23, 25
DEFER_MIN_DEFAULT = 1 << 24
MM_INFO_GRID_CELLS_X, MM_INFO_GRID_CELLS_Z = 2, 4
MM_INFO_LAST_LDS_MODE, MM_INFO_LAST_KERNEL_FORM, MM_INFO_LAST_RING = 12, 22, 23
FACTS = (*range(1, 11), 13, 18, 19, 20, 21)  # MM_INFO_*: what an upload derives from the scene
LAST = (MM_INFO_LAST_KERNEL_FORM, MM_INFO_LAST_LDS_MODE, MM_INFO_LAST_RING)
VIEW = (640, 480)
ORIGIN = (288, 224)  # the horizon down the corridors
SOUP = (312, 144)    # five of the soup's rects and their edges: at (0, 0) and ORIGIN every path of S and B misses
WINDOWS = ((0, 0), ORIGIN, SOUP)
BIG, SMALL, TINY = (128, 64), (64, 32), (32, 16)
RINGS = {MM_OPT_DEFER: 32, MM_OPT_DEFER_MIN: 0}
BL = ML = 8
AOV_LIMIT = 15
NAMES = ("normal_depth", "albedo", "id")


def _bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint32)


def _same(got, ref):
    g, r = _bits(got), _bits(ref)
    return g.shape == r.shape and bool((g == r).all())


def _u():
    from mirror_maze import default_uniform

    return default_uniform(*VIEW, 0)


def _ext(spp, frame):
    from mirror_maze import make_ext

    return make_ext(spp, BL, ML, frame=frame)


# ---- scenes and references -----------------------------------------------------
@functools.lru_cache(maxsize=None)
def _scene(name):
    """M: the N = 10 maze (a flat grid that sits whole in LDS and can run the rings); S: a 300-rect soup; B: the
    soup with a corner at 2^60, which has no grid and walks the BVH (test_gpu_random_scene.py)."""
    from mirror_maze import Scene
    from test_gpu_random_scene import random_scene

    if name == "M":
        return Scene.build(10, 0)
    s = random_scene(300, 5, False)
    if name == "S":
        return s
    rects = s.rects.copy()
    rects[0, 0:9] = np.float32([2.0**60 - 2.0**58, -8.0, 0.0, 2.0**58, 0.0, 0.0, 0.0, 16.0, 0.0])
    nodes, idx = Scene.bvh(rects)
    return Scene(0, rects, nodes, idx, s.is_mirror, s.emission, np.zeros((0, 0), np.uint8), 0)


@functools.lru_cache(maxsize=None)
def _oracle(name):
    from oracle.oracle import Oracle

    return Oracle.from_scene(_scene(name))


@functools.lru_cache(maxsize=None)
def _big_ref(name, spp, frame):
    """(the oracle's 128 x 64 tile at ORIGIN, its closest-hit queries), read-only."""
    ref, rays = oracle_tile(_oracle(name), _u(), _ext(spp, frame), *ORIGIN, *BIG)
    ref.setflags(write=False)
    return ref, rays


def _ref(name, spp, frame, size):
    """The oracle's tile of `size` at ORIGIN: the top-left corner of the frame's 128 x 64 reference."""
    w, h = size
    return _big_ref(name, spp, frame)[0][:h, :w]


@functools.lru_cache(maxsize=None)
def _tiny_ref(name, spp, frame, x0, y0):
    """(the oracle's 32 x 16 tile at (x0, y0), rays, paths), read-only."""
    ref, st = _oracle(name).trace_tile(_u(), _ext(spp, frame), x0, y0, *TINY)
    ref.setflags(write=False)
    return ref, st.rays, st.paths


@pytest.fixture(scope="module")
def ref_lib(tmp_path_factory):
    return A.build_ref(tmp_path_factory.mktemp("aov_ref"))


_AOV = {}


def _aov_ref(ref_lib, name):
    """(tests/aov_ref.c's buffers of the 32 x 16 tiles at ORIGIN and SOUP, its (t, k) of _query_rays()), once
    per scene."""
    if name not in _AOV:
        ref = A.Ref(ref_lib, _scene(name))
        _AOV[name] = ([ref.tile(_u(), AOV_LIMIT, *at, *TINY) for at in (ORIGIN, SOUP)], ref.query(_query_rays()))
    return _AOV[name]


@functools.lru_cache(maxsize=None)
def _query_rays():
    """64 rays (n, 2, 4) in random directions: 32 from points around the default camera (inside the maze), 32
    from points among the soup's rects."""
    rng = np.random.default_rng(2024)
    rays = np.zeros((64, 2, 4), np.float32)
    rays[:32, 0, :3] = np.float32([-5.0, 0.0, -45.0]) + rng.uniform(-4.0, 4.0, (32, 3)) * np.float32([1.0, 0.1, 1.0])
    rays[32:, 0, :3] = rng.uniform(-150.0, 150.0, (32, 3))
    d = rng.normal(size=(64, 3))
    rays[:, 1, :3] = d / np.linalg.norm(d, axis=1, keepdims=True)
    rays.setflags(write=False)
    return rays


@functools.lru_cache(maxsize=None)
def _pixel_list():
    """100 (x, y) entries inside the 128 x 64 window at ORIGIN, entries 90..97 duplicates of 0..7, entry 98
    outside the view (zeros), entry 99 the window's last pixel."""
    rng = np.random.default_rng(7)
    px = np.stack([ORIGIN[0] + rng.integers(0, BIG[0], 100), ORIGIN[1] + rng.integers(0, BIG[1], 100)], axis=1)
    px[90:98] = px[0:8]
    px[98] = (VIEW[0] + 3, 5)
    px[99] = (ORIGIN[0] + BIG[0] - 1, ORIGIN[1] + BIG[1] - 1)
    px = np.ascontiguousarray(px.astype(np.int32))
    px.setflags(write=False)
    return px


def _pixels_ref(name, spp, frame):
    """trace_pixels' result for _pixel_list() by the oracle: each entry its pixel of the window, zeros outside
    the view (mm_api.h)."""
    px = _pixel_list()
    big = _big_ref(name, spp, frame)[0]
    out = np.zeros((len(px), 4), np.float32)
    inside = px[:, 0] < VIEW[0]
    out[inside] = big[px[inside, 1] - ORIGIN[1], px[inside, 0] - ORIGIN[0]]
    return out


@functools.lru_cache(maxsize=None)
def _ray_list():
    """128 mm_trace_rays records (origin, key bits, direction, -) from the default camera's centre."""
    rng = np.random.default_rng(11)
    rays = np.zeros((128, 8), np.float32)
    rays[:, 0:3] = np.float32([-5.0, 0.0, -45.0])
    d = rng.normal(size=(128, 3))
    rays[:, 4:7] = d / np.linalg.norm(d, axis=1, keepdims=True)
    rays.view(np.uint32)[:, 3] = rng.integers(0, 2**32, 128, dtype=np.uint64).astype(np.uint32)
    rays.setflags(write=False)
    return rays


def _renderer(name=None, opts=None):
    from mirror_maze import Renderer

    r = Renderer(0)
    for k, v in (opts or {}).items():
        r.set_option(k, v)
    if name is not None:
        r.upload_scene(_scene(name))
    return r


def _nan(*shape):
    import torch

    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def _facts(r):
    return {k: r.scene_info(k) for k in FACTS}


def _last(r):
    return tuple(r.scene_info(k) for k in LAST)


# ---- a: two streams, tile calls ---------------------------------------------------
@pytest.mark.parametrize("opts", [{}, RINGS], ids=["default", "rings"])
def test_tile_calls_alternating_between_two_streams(gpu, opts):
    """Six trace_tile calls alternating between two streams with no sync between them, 128 x 64 x 8 spp and
    64 x 32 x 3 spp in turn, call i with frame i: a launch that starts while the one before it still runs would
    find the shared queue head past its own length and claim nothing -- its NaN would stay -- and the mixed
    waves-done count would leave a status word unpublished.  Every output equals the oracle and every call
    reads finished-clean.

    Never run against a library without the ordering, the parent commit included (what two launches on one set
    of queue words do to a GPU is not something to find out by trying): what the test is sensitive to rests on
    reading the kernel's dequeue and persistent_exit, a supposition, not a measurement."""
    import torch

    shapes = [(BIG, 8) if i % 2 == 0 else (SMALL, 3) for i in range(6)]
    refs = [_ref("M", spp, i, size) for i, (size, spp) in enumerate(shapes)]
    r = _renderer("M", opts)
    outs = [_nan(size[1], size[0], 4) for size, _ in shapes]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    calls = []
    for i, (size, spp) in enumerate(shapes):
        with torch.cuda.stream(streams[i & 1]):
            r.trace_tile(_u(), _ext(spp, i), *ORIGIN, *size, out=outs[i])
        calls.append(r.last_call())
    torch.cuda.synchronize()
    r.sync()
    assert calls == list(range(calls[0], calls[0] + 6))
    bad = [int((_bits(o) != _bits(ref)).sum()) for o, ref in zip(outs, refs)]
    assert bad == [0] * 6, bad
    assert [r.call_status(c) for c in calls] == [True] * 6
    r.close()


# ---- b: mixed kinds, one stream and two ---------------------------------------------
def _mixed_calls():
    """The six steps as (name, options set before it, call(r, outs) enqueuing into the buffers `outs`, the
    buffers' shapes and dtypes)."""
    import torch

    u = _u()
    f32, i32 = torch.float32, torch.int32
    dev = "cuda"
    px = torch.from_numpy(np.array(_pixel_list())).to(dev)
    rays = torch.from_numpy(np.array(_ray_list())).to(dev)
    qrays = torch.from_numpy(np.array(_query_rays())).to(dev)
    w, h = SMALL
    return [
        ("tile_var", {}, lambda r, o: r.trace_tile_var(u, _ext(12, 20), *ORIGIN, w, h, out=o[0], var=o[1]),
         [((h, w, 4), f32), ((h, w), f32)]),
        ("pixels", {}, lambda r, o: r.trace_pixels(u, _ext(24, 21), px, out=o[0]), [((100, 4), f32)]),
        ("rays", {}, lambda r, o: r.trace_rays(_ext(8, 22), rays, jitter=True, out=o[0], var=o[1]),
         [((128, 4), f32), ((128,), f32)]),
        ("aov", {}, lambda r, o: r.trace_aov(u, None, AOV_LIMIT, x0=ORIGIN[0], y0=ORIGIN[1], w=w, h=h,
                                             out=dict(zip(NAMES, o))),
         [((1, h, w, 4), f32), ((1, h, w, 4), f32), ((1, h, w), i32)]),
        ("query", {}, lambda r, o: r.query_rays(qrays, out=o[0]), [((64, 2), i32)]),
        # 2 x 128 x 64 x 3 staged samples: more than any call before it, so d_samples is regrown
        ("frames", {MM_OPT_DEFER_MIN: 0}, lambda r, o: r.trace_tile_frames(u, _ext(3, 23), 2, *ORIGIN, *BIG, out=o[0]),
         [((2, BIG[1], BIG[0], 4), f32)]),
        ("tile", {MM_OPT_DEFER_MIN: DEFER_MIN_DEFAULT}, lambda r, o: r.trace_tile(u, _ext(8, 25), *ORIGIN, w, h, out=o[0]),
         [((h, w, 4), f32)]),
    ]


def _buffers(spec):
    """NaN-filled float buffers, -1-filled integer ones."""
    import torch

    return [torch.full(shape, float("nan") if dt == torch.float32 else -1, dtype=dt, device="cuda")
            for shape, dt in spec]


_TWINS = {}


def _serial_twins(steps):
    """Each step alone on a fresh context with a sync after it: its buffers' bits, once per module."""
    import torch

    if not _TWINS:
        for name, opts, call, spec in steps:
            r = _renderer("M", opts)
            outs = _buffers(spec)
            torch.cuda.synchronize()
            call(r, outs)
            r.sync()
            torch.cuda.synchronize()
            _TWINS[name] = [_bits(o).copy() for o in outs]
            r.close()
    return _TWINS


@pytest.mark.parametrize("streams", [1, 2])
def test_mixed_calls_without_a_sync_equal_their_serial_twins(gpu, streams):
    """trace_tile_var, trace_pixels (duplicates, an entry outside the view), trace_rays with its variance,
    trace_aov, query_rays, a two-frame trace_tile_frames that forces the staged samples to be regrown, and a
    fused trace_tile, on one context with no host sync until the end -- on one stream, and alternating between
    two.  Each result equals the same call alone on a fresh context; the tiles equal the oracle too.  No call
    reads another's output, so the caller owes no wait_stream: what orders the calls is the library alone.

    streams = 2 was not run against a library without the ordering (see the two-stream tile test)."""
    import torch

    steps = _mixed_calls()
    twins = _serial_twins(steps)
    r = _renderer("M")
    outs = [_buffers(spec) for _, _, _, spec in steps]
    torch.cuda.synchronize()
    lanes = [torch.cuda.Stream() for _ in range(streams)]
    for i, (name, opts, call, _) in enumerate(steps):
        for k, v in opts.items():
            r.set_option(k, v)
        with torch.cuda.stream(lanes[i % streams]):
            call(r, outs[i])
    torch.cuda.synchronize()
    r.sync()
    r.close()
    got = {name: outs[i] for i, (name, _, _, _) in enumerate(steps)}
    differ = {name: [int((_bits(o) != t).sum()) for o, t in zip(got[name], twins[name])] for name in got}
    assert all(sum(v) == 0 for v in differ.values()), differ
    assert _same(got["tile_var"][0], _ref("M", 12, 20, SMALL))
    assert _same(got["frames"][0][0], _ref("M", 3, 23, BIG)) and _same(got["frames"][0][1], _ref("M", 3, 24, BIG))
    assert _same(got["tile"][0], _ref("M", 8, 25, SMALL))
    assert _same(got["pixels"][0], _pixels_ref("M", 24, 21))


# ---- c: parity mode beside a trace call ---------------------------------------------
def test_parity_mode_on_another_stream_than_the_trace_calls(gpu):
    """A 128 x 64 trace_tile with stats on stream a and a second one left running there, then compute_shader and
    read_texture on stream b (the raw mm_set_stream, as in test_gpu_binding.py): mm_trace_chunks zeroes the
    stats and error words and shares the status slots with the trace calls.  The framebuffer equals the
    committed parity fixture, the tiles and the first one's rays / paths the oracle.

    Not run against a library without the ordering (see the two-stream tile test)."""
    import torch

    from mirror_maze import default_uniform, lib

    g = np.load(GOLDEN / "oracle_p0.npz")
    r = _renderer("M")
    first, second = _nan(BIG[1], BIG[0], 4), _nan(BIG[1], BIG[0], 4)
    torch.cuda.synchronize()
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(a):
        _, st = r.trace_tile(_u(), _ext(8, 0), *ORIGIN, *BIG, out=first, stats=True)
        r.trace_tile(_u(), _ext(8, 2), *ORIGIN, *BIG, out=second)
    r._check(lib().mm_set_stream(r._ctx, b.cuda_stream))
    r.compute_shader(default_uniform(1024, 768, 0), g["chunks"])
    f, _ = r.read_texture()
    torch.cuda.synchronize()
    r.sync()
    assert np.array_equal(_bits(f[g["ys"], g["xs"], :3]), _bits(g["rgb_t0"]))
    ref, rays = _big_ref("M", 8, 0)
    assert _same(first, ref) and (st.rays, st.paths) == (rays, BIG[0] * BIG[1] * 8)
    assert _same(second, _big_ref("M", 8, 2)[0])
    r.close()


# ---- d: scene swaps -------------------------------------------------------------------
def _exercise(r, name, ref_lib):
    """What tests d, f and g ask of a context holding scene `name`: the facts; 32 x 16 tiles at WINDOWS with 8
    and 3 spp, 32 x 16 trace_aov tiles at ORIGIN and SOUP and 64 query_rays, each equal to its reference, with
    the stats' rays / paths; returns (facts, the launch records after every trace call)."""
    import torch

    facts = _facts(r)
    last = []
    for (x0, y0) in WINDOWS:
        for spp in (8, 3):
            got, st = r.trace_tile(_u(), _ext(spp, 3), x0, y0, *TINY, out=_nan(TINY[1], TINY[0], 4), stats=True)
            ref, rays, paths = _tiny_ref(name, spp, 3, x0, y0)
            assert _same(got, ref), (name, x0, y0, spp)
            assert (st.rays, st.paths) == (rays, paths), (name, x0, y0, spp)
            last.append(_last(r))
    aov_refs, (t_ref, k_ref) = _aov_ref(ref_lib, name)
    gots = [r.trace_aov(_u(), None, AOV_LIMIT, x0=x0, y0=y0, w=TINY[0], h=TINY[1]) for (x0, y0) in (ORIGIN, SOUP)]
    t, k = r.query_rays(torch.from_numpy(np.array(_query_rays())).cuda())
    r.sync()
    for got, ref in zip(gots, aov_refs):
        assert {n: int((_bits(got[n])[0] != _bits(ref[n])).sum()) for n in NAMES} == dict.fromkeys(NAMES, 0), name
    assert _same(t, t_ref) and _same(k, k_ref), name
    return facts, last


_FRESH = {}


def _fresh(name, ref_lib, opts=None):
    """_exercise on a fresh context that has only ever held `name`."""
    key = (name, tuple(sorted((opts or {}).items())))
    if key not in _FRESH:
        r = _renderer(name, opts)
        _FRESH[key] = _exercise(r, name, ref_lib)
        r.close()
    return _FRESH[key]


def test_scene_swaps_on_one_context(gpu, ref_lib):
    """M, then S, then B, then M again on one context: after every upload the facts (MM_INFO 1-10, 13, 18-21)
    and the launch records (kernel form, LDS mode, ring) are a fresh context's for that scene, and tiles, AOVs
    and ray queries equal their references -- nothing of the grid, the lean flag or the record counts of the
    scene before is left."""
    r = _renderer()
    for name in ("M", "S", "B", "M"):
        r.upload_scene(_scene(name))
        assert _exercise(r, name, ref_lib) == _fresh(name, ref_lib), name
    assert _fresh("M", ref_lib)[0] != _fresh("S", ref_lib)[0] != _fresh("B", ref_lib)[0]
    assert _fresh("M", ref_lib)[0][1] == 1.0 and _fresh("B", ref_lib)[0][1] == 0.0  # MM_INFO_GRID_OK
    r.close()


# ---- e: upload with work in flight ------------------------------------------------------
def test_upload_with_a_launch_still_running(gpu):
    """A 128 x 64 trace of M with the rings forced, no sync, and S uploaded at once: the upload waits for the
    context's queued work before it frees M's buffers, so the first result is oracle(M)'s and a trace after
    the upload oracle(S)'s (at SOUP, where S is hit and the two scenes differ)."""
    import torch

    r = _renderer("M", RINGS)
    first, second = _nan(BIG[1], BIG[0], 4), _nan(TINY[1], TINY[0], 4)
    torch.cuda.synchronize()
    r.trace_tile(_u(), _ext(8, 1), *ORIGIN, *BIG, out=first)
    r.upload_scene(_scene("S"))
    r.trace_tile(_u(), _ext(8, 3), *SOUP, *TINY, out=second)
    r.sync()
    assert _same(first, _big_ref("M", 8, 1)[0])
    assert _same(second, _tiny_ref("S", 8, 3, *SOUP)[0])
    assert not _same(second, _tiny_ref("M", 8, 3, *SOUP)[0])
    r.close()


# ---- f: options read at upload ----------------------------------------------------------
def test_grid_options_act_at_the_next_upload(gpu, ref_lib):
    """MM_OPT_GRID_CELL set with M uploaded changes nothing until M is uploaded again; then the cell counts are
    a fresh context's at that cell size, and the traces stay exact before and after."""
    r = _renderer("M")
    before = _facts(r)
    r.set_option(MM_OPT_GRID_CELL, 200)
    assert _exercise(r, "M", ref_lib) == _fresh("M", ref_lib)
    assert _facts(r) == before
    r.upload_scene(_scene("M"))
    at_200 = _fresh("M", ref_lib, {MM_OPT_GRID_CELL: 200})
    assert _exercise(r, "M", ref_lib) == at_200
    cells = (MM_INFO_GRID_CELLS_X, MM_INFO_GRID_CELLS_Z)
    assert all(_facts(r)[k] != before[k] for k in cells), (before, _facts(r))
    assert all(_facts(r)[k] == at_200[0][k] for k in cells)
    r.close()


# ---- g: a refused upload keeps the scene ----------------------------------------------
def _raw_upload(r, rects, n_rects, nodes, n_nodes, idx, mats, emis):
    from mirror_maze import lib

    arrays = [np.ascontiguousarray(rects, dtype=np.float32), np.ascontiguousarray(nodes),
              np.ascontiguousarray(idx, dtype=np.uint32), np.ascontiguousarray(mats, dtype=np.uint8),
              np.ascontiguousarray(emis, dtype=np.float32)]
    rc = lib().mm_upload_scene(r._ctx, arrays[0].ctypes.data, n_rects, arrays[1].ctypes.data, n_nodes,
                               arrays[2].ctypes.data, arrays[3].ctypes.data, arrays[4].ctypes.data)
    return rc, lib().mm_last_error(r._ctx).decode()


def test_a_refused_upload_keeps_the_scene(gpu, ref_lib):
    """Three uploads the argument checks refuse -- an index out of range, more than 2n - 1 nodes
    (MM_ERR_INVALID), a leaf of 256 planes (MM_ERR_UNSUPPORTED; from the 300-rect soup, whose 256 rects such a
    leaf can hold) -- each leave M in place: the facts unchanged, tiles, AOVs and queries exact (mm_api.h,
    mm_upload_scene)."""
    from mirror_maze._lib import MM_ERR_INVALID, MM_ERR_UNSUPPORTED

    m, s = _scene("M"), _scene("S")
    r = _renderer("M")
    fresh = _fresh("M", ref_lib)
    assert _exercise(r, "M", ref_lib) == fresh
    bad_idx = np.array(m.idx, dtype=np.uint32)
    bad_idx[0] = m.n_rects
    big_leaf = np.array(s.nodes)
    leaf = int(np.flatnonzero(big_leaf["count"] > 0)[0])
    big_leaf[leaf]["left_first"], big_leaf[leaf]["count"] = 0, 256
    assert s.n_rects >= 256
    refusals = [
        (MM_ERR_INVALID, (m.rects, m.n_rects, m.nodes, len(m.nodes), bad_idx, m.is_mirror, m.emission)),
        (MM_ERR_INVALID, (m.rects, m.n_rects, m.nodes, 2 * m.n_rects + 1, m.idx, m.is_mirror, m.emission)),
        (MM_ERR_UNSUPPORTED, (s.rects, s.n_rects, big_leaf, len(big_leaf), s.idx, s.is_mirror, s.emission)),
    ]
    for code, args in refusals:
        rc, err = _raw_upload(r, *args)
        assert rc == code and rc < 0 and err.startswith("mm_upload_scene:"), (rc, err)
        assert _exercise(r, "M", ref_lib) == fresh, err
    r.close()


# ---- h: the call after a failed call is exact --------------------------------------------
@pytest.mark.parametrize("kind", ["tile-rings", "pixels", "rays"])
def test_the_call_after_a_failed_call_is_exact(gpu, kind):
    """MM_OPT_FAULT_INJECT 1 (the error-path switch, as in test_gpu_pixel_lists.py) fails one call, which is
    reported by name; with the switch off, the next call -- of another kind -- equals the oracle: the failed
    launch left the queue words, the staged samples, the tail rings and the error word as a clean one does."""
    import torch

    from mirror_maze import MMError

    r = _renderer("M", RINGS if kind == "tile-rings" else None)
    px = torch.from_numpy(np.array(_pixel_list())).cuda()
    rays = torch.from_numpy(np.array(_ray_list())).cuda()
    out = _nan(100, 4) if kind == "tile-rings" else _nan(SMALL[1], SMALL[0], 4)
    torch.cuda.synchronize()
    r.set_option(MM_OPT_FAULT_INJECT, 1)
    if kind == "tile-rings":
        r.trace_tile(_u(), _ext(8, 4), *ORIGIN, *BIG)
        what = "(mm_trace_tile, "
    elif kind == "pixels":
        r.trace_pixels(_u(), _ext(24, 4), px)
        what = "(mm_trace_pixels, "
    else:
        r.trace_rays(_ext(8, 4), rays, jitter=True, var=True)
        what = "(mm_trace_rays, "
    failed = r.last_call()
    r.set_option(MM_OPT_FAULT_INJECT, 0)
    with pytest.raises(MMError) as ei:
        r.sync()
    assert f"call #{failed} {what}" in str(ei.value) and "injected fault" in str(ei.value), str(ei.value)
    if kind == "tile-rings":
        r.trace_pixels(_u(), _ext(8, 5), px, out=out)
        ref = _pixels_ref("M", 8, 5)
    else:
        r.trace_tile(_u(), _ext(8, 5), *ORIGIN, *SMALL, out=out)
        ref = _ref("M", 8, 5, SMALL)
    r.sync()
    assert r.call_status(r.last_call()) is True and r.last_call() == failed + 1
    assert _same(out, ref)
    r.close()
