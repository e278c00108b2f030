"""Pixel lists of many frames in one launch (mm_trace_pixel_lists, Renderer.trace_pixel_lists /
refine_frames).  The reference of every comparison is mm_trace_pixels (mm_trace_pixels_var for the variance
call) called once per list with that list's camera and RNG frame, on a context with the default options; those
calls are pinned to the oracle by tests/test_gpu_trace_pixels.py and tests/test_gpu_variance.py.  Every
comparison is on float bits, zero differing entries."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import aov_support as A
import topup_support as TU

pytestmark = pytest.mark.gpu

MM_INFO_LAST_FORM, MM_INFO_LAST_LDS_MODE, MM_INFO_LAST_DEFER = 11, 12, 14
MM_OPT_LDS_NODES, MM_OPT_TRAVERSAL, MM_OPT_FUSE_RESOLVE = 1, 7, 12
VIEW = TU.WALK_VIEW  # 160 x 120
# 0, 1, 8 and 9 entries, an empty list, a long one: at 8 spp lists 1 and 2 are one chunk each and list 3 two, so
# a claim of four chunks spans cameras 1, 2 and 3 and starts the next in list 5
LENGTHS = [0, 1, 8, 9, 0, 200]
KEYS = [2**20 + 7, 5, 2**20 + 64 * 3 + 1, 9000, 77, 2**31 + 11]  # not consecutive


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if np.asarray(a).dtype == np.float32 else np.asarray(a).dtype)


def _diff(got, ref):
    g, r = _bits(got), _bits(ref)
    assert g.shape == r.shape, (g.shape, r.shape)
    return int((g != r).reshape(len(g), -1).any(axis=-1).sum()) if len(g) else 0


def _np(t):
    return t.cpu().numpy()


def _renderer(scene, opts=None, pipe=0):
    from mirror_maze import Renderer

    r = Renderer(0)
    r.set_pipeline(pipe)
    for k, v in (opts or {}).items():
        r.set_option(k, v)
    if scene is not None:
        r.upload_scene(scene)
    return r


def _cameras(base, n):
    """n distinct cameras near the (10,) record `base`: a few centimetres apart."""
    cams = np.tile(np.ascontiguousarray(base, dtype=np.float32), (n, 1))
    for f in range(n):
        cams[f, 0] += np.float32(0.011 * f)
        cams[f, 2] += np.float32(0.017 * f)
    return cams


def _lists(lengths, view, seed):
    """((N, 2) uint32 pixels of the view, seeded; offsets)."""
    rng = np.random.default_rng(seed)
    n = int(sum(lengths))
    px = np.stack([rng.integers(0, view[0], n), rng.integers(0, view[1], n)], axis=1).astype(np.uint32)
    return np.ascontiguousarray(px), np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)


def _with_cam(u, cam10):
    from mirror_maze import mm_camera, mm_uniform

    v = mm_uniform.from_buffer_copy(bytes(u))
    v.cam = mm_camera.from_buffer_copy(np.ascontiguousarray(cam10, dtype=np.float32).tobytes())
    return v


def _per_list(r, u, cams, e, keys, px, offs, var=False, rgba8=False, out=None):
    """What one mm_trace_pixels[_var] call per list gives: (out, var or None, rays, paths)."""
    from mirror_maze import make_ext

    outs, vars_, rays, paths = [], [], 0, 0
    for f in range(len(offs) - 1):
        a, b = int(offs[f]), int(offs[f + 1])
        uf = u if cams is None else _with_cam(u, cams[f])
        ef = make_ext(e.spp, e.bounce_limit, e.mirror_limit, frame=(e.frame + f if keys is None else int(keys[f])),
                      flags=e.flags)
        o = None if out is None else out[a:b]
        if var:
            o, v, st = r.trace_pixels_var(uf, ef, px[a:b], out=o, stats=True, rgba8=rgba8)
            vars_.append(_np(v))
        else:
            o, st = r.trace_pixels(uf, ef, px[a:b], out=o, stats=True, rgba8=rgba8)
        outs.append(_np(o))
        if b > a:
            rays, paths = rays + st.rays, paths + st.paths
    return np.concatenate(outs), (np.concatenate(vars_) if var else None), rays, paths


@pytest.fixture(scope="module")
def maze(gpu):
    """The N=4 maze at 160x120 from inside (the walk's first camera), six cameras, and a context with the
    default options for the references."""
    from mirror_maze import Scene, default_uniform

    s = Scene.build(4, 0)
    cams = _cameras(TU.walk_cameras()[0], 6)
    cams[4:] = _cameras(TU.walk_cameras()[3], 2)  # two of them turned
    u = _with_cam(default_uniform(*VIEW, 0), cams[0])
    ref = _renderer(s)
    yield s, u, cams, ref
    ref.close()


def _scene_case(name, maze):
    from mirror_maze import default_uniform

    if name == "maze":
        s, u, cams, _ = maze
        return s, u, cams
    if name == "corridor":
        s, u = A.corridor()
        return s, u, _cameras(np.frombuffer(bytes(u.cam), dtype=np.float32), 6)
    from test_gpu_random_scene import random_scene

    u = default_uniform(320, 180, 0)
    return random_scene(3000, 7, False), u, _cameras(np.frombuffer(bytes(u.cam), dtype=np.float32), 6)


@pytest.mark.parametrize("name", ["maze", "corridor", "soup"])
def test_six_lists_six_cameras(maze, name):
    """0, 1, 8, 9, 0 and 200 entries with six cameras and keys that are not consecutive: every entry is its own
    list call's, the stats are the calls' sums, and it is one launch under one call number."""
    from mirror_maze import make_ext

    s, u, cams = _scene_case(name, maze)
    view = (int(u.view_w), int(u.view_h))
    px, offs = _lists(LENGTHS, view, seed=1)
    e = make_ext(8, 8, 8, frame=3)
    r = _renderer(s)
    want, _, rays, paths = _per_list(r, u, cams, e, KEYS, px, offs)
    calls = r.last_call()
    got, var, st = r.trace_pixel_lists(u, cams, e, px, offs, frame_keys=KEYS, stats=True)
    assert var is None and tuple(got.shape) == (218, 4)
    assert _diff(_np(got), want) == 0
    assert (st.rays, st.paths) == (rays, paths) and paths == 218 * 8
    assert r.last_call() == calls + 1 and r.last_timing()[1] == 1
    assert r.scene_info(MM_INFO_LAST_DEFER) == 0
    # the cameras and keys matter: neighbouring lists' results differ from each other's references
    other, _, _, _ = _per_list(r, u, cams[::-1].copy(), e, KEYS[::-1], px, offs)
    assert _diff(other, want) > 20
    r.close()


def test_one_list_null_cameras_null_keys_and_many_short_lists(maze):
    """n_lists = 1; cams = NULL (uni->cam everywhere); frame_keys = NULL (ext->frame + f); 300 lists of 0..3
    entries (the search's depth, runs of empty lists)."""
    from mirror_maze import make_ext

    s, u, cams, ref = maze
    e = make_ext(8, 8, 8, frame=40)
    r = _renderer(s)
    px, offs = _lists([185], VIEW, seed=2)
    want, _, _, _ = _per_list(ref, u, cams[2:3], e, [123], px, offs)
    got, _, _ = r.trace_pixel_lists(u, cams[2:3], e, px, offs, frame_keys=[123])
    assert _diff(_np(got), want) == 0
    px, offs = _lists(LENGTHS, VIEW, seed=3)
    want, _, _, _ = _per_list(ref, u, None, e, KEYS, px, offs)
    got, _, _ = r.trace_pixel_lists(u, None, e, px, offs, frame_keys=KEYS)
    assert _diff(_np(got), want) == 0
    want, _, _, _ = _per_list(ref, u, cams, e, None, px, offs)
    got, _, _ = r.trace_pixel_lists(u, cams, e, px, offs)
    assert _diff(_np(got), want) == 0
    lengths = np.random.default_rng(300).integers(0, 4, 300).tolist()
    assert lengths.count(0) > 30
    px, offs = _lists(lengths, VIEW, seed=4)
    cams300 = _cameras(cams[0], 300)
    keys300 = (np.arange(300, dtype=np.uint32) * 64 + 2**20).tolist()
    want, _, rays, paths = _per_list(ref, u, cams300, e, keys300, px, offs)
    got, _, st = r.trace_pixel_lists(u, cams300, e, px, offs, frame_keys=keys300, stats=True)
    assert _diff(_np(got), want) == 0 and (st.rays, st.paths) == (rays, paths)
    r.close()


def _edge_lists():
    """Four lists whose first and last entries lie outside the view or repeat another entry."""
    W, H = VIEW
    inside, _ = _lists([30], VIEW, seed=5)
    inside = inside.astype(np.int64)
    lists = [
        np.concatenate([[[W, 0]], inside[0:7], [[2**31, 2**31]]]),        # outside first and last
        np.concatenate([inside[3:4], inside[7:12], inside[3:4]]),          # the same pixel first and last
        np.concatenate([[[0, H]], [[0, H]]]),                              # nothing but outside entries
        np.concatenate([inside[12:30], inside[12:13], [[W - 1, H - 1]], [[2**32 - 1, 5]]]),
    ]
    px = np.ascontiguousarray(np.concatenate(lists).astype(np.uint32))
    offs = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.uint64)
    outside = (px[:, 0] >= W) | (px[:, 1] >= H)
    return px, offs, outside


@pytest.mark.parametrize("case", ["fused-8", "staged-3", "staged-24", "unfused-2", "unfused-8"])
def test_duplicates_and_entries_outside_the_view(maze, case):
    """Entries outside the view and duplicates in the first and last position of a list, through the fused
    resolve and each resolve kernel: float, RGBA8 and MM_EXT_ACCUMULATE on a pre-filled out."""
    import torch

    from mirror_maze import MM_EXT_ACCUMULATE, make_ext

    s, u, cams, ref = maze
    spp = int(case.split("-")[1])
    r = _renderer(s, {MM_OPT_FUSE_RESOLVE: 0} if case.startswith("unfused") else {})
    px, offs, outside = _edge_lists()
    assert outside.sum() == 5 and outside[0] and outside[int(offs[1]) - 1] and outside[-1]
    keys = KEYS[:4]
    e = make_ext(spp, 8, 8, frame=6)
    want, _, rays, paths = _per_list(ref, u, cams[:4], e, keys, px, offs)
    got, _, st = r.trace_pixel_lists(u, cams[:4], e, px, offs, frame_keys=keys, stats=True,
                                     out=torch.full((len(px), 4), 7.0, device="cuda"))
    got = _np(got)
    assert _diff(got, want) == 0 and (_bits(got[outside]) == 0).all() and (got[~outside][:, 3] == 1.0).all()
    assert (st.rays, st.paths) == (rays, paths) and paths == int((~outside).sum()) * spp
    a, b = int(offs[1]), int(offs[2])
    assert got[a].tobytes() == got[b - 1].tobytes()  # the duplicate
    u8, _, _ = r.trace_pixel_lists(u, cams[:4], e, px, offs, frame_keys=keys,
                                   out=torch.full((len(px), 4), 9, dtype=torch.uint8, device="cuda"))
    want8, _, _, _ = _per_list(ref, u, cams[:4], e, keys, px, offs, rgba8=True)
    assert np.array_equal(_np(u8), want8) and (_np(u8)[outside] == 0).all()
    ea = make_ext(spp, 8, 8, frame=6, flags=MM_EXT_ACCUMULATE)
    acc = torch.full((len(px), 4), 7.0, device="cuda")
    r.trace_pixel_lists(u, cams[:4], ea, px, offs, frame_keys=keys, out=acc)
    acc_ref = torch.full((len(px), 4), 7.0, device="cuda")
    _per_list(ref, u, cams[:4], ea, keys, px, offs, out=acc_ref)
    assert _diff(_np(acc), _np(acc_ref)) == 0
    assert (_np(acc)[outside] == 7.0).all() and (_np(acc)[~outside][:, 3] == 8.0).all()
    r.close()


@pytest.mark.parametrize("spp,fuse", [(1, 1), (3, 1), (8, 1), (24, 1), (64, 1), (128, 1), (1, 0), (4, 0), (8, 0)],
                         ids=["1", "3", "8", "24", "64", "128", "1-unfused", "4-unfused", "8-unfused"])
def test_every_resolve(maze, spp, fuse):
    """spp 1, 8 and 64 through the fused resolve, 3 (left to right) and 24, 128 (blocks of 8) staged, and the
    three resolve kernels with MM_OPT_FUSE_RESOLVE 0: one launch or two."""
    from mirror_maze import make_ext

    s, u, cams, ref = maze
    e = make_ext(spp, 8, 8, frame=9)
    px, offs = _lists(LENGTHS, VIEW, seed=10 + spp)
    want, _, rays, paths = _per_list(ref, u, cams, e, KEYS, px, offs)
    r = _renderer(s, {MM_OPT_FUSE_RESOLVE: fuse})
    got, _, st = r.trace_pixel_lists(u, cams, e, px, offs, frame_keys=KEYS, stats=True)
    assert _diff(_np(got), want) == 0, spp
    assert (st.rays, st.paths) == (rays, paths) and paths == 218 * spp
    assert r.last_timing()[1] == (1 if fuse and 64 % spp == 0 else 2)
    r.close()


@pytest.mark.parametrize("spp", [2, 3, 8, 24])
def test_variance_call(maze, spp):
    """var_dev set: (out, var) are mm_trace_pixels_var's per list, entries outside the view included."""
    from mirror_maze import make_ext

    s, u, cams, ref = maze
    e = make_ext(spp, 8, 8, frame=12)
    r = _renderer(s)
    for px, offs, n in ((*_lists(LENGTHS, VIEW, seed=20 + spp), 6), (*_edge_lists()[:2], 4)):
        want, want_v, rays, paths = _per_list(ref, u, cams[:n], e, KEYS[:n], px, offs, var=True)
        got, got_v, st = r.trace_pixel_lists(u, cams[:n], e, px, offs, frame_keys=KEYS[:n], var=True, stats=True)
        assert _diff(_np(got), want) == 0 and np.array_equal(_bits(_np(got_v)), _bits(want_v))
        assert (st.rays, st.paths) == (rays, paths) and r.last_timing()[1] == 2
        assert float(want_v.max()) > 0
    u8, v8, _ = r.trace_pixel_lists(u, cams[:n], e, px, offs, frame_keys=KEYS[:n], var=True, rgba8=True)
    assert np.array_equal(_np(u8), _np(r.quantize(got))) and np.array_equal(_bits(_np(v8)), _bits(want_v))
    r.close()


def _raw(r, u, e, px, offs, out, cams=None, keys=None, n_lists=None, var=None, uni=True, ext=True):
    from mirror_maze import lib

    P = C.c_void_p
    return lib().mm_trace_pixel_lists(
        r._ctx, C.byref(u) if uni else None, None if cams is None else cams.ctypes.data, C.byref(e) if ext else None,
        None if keys is None else keys.ctypes.data, len(offs) - 1 if n_lists is None else n_lists, P(px),
        None if offs is None else offs.ctypes.data, P(out), P(var), None)


def test_variance_refusals(maze):
    """spp 1, MM_EXT_ACCUMULATE and a var_dev overlapping out_dev (or misaligned) are MM_ERR_INVALID; nothing is
    enqueued."""
    import torch

    from mirror_maze import MM_EXT_ACCUMULATE, lib, make_ext
    from mirror_maze._lib import MM_ERR_INVALID, MM_OK

    s, u, cams, ref = maze
    r = _renderer(s)
    pxh, offs = _lists([3, 0, 5], VIEW, seed=30)
    px = torch.from_numpy(pxh.view(np.int32)).cuda()
    out = torch.zeros((8, 4), dtype=torch.float32, device="cuda")
    var = torch.zeros((12,), dtype=torch.float32, device="cuda")
    good = make_ext(8, 8, 8, frame=1)
    calls = r.last_call()
    for e, var_ptr, what in ((make_ext(1, 8, 8), var.data_ptr(), "spp >= 2"),
                             (make_ext(8, 8, 8, flags=MM_EXT_ACCUMULATE), var.data_ptr(), "MM_EXT_ACCUMULATE"),
                             (good, var.data_ptr() + 2, "aligned"),
                             (good, out.data_ptr(), "overlaps"),
                             (good, out.data_ptr() + 8 * 16 - 4, "overlaps")):
        assert _raw(r, u, e, px.data_ptr(), offs, out.data_ptr(), var=var_ptr) == MM_ERR_INVALID, what
        msg = lib().mm_last_error(r._ctx).decode()
        assert "mm_trace_pixel_lists" in msg and what in msg, msg
    assert r.last_call() == calls
    assert _raw(r, u, good, px.data_ptr(), offs, out.data_ptr(), var=var.data_ptr()) == MM_OK
    r.sync()
    assert float(var[:8].max()) > 0 and r.last_call() == calls + 1
    r.close()


@pytest.mark.parametrize("case", ["form5", "form7", "no-lds", "reference"])
def test_query_methods_and_placements(maze, case):
    """MM_OPT_TRAVERSAL 5 and 7, MM_OPT_LDS_NODES 0 and MM_PIPE_REFERENCE (one reference list launch per
    non-empty list, under one call number), plain and with the variance."""
    from mirror_maze import MM_PIPE_REFERENCE, make_ext

    s, u, cams, ref = maze
    opts, pipe, form = {"form5": ({MM_OPT_TRAVERSAL: 5}, 0, 5), "form7": ({MM_OPT_TRAVERSAL: 7}, 0, 7),
                        "no-lds": ({MM_OPT_LDS_NODES: 0}, 0, None),
                        "reference": ({}, MM_PIPE_REFERENCE, None)}[case]
    px, offs, _ = _edge_lists()
    px2, offs2 = _lists(LENGTHS, VIEW, seed=41)
    r = _renderer(s, opts, pipe)
    for spp in (8, 3):
        e = make_ext(spp, 8, 8, frame=4)
        for p, o, n in ((px, offs, 4), (px2, offs2, 6)):
            want, want_v, rays, paths = _per_list(ref, u, cams[:n], e, KEYS[:n], p, o, var=True)
            calls = r.last_call()
            got, _, st = r.trace_pixel_lists(u, cams[:n], e, p, o, frame_keys=KEYS[:n], stats=True)
            assert _diff(_np(got), want) == 0 and (st.rays, st.paths) == (rays, paths)
            assert r.last_call() == calls + 1
            if pipe == MM_PIPE_REFERENCE:  # a launch per non-empty list and the resolve
                assert r.last_timing()[1] == int((np.diff(o.astype(np.int64)) > 0).sum()) + 1
            got, got_v, _ = r.trace_pixel_lists(u, cams[:n], e, p, o, frame_keys=KEYS[:n], var=True)
            assert _diff(_np(got), want) == 0 and np.array_equal(_bits(_np(got_v)), _bits(want_v))
    if form is not None:
        assert r.scene_info(MM_INFO_LAST_FORM) == form and r.scene_info(MM_INFO_LAST_LDS_MODE) == 3
    if case == "no-lds":
        assert r.scene_info(MM_INFO_LAST_LDS_MODE) in (0, 13)
    r.close()


def test_wavefront_is_unsupported(maze):
    from mirror_maze import MMError, make_ext
    from mirror_maze._lib import MM_ERR_UNSUPPORTED, MM_PIPE_WAVEFRONT

    s, u, cams, _ = maze
    r = _renderer(s, pipe=MM_PIPE_WAVEFRONT)
    px, offs = _lists([3, 4], VIEW, seed=50)
    calls = r.last_call()
    with pytest.raises(MMError) as ei:
        r.trace_pixel_lists(u, cams[:2], make_ext(8, 8, 8), px, offs)
    assert ei.value.code == MM_ERR_UNSUPPORTED and "MM_PIPE_WAVEFRONT" in str(ei.value)
    assert r.last_call() == calls
    r.close()


def test_back_to_back_calls_do_not_share_records(maze):
    """Twelve calls with two different list tables alternating, on one stream, read back after ONE sync: each
    result is its own table's (the tables take fresh records; the record ring grows once on the way)."""
    import torch

    from mirror_maze import make_ext

    s, u, cams, ref = maze
    e = make_ext(8, 8, 8, frame=60)
    pa, oa = _lists(LENGTHS, VIEW, seed=61)
    pb, ob = _lists([40, 0, 3, 64, 1], VIEW, seed=62)
    ca, cb = cams, cams[::-1][:5].copy()
    ka, kb = KEYS, [5, 4, 3, 2, 2**20]
    want_a, _, _, _ = _per_list(ref, u, ca, e, ka, pa, oa)
    want_b, _, _, _ = _per_list(ref, u, cb, e, kb, pb, ob)
    r = _renderer(s)
    ta, tb = (torch.from_numpy(p.view(np.int32)).cuda() for p in (pa, pb))
    outs = []
    r.sync()
    for k in range(12):
        if k % 2 == 0:
            outs.append(r.trace_pixel_lists(u, ca, e, ta, oa, frame_keys=ka)[0])
        else:
            outs.append(r.trace_pixel_lists(u, cb, e, tb, ob, frame_keys=kb)[0])
    r.sync()
    for k, o in enumerate(outs):
        assert _diff(_np(o), want_a if k % 2 == 0 else want_b) == 0, k
    r.close()


def test_arguments(maze):
    """Every refusal; a total of 0 entries is MM_OK and takes no call number; no scene; then a valid call."""
    import torch

    from mirror_maze import MM_EXT_ACCUMULATE, lib, make_ext
    from mirror_maze._lib import MM_ERR_INVALID, MM_ERR_NO_SCENE, MM_EXT_RGBA8, MM_OK, mm_uniform

    s, u, cams, ref = maze
    r = _renderer(s)
    pxh, offs = _lists([3, 0, 5], VIEW, seed=70)
    px = torch.from_numpy(pxh.view(np.int32)).cuda()
    out = torch.zeros((9, 4), dtype=torch.float32, device="cuda")
    e = make_ext(8, 8, 8, frame=2)
    U64 = lambda *v: np.array(v, dtype=np.uint64)  # noqa: E731
    raw = lambda **kw: _raw(r, kw.pop("u", u), kw.pop("e", e), kw.pop("px", px.data_ptr()),  # noqa: E731
                            kw.pop("offs", offs), kw.pop("out", out.data_ptr()), **kw)
    assert lib().mm_trace_pixel_lists(None, C.byref(u), None, C.byref(e), None, 3, px.data_ptr(), offs.ctypes.data,
                                      out.data_ptr(), None, None) == MM_ERR_INVALID
    calls = r.last_call()
    for kw in (dict(uni=False), dict(ext=False), dict(px=None), dict(out=None), dict(offs=None, n_lists=3)):
        assert raw(**kw) == MM_ERR_INVALID, kw
    for n in (0, 65536, 2**32 - 1):
        assert raw(n_lists=n) == MM_ERR_INVALID
    assert raw(offs=U64(1, 3, 8)) == MM_ERR_INVALID
    assert raw(offs=U64(0, 5, 3, 8)) == MM_ERR_INVALID
    assert raw(px=px.data_ptr() + 4) == MM_ERR_INVALID
    assert raw(out=out.data_ptr() + 4) == MM_ERR_INVALID
    assert raw(e=make_ext(8, 8, 8, flags=MM_EXT_RGBA8), out=out.data_ptr() + 2) == MM_ERR_INVALID
    for bad in (make_ext(0, 8, 8), make_ext(4097, 8, 8), make_ext(8, 32768, 8),
                make_ext(8, 8, 8, flags=MM_EXT_RGBA8 | MM_EXT_ACCUMULATE)):
        assert raw(e=bad) == MM_ERR_INVALID, bytes(bad)
    bad_view = mm_uniform.from_buffer_copy(u)
    bad_view.view_w = 0.0
    assert raw(u=bad_view) == MM_ERR_INVALID
    # the 32-bit queue over padded lists (nothing is read): 2^26 - 2^18 - 1 chunks fit
    most = 2**26 - 2**18 - 1
    assert raw(e=make_ext(64, 8, 8), offs=U64(0, 5, most + 1)) == MM_ERR_INVALID
    assert raw(e=make_ext(8, 8, 8), offs=U64(0, 1, 2, 8 * (most - 1) + 2)) == MM_ERR_INVALID
    assert raw(e=make_ext(1, 8, 8), offs=U64(0, 2**40)) == MM_ERR_INVALID
    # staged samples: 2^29 paths
    assert raw(e=make_ext(3, 8, 8), offs=U64(0, 100, 2**29 // 3 + 1)) == MM_ERR_INVALID
    r.set_option(MM_OPT_FUSE_RESOLVE, 0)
    assert raw(offs=U64(0, 2**25, 2**26 + 1)) == MM_ERR_INVALID
    r.set_option(MM_OPT_FUSE_RESOLVE, 1)
    assert r.last_call() == calls
    # a total of 0 entries: MM_OK whatever else is null, nothing enqueued, no call number
    assert raw(offs=U64(0, 0, 0)) == MM_OK
    assert raw(offs=U64(0, 0), px=None, out=None, uni=False, ext=False) == MM_OK
    empty, var, st = r.trace_pixel_lists(u, cams[:2], e, np.zeros((0, 2), np.uint32), [0, 0, 0], var=True, stats=True)
    assert tuple(empty.shape) == (0, 4) and tuple(var.shape) == (0,) and r.last_call() == calls
    bare = _renderer(None)
    assert _raw(bare, u, e, px.data_ptr(), offs, out.data_ptr()) == MM_ERR_NO_SCENE
    bare.close()
    with pytest.raises(ValueError):
        r.trace_pixel_lists(u, cams[:2], e, pxh, offs)  # three lists, two cameras
    with pytest.raises(ValueError):
        r.trace_pixel_lists(u, None, e, pxh, [0, 3, 7])  # offsets end before the array does
    assert raw(cams=cams[:3].copy()) == MM_OK
    r.sync()
    want, _, _, _ = _per_list(ref, u, cams[:3], e, None, pxh, offs)
    assert _diff(_np(out)[:8], want) == 0 and r.last_call() == calls + 1
    r.close()


def test_a_failed_call_is_reported_by_name(maze):
    """The call tracker names the call with its lists, entries and spp (MM_OPT_FAULT_INJECT 1 sets an error bit
    in the launch; the results are then not used)."""
    from mirror_maze import MMError, make_ext
    from mirror_maze._lib import MM_OPT_FAULT_INJECT

    s, u, cams, ref = maze
    r = _renderer(s)
    px, offs = _lists(LENGTHS, VIEW, seed=80)
    e = make_ext(8, 8, 8, frame=41)
    r.sync()
    r.set_option(MM_OPT_FAULT_INJECT, 1)
    r.trace_pixel_lists(u, cams, e, px, offs, frame_keys=KEYS)
    r.set_option(MM_OPT_FAULT_INJECT, 0)
    with pytest.raises(MMError) as ei:
        r.sync()
    assert f"call #{r.last_call()} (mm_trace_pixel_lists, 6 lists, 218 pixels, 8 spp)" in str(ei.value)
    assert "injected fault" in str(ei.value)
    r.sync()
    got, _, _ = r.trace_pixel_lists(u, cams, e, px, offs, frame_keys=KEYS)  # the context is clean again
    want, _, _, _ = _per_list(ref, u, cams, e, KEYS, px, offs)
    assert _diff(_np(got), want) == 0
    r.close()


def test_refine_frames_equals_refine_per_frame(maze):
    """Three frames of the walk traced with their variance in one launch, then two rounds: refine_frames on the
    batch against refine() frame by frame with the same keys, on all bits of colour, variance and count."""
    import torch

    from mirror_maze import make_ext
    from mirror_maze._lib import MM_OPT_DEFER_MIN

    s, u, _, _ = maze
    cams = TU.walk_cameras()[[0, 1, 3]]
    vw, vh = VIEW
    e = make_ext(8, 8, 8, frame=100)
    r = _renderer(s, {MM_OPT_DEFER_MIN: 0})  # (a multi-frame variance launch stages its samples through the rings)
    color, var, _ = r.trace_tile_var(u, e, 0, 0, vw, vh, cameras=cams)
    count = torch.full((3, vh, vw), 8.0, dtype=torch.float32, device="cuda")
    c1, v1, n1 = color.clone(), var.clone(), count.clone()
    rel_tol, extra = 0.26, 24
    for rnd in range(2):
        keys = [2**20 + 64 * f + rnd for f in range(3)]
        calls = r.last_call()
        got = r.refine_frames(u, cams, e, color, var, count, rel_tol, extra, keys)
        assert r.last_call() == calls + 1  # one trace call for the batch
        want = [r.refine(_with_cam(u, cams[f]), e, c1[f], v1[f], n1[f], rel_tol, extra, keys[f]) for f in range(3)]
        assert got == want and all(n > 0 for n in got), (got, want)
        assert np.array_equal(_bits(_np(color)), _bits(_np(c1)))
        assert np.array_equal(_bits(_np(var)), _bits(_np(v1)))
        assert np.array_equal(_bits(_np(count)), _bits(_np(n1)))
    assert set(np.unique(_np(count)).tolist()) == {8.0, 32.0, 56.0}
    calls = r.last_call()
    assert r.refine_frames(u, cams, e, color, var, count, float("inf"), extra, [1, 2, 3]) == [0, 0, 0]
    assert r.last_call() == calls
    r.close()


def test_list_ring_wraps_at_its_full_size(maze):
    """Eight calls with tables of 65535 lists (1114112 words each), nearly all of them empty: by the staging
    ring's policy (mm_stage_ring.h ring_place) the ring grows to 1, 2 and then 4 tables (calls 1, 2 and 4: past
    2^22 words, from where on it wraps), call 7 fills it exactly and call 8 waits for the device and takes the
    ring's first words again, without growing.  The last two calls' entries are mm_trace_pixels' per non-empty
    list; a table of empty lists alone takes no words and no call number."""
    import torch

    from mirror_maze import make_ext

    s, u, cams, ref = maze
    n_lists, words = 65535, (8 + 65535 + 1 + 15) // 16 * 16 + 16 * 65535
    assert 2 * words < 2**22 <= 4 * words
    e = make_ext(8, 8, 8, frame=90)
    r = _renderer(s)
    runs = []
    for k in range(8):
        lengths = np.zeros(n_lists, dtype=np.int64)
        where = [0, 1, 77 + k, 32768, 65000 - 9 * k, 65534]  # the first and the last list among them
        lengths[where] = [3, 1, 9, 8, 2 + k, 5]
        px, offs = _lists(lengths, VIEW, seed=900 + k)
        cams_k = np.ascontiguousarray(cams[(np.arange(n_lists) + k) % len(cams)])
        keys_k = (np.arange(n_lists, dtype=np.uint32) * 3 + 2**20 + k)
        calls = r.last_call()
        out = r.trace_pixel_lists(u, cams_k, e, torch.from_numpy(px.view(np.int32)).cuda(), offs, frame_keys=keys_k)[0]
        assert r.last_call() == calls + 1
        runs.append((where, px, offs, cams_k, keys_k, out))
    calls = r.last_call()
    none = r.trace_pixel_lists(u, cams_k, e, np.zeros((0, 2), np.uint32), np.zeros(n_lists + 1, np.uint64),
                               frame_keys=keys_k)[0]
    assert tuple(none.shape) == (0, 4) and r.last_call() == calls  # the empty-list path: no call number
    r.sync()
    for where, px, offs, cams_k, keys_k, out in runs[-2:]:
        where = sorted(where)
        sub = np.concatenate([[0], np.cumsum([int(offs[f + 1] - offs[f]) for f in where])]).astype(np.uint64)
        assert int(sub[-1]) == len(px)  # (the other lists are empty: the entries are these lists' back to back)
        want, _, _, _ = _per_list(ref, u, cams_k[where], e, keys_k[where].tolist(), px, sub)
        assert _diff(_np(out), want) == 0
    r.close()
