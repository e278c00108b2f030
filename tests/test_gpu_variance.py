"""The per-pixel sample variance on the GPU: mm_trace_tile_var and
mm_trace_pixels_var bit for bit against tests/variance_ref.c (a C statement of
include/mm_api.h's definition over the oracle's samples) and against the plain
calls, through every route those have, and Renderer.refine end to end on the
frame whose tolerance tests/test_variance.py derives on the CPU.

The scene is Scene.build(4, 0), the view 64x48 from the walk's first camera
(variance_support.view_uniform), the limits 8/8 unless a test says otherwise."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import topup_support as TU
import variance_support as V

pytestmark = pytest.mark.gpu

SPPS = V.SPPS_LINEAR + V.SPPS_BLOCK
FRAME = 3


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _np(t):
    return t.cpu().numpy()


@pytest.fixture(scope="module")
def scene(gpu):
    from mirror_maze import Scene

    return Scene.build(4, 0)


def _renderer(scene, opts=None, pipe=0):
    from mirror_maze import Renderer

    r = Renderer(0)
    if pipe:
        r.set_pipeline(pipe)
    for k, v in (opts or {}).items():
        r.set_option(k, v)
    r.upload_scene(scene)
    return r


@pytest.fixture(scope="module")
def rdr(scene):
    r = _renderer(scene)
    yield r
    r.close()


@pytest.fixture(scope="module")
def refs(scene, tmp_path_factory):
    """variance_ref.c's (out, var) of TILE for every spp and y_stride 1 and 2; read-only."""
    from mirror_maze import make_ext

    ref = V.Ref(V.build_ref(tmp_path_factory.mktemp("variance_ref")), scene)
    u = V.view_uniform()
    d = {}
    for spp in SPPS:
        for ys in (1, 2):
            out, var = ref.tile(u, make_ext(spp, 8, 8, frame=FRAME), *V.TILE, ys)
            out.setflags(write=False)
            var.setflags(write=False)
            d[(spp, ys)] = (out, var)
    return d


@pytest.mark.parametrize("spp", SPPS)
def test_tile_is_the_reference(rdr, refs, spp):
    """1. Tile (5, 3, 23, 10): var equals variance_ref.c on all bits, out equals
    the plain trace_tile (and the reference) on all bits, with y_stride 1 and
    2.  spp 2, 3, 4, 12 take k_resolve_var, 8 (in registers), 16, 24, 64
    k_resolve8_var."""
    from mirror_maze import make_ext

    u, e = V.view_uniform(), make_ext(spp, 8, 8, frame=FRAME)
    x0, y0, w, h = V.TILE
    for ys in (1, 2):
        want_out, want_var = refs[(spp, ys)]
        out, var, st = rdr.trace_tile_var(u, e, x0, y0, w, h, y_stride=ys, stats=True)
        assert rdr.last_timing()[1] == 2  # the trace and the resolve
        plain, _ = rdr.trace_tile(u, e, x0, y0, w, h, y_stride=ys)
        assert tuple(out.shape) == (h, w, 4) and tuple(var.shape) == (h, w)
        assert np.array_equal(_bits(_np(out)), _bits(_np(plain)))
        assert np.array_equal(_bits(_np(out)), _bits(want_out))
        assert np.array_equal(_bits(_np(var)), _bits(want_var))
        assert st.paths == w * h * spp
    assert (want_var > 0).mean() > 0.1


@pytest.mark.parametrize("route", ["reference", "form5", "grid", "rgba8"])
@pytest.mark.parametrize("spp", [8, 12])
def test_every_route_of_the_plain_calls(scene, rdr, refs, route, spp):
    """2. MM_PIPE_REFERENCE, MM_OPT_TRAVERSAL 5 and 11, and MM_EXT_RGBA8 (out as
    the plain RGBA8 call, var unchanged)."""
    import torch

    from mirror_maze import MM_PIPE_REFERENCE, make_ext
    from mirror_maze._lib import MM_OPT_TRAVERSAL

    u, e = V.view_uniform(), make_ext(spp, 8, 8, frame=FRAME)
    want_out, want_var = refs[(spp, 1)]
    if route == "rgba8":
        out, var, _ = rdr.trace_tile_var(u, e, *V.TILE, rgba8=True)
        plain, _ = rdr.trace_tile(u, e, *V.TILE, rgba8=True)
        assert out.dtype == torch.uint8 and torch.equal(out, plain) and int(out[..., :3].max()) > 0
        assert np.array_equal(_bits(_np(var)), _bits(want_var))
        return
    opts, pipe = {"reference": ({}, MM_PIPE_REFERENCE), "form5": ({MM_OPT_TRAVERSAL: 5}, 0),
                  "grid": ({MM_OPT_TRAVERSAL: 11}, 0)}[route]
    r = _renderer(scene, opts, pipe)
    out, var, _ = r.trace_tile_var(u, e, *V.TILE)
    plain, _ = r.trace_tile(u, e, *V.TILE)
    assert np.array_equal(_bits(_np(out)), _bits(_np(plain))) and np.array_equal(_bits(_np(out)), _bits(want_out))
    assert np.array_equal(_bits(_np(var)), _bits(want_var))
    r.close()


@pytest.mark.parametrize("spp", [8, 12])
def test_three_cameras_in_one_launch(scene, rdr, spp):
    """3. Three cameras of the walk in one launch, with MM_OPT_DEFER_MIN 0 so
    the tail rings run: each frame's out and var equal the single-frame call
    (of a context with the default options) with that camera and frame number;
    the frame-sequence form (one camera) likewise."""
    from mirror_maze import MM_INFO_LAST_DEFER, make_ext
    from mirror_maze._lib import MM_OPT_DEFER_MIN

    u, e = V.view_uniform(), make_ext(spp, 8, 8, frame=FRAME)
    cams = TU.walk_cameras()[:3]
    x0, y0, w, h = V.TILE
    r = _renderer(scene, {MM_OPT_DEFER_MIN: 0})
    out, var, _ = r.trace_tile_var(u, e, x0, y0, w, h, cameras=cams)
    assert r.scene_info(MM_INFO_LAST_DEFER) == 1
    assert tuple(out.shape) == (3, h, w, 4) and tuple(var.shape) == (3, h, w)
    plain, _ = r.trace_tile_cameras(u, cams, e, x0, y0, w, h)
    assert np.array_equal(_bits(_np(out)), _bits(_np(plain)))
    seq_out, seq_var, _ = r.trace_tile_var(u, e, x0, y0, w, h, n_frames=3)
    assert r.scene_info(MM_INFO_LAST_DEFER) == 1 and tuple(seq_var.shape) == (3, h, w)
    for f in range(3):
        ef = make_ext(spp, 8, 8, frame=FRAME + f)
        one_out, one_var, _ = rdr.trace_tile_var(V.view_uniform(f), ef, x0, y0, w, h)
        assert np.array_equal(_bits(_np(out[f])), _bits(_np(one_out))), f
        assert np.array_equal(_bits(_np(var[f])), _bits(_np(one_var))), f
        one_out, one_var, _ = rdr.trace_tile_var(u, ef, x0, y0, w, h)
        assert np.array_equal(_bits(_np(seq_out[f])), _bits(_np(one_out))), f
        assert np.array_equal(_bits(_np(seq_var[f])), _bits(_np(one_var))), f
    assert not np.array_equal(_np(var[0]), _np(var[1]))
    r.close()


@pytest.mark.parametrize("spp", [8, 12])
def test_pixel_list(rdr, refs, spp):
    """4. 200 entries in random order with duplicates, four outside the view and
    (2^31, 2^31): each entry's (out, var) is that pixel of the tile call, out
    is mm_trace_pixels', and entries outside the view give zeros."""
    from mirror_maze import make_ext

    u, e = V.view_uniform(), make_ext(spp, 8, 8, frame=FRAME)
    x0, y0, w, h = V.TILE
    px, inside = V.list_pixels()
    assert len(px) == 200 and (~inside).sum() == 5
    tile_out, tile_var, _ = rdr.trace_tile_var(u, e, x0, y0, w, h)
    out, var, st = rdr.trace_pixels_var(u, e, px, stats=True)
    plain, _ = rdr.trace_pixels(u, e, px)
    assert tuple(out.shape) == (200, 4) and tuple(var.shape) == (200,) and st.paths == 195 * spp
    out, var = _np(out), _np(var)
    assert np.array_equal(_bits(out), _bits(_np(plain)))
    j, i = px[inside, 1].astype(np.int64) - y0, px[inside, 0].astype(np.int64) - x0
    assert np.array_equal(_bits(out[inside]), _bits(_np(tile_out)[j, i]))
    assert np.array_equal(_bits(var[inside]), _bits(_np(tile_var)[j, i]))
    assert np.array_equal(_bits(var[inside]), _bits(refs[(spp, 1)][1][j, i]))
    assert not _bits(out[~inside]).any() and not _bits(var[~inside]).any()
    # an empty list is no launch and no error
    calls = rdr.last_call()
    o0, v0, _ = rdr.trace_pixels_var(u, e, np.zeros((0, 2), np.uint32))
    assert tuple(o0.shape) == (0, 4) and tuple(v0.shape) == (0,) and rdr.last_call() == calls


def test_row_batches(scene, gpu):
    """5. GPU against GPU (the oracle cannot reach the size): view and tile
    4096x2100 at 8 spp, limits 2/2 -- 68.8 M paths, two row batches at 64 Mi
    (2048 rows, then 52), about 0.8 GB staged.  Rows 2040..2099 of out and var
    equal a 4096x60 call at y0 = 2040 on all bits (that call's routine is pinned
    by the tests above): the second batch's var slice starts at its own rows."""
    import torch

    from mirror_maze import default_uniform, make_ext, mm_camera

    W, H = 4096, 2100
    need = 12 * W * H * 8 + 20 * W * H + (256 << 20)  # the staged samples, out and var, and some room
    free = torch.cuda.mem_get_info(gpu)[0]
    if free < need:
        pytest.skip(f"the device has {free >> 20} MiB free, the case needs {need >> 20} MiB")
    u = default_uniform(W, H, 0)
    u.cam = mm_camera.from_buffer_copy(np.ascontiguousarray(TU.walk_cameras()[0], dtype=np.float32).tobytes())
    e = make_ext(8, 2, 2, frame=FRAME)
    assert W * 8 * 2048 == 64 << 20 and 2040 < 2048 < H
    r = _renderer(scene)
    out, var, _ = r.trace_tile_var(u, e, 0, 0, W, H)
    assert r.last_timing()[1] == 4  # two batches of two launches
    part_out, part_var, _ = r.trace_tile_var(u, e, 0, 2040, W, 60)
    assert r.last_timing()[1] == 2
    assert torch.equal(out[2040:].view(torch.int32), part_out.view(torch.int32))
    assert torch.equal(var[2040:].view(torch.int32), part_var.view(torch.int32))
    assert float((part_var > 0).float().mean()) > 0.1 and float((var[:2040] > 0).float().mean()) > 0.1
    r.close()


def test_errors(scene, rdr):
    """6. spp 1, MM_EXT_ACCUMULATE, a null, a misaligned and an overlapping
    var_dev are MM_ERR_INVALID for both calls; a multi-frame call whose plan has
    no deferral gives the plain call's own error with MM_OPT_FUSE_RESOLVE 0."""
    import torch

    from mirror_maze import MM_EXT_ACCUMULATE, MMError, make_ext
    from mirror_maze._lib import MM_ERR_INVALID, MM_OPT_FUSE_RESOLVE, lib

    L = lib()
    u = V.view_uniform()
    x0, y0, w, h = V.TILE
    out = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    var = torch.zeros((h * w + 4,), dtype=torch.float32, device="cuda")
    px = torch.tensor([[5, 3], [6, 4]], dtype=torch.int32, device="cuda")
    rdr.sync()
    calls = rdr.last_call()

    def tile(e, var_ptr, out_ptr=None):
        return L.mm_trace_tile_var(rdr._ctx, C.byref(u), None, C.byref(e), 1, x0, y0, w, h, 1,
                                   out_ptr or out.data_ptr(), var_ptr, None)

    def plist(e, var_ptr, out_ptr=None):
        return L.mm_trace_pixels_var(rdr._ctx, C.byref(u), C.byref(e), px.data_ptr(), 2, out_ptr or out.data_ptr(),
                                     var_ptr, None)

    good = make_ext(8, 8, 8, frame=FRAME)
    for call, name in ((tile, "mm_trace_tile_var"), (plist, "mm_trace_pixels_var")):
        for e, var_ptr, out_ptr, what in (
                (make_ext(1, 8, 8), var.data_ptr(), None, "spp >= 2"),
                (make_ext(8, 8, 8, flags=MM_EXT_ACCUMULATE), var.data_ptr(), None, "MM_EXT_ACCUMULATE"),
                (good, None, None, "null var_dev"),
                (good, var.data_ptr() + 2, None, "aligned"),
                (good, out.data_ptr(), None, "overlaps"),
                (good, out.data_ptr() + 16, None, "overlaps"),
                (good, var.data_ptr() + 16, var.data_ptr(), "overlaps")):
            assert call(e, var_ptr, out_ptr) == MM_ERR_INVALID, (name, what)
            msg = L.mm_last_error(rdr._ctx).decode()
            assert name in msg and what in msg, msg
    assert rdr.last_call() == calls  # nothing was enqueued
    # 3 frames of a small tile: below MM_OPT_DEFER_MIN there are no rings, and the samples must be staged
    with pytest.raises(MMError) as var_err:
        rdr.trace_tile_var(u, good, x0, y0, w, h, n_frames=3)
    r0 = _renderer(scene, {MM_OPT_FUSE_RESOLVE: 0})
    with pytest.raises(MMError) as plain_err:
        r0.trace_tile_frames(u, good, 3, x0, y0, w, h)
    r0.close()
    assert var_err.value.code == plain_err.value.code and str(var_err.value) == str(plain_err.value)
    assert "mm_trace_tile_frames" in str(var_err.value)
    # the context still works
    _, v, _ = rdr.trace_tile_var(u, good, x0, y0, w, h)
    assert float(v.max()) > 0


def test_failed_calls_are_reported_by_name(scene):
    """6. The call tracker names the two calls by their entry points (the error
    path's switch, MM_OPT_FAULT_INJECT 1, sets an error bit in the launch; the
    results are then not used)."""
    from mirror_maze import MMError, make_ext
    from mirror_maze._lib import MM_OPT_FAULT_INJECT

    u = V.view_uniform()
    x0, y0, w, h = V.TILE
    r = _renderer(scene)
    r.sync()
    r.set_option(MM_OPT_FAULT_INJECT, 1)
    r.trace_tile_var(u, make_ext(12, 8, 8, frame=41), x0, y0, w, h, y_stride=2)
    r.set_option(MM_OPT_FAULT_INJECT, 0)
    with pytest.raises(MMError) as ei:
        r.sync()
    assert f"call #{r.last_call()} (mm_trace_tile_var, frames 41..41, tile ({x0}, {y0}) {w}x{h} / 2, 12 spp)" in str(ei.value)
    assert "injected fault" in str(ei.value)
    r.sync()
    r.set_option(MM_OPT_FAULT_INJECT, 1)
    r.trace_pixels_var(u, make_ext(8, 8, 8, frame=42), np.array([[3, 4], [5, 6], [63, 47]], np.uint32))
    r.set_option(MM_OPT_FAULT_INJECT, 0)
    with pytest.raises(MMError) as ei:
        r.sync()
    assert f"call #{r.last_call()} (mm_trace_pixels_var, frame 42, 3 pixels, 8 spp)" in str(ei.value)
    assert "injected fault" in str(ei.value)
    r.sync()
    _, v, _ = r.trace_pixels_var(u, make_ext(8, 8, 8, frame=42), np.array([[3, 4]], np.uint32))  # clean again
    assert tuple(v.shape) == (1,)
    r.close()


def test_refine_end_to_end(rdr):
    """7. One 8-spp frame of the walk's turned camera at 160x120, then
    refine(rel_tol = REFINE_REL_TOL, extra_spp = 24).  (a) n_selected is
    variance_support.REFINE_SELECTED = 3882 of 19200 pixels, the count
    tests/test_variance.py derives from the reference alone.  (b) Every
    unselected pixel keeps its bits in color, var and count.  (c) Selected
    pixels end with count 32.  (d) Over the selected pixels the MSE against a
    512-spp frame falls to less than half: the expectation is 8 / 32 = 0.25, the
    variance of a mean of independent samples (the margin of
    test_gpu_topup.py::test_top_up_end_to_end).  A second refine with rel_tol =
    inf selects nothing and launches nothing."""
    import torch

    from mirror_maze import make_ext, select_noisy

    vw, vh = V.REFINE_VIEW
    u = V.refine_uniform()
    e = make_ext(V.REFINE_SPP, 8, 8, frame=V.REFINE_FRAME)
    color, var, _ = rdr.trace_tile_var(u, e, 0, 0, vw, vh)
    count = torch.full((vh, vw), float(V.REFINE_SPP), dtype=torch.float32, device="cuda")
    before = (_np(color).copy(), _np(var).copy(), _np(count).copy())
    px = _np(select_noisy(color, var, count, V.REFINE_REL_TOL)).astype(np.int64)
    sel = np.zeros((vh, vw), bool)
    sel[px[:, 1], px[:, 0]] = True
    calls = rdr.last_call()
    n = rdr.refine(u, e, color, var, count, V.REFINE_REL_TOL, V.REFINE_EXTRA, 2**20 + 3)
    assert rdr.last_call() == calls + 1  # one trace call
    after = (_np(color), _np(var), _np(count))
    # (a)
    assert n == int(sel.sum()) == V.REFINE_SELECTED
    # (b)
    for b, a in zip(before, after):
        assert np.array_equal(_bits(a[~sel]), _bits(b[~sel]))
    assert np.array_equal(_bits(after[0][..., 3]), _bits(before[0][..., 3]))
    # (c)
    assert (after[2][sel] == 32.0).all() and (after[2][~sel] == 8.0).all()
    assert np.isfinite(after[1]).all() and (after[1] >= 0).all()
    # (d)
    truth, _ = rdr.trace_tile(u, make_ext(512, 8, 8, frame=777), 0, 0, vw, vh)
    t = _np(truth).astype(np.float64)[sel][:, :3]
    mse_before = ((before[0].astype(np.float64)[sel][:, :3] - t) ** 2).mean()
    mse_after = ((after[0].astype(np.float64)[sel][:, :3] - t) ** 2).mean()
    print(f"selected {n}, MSE before {mse_before:.6g}, after {mse_after:.6g}, ratio {mse_after / mse_before:.4f}")
    assert mse_before > 0 and mse_after / mse_before < 0.5
    calls = rdr.last_call()
    assert rdr.refine(u, e, color, var, count, float("inf"), V.REFINE_EXTRA, 2**20 + 4) == 0
    assert rdr.last_call() == calls
    for a, c in zip(after, (color, var, count)):
        assert np.array_equal(_bits(_np(c)), _bits(a))
