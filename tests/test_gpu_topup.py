"""Topping up short histories on the GPU: mm_blend_pixels bit for bit against
tests/topup_ref.c, and Renderer.top_up end to end on a walk whose last step is
a turn (topup_support.walk_cameras; tests/test_topup.py derives the count of
short-history pixels on the CPU)."""
from __future__ import annotations

import numpy as np
import pytest

import topup_support as S

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def tu_lib(tmp_path_factory):
    return S.build_ref(tmp_path_factory.mktemp("topup_ref"))


@pytest.mark.parametrize("m", S.WEIGHTS)
def test_blend_pixels_is_the_reference(gpu, tu_lib, m):
    """8. A 37x5 window at (11, 7), alphas from {1, 2.5, 31}, 120 entries inside
    the window among 40 outside it: every bit is topup_ref.c's, and the pixels
    the list does not name keep theirs."""
    import torch

    from mirror_maze import Renderer

    image, px, extra = S.blend_inputs()
    x0, y0, w, h = S.WINDOW
    want, inside = S.blend_ref(tu_lib, image, x0, y0, px, extra, m)
    assert inside == 120
    with Renderer(0) as r:  # no scene needed
        img = torch.from_numpy(image).cuda()
        got = r.blend_pixels(img, px, torch.from_numpy(extra).cuda(), m, x0=x0, y0=y0)
        assert got is img
        got = got.cpu().numpy()
        assert np.array_equal(_bits(got), _bits(want))
        changed = (_bits(got) != _bits(image)).any(axis=-1)
        assert changed.sum() == 120
        # an empty list is no launch and no error
        assert r.blend_pixels(img, np.zeros((0, 2), np.uint32), torch.zeros((0, 4), device="cuda"), m) is img
        assert np.array_equal(_bits(img.cpu().numpy()), _bits(want))


@pytest.fixture(scope="module")
def walk(gpu):
    """The walk traced, its guides, and its accumulation; read-only."""
    from mirror_maze import Renderer, Scene, default_uniform, make_ext

    vw, vh = S.WALK_VIEW
    r = Renderer(0)
    r.upload_scene(Scene.build(4, 0))
    u = default_uniform(vw, vh, 0)
    cams = S.walk_cameras()
    ext = make_ext(8, 8, 8, frame=0)
    color, _ = r.trace_tile_cameras(u, cams, ext, 0, 0, vw, vh)
    aov = r.trace_aov(u, cams, 8, x0=0, y0=0, w=vw, h=vh)
    acc = r.accumulate(u, cams, color, aov)
    yield r, u, cams, ext, aov, acc
    r.close()


def _with_cam(u, row):
    from mirror_maze import mm_camera, mm_uniform

    v = mm_uniform.from_buffer_copy(u)
    v.cam = mm_camera.from_buffer_copy(np.ascontiguousarray(row, dtype=np.float32).tobytes())
    return v


def test_top_up_end_to_end(walk):
    """9. accumulate, then top_up(n_min=2, extra_spp=24) on the walk's last
    frame, whose turn leaves 3569 of its 19200 pixels at N < 2 (the count
    tests/test_topup.py::test_walk_selects_enough_pixels derives on the CPU
    from temporal_ref.c over aov_ref.c's guides).  (a) Every selected pixel
    ends with alpha N + 3, every other pixel keeps its bits, n_selected is the
    count the host takes from the accumulated alpha and id.  (b) Over the
    selected pixels the MSE against a 512-spp frame of that camera falls to
    less than half: the expectation is 8 / (8 + 24) = 0.25, the variance of a
    mean of independent samples."""
    from mirror_maze import MM_AOV_ID_FAILED, MM_AOV_ID_MISS, make_ext

    r, u, cams, ext, aov, acc = walk
    vw, vh = S.WALK_VIEW
    before = acc[3].cpu().numpy()
    ids = aov["id"][3].cpu().numpy().view(np.uint32)
    sel = (before[..., 3] < 2) & (ids != MM_AOV_ID_MISS) & (ids != MM_AOV_ID_FAILED)
    assert int(sel.sum()) == S.WALK_SELECTED >= 300
    calls = r.last_call()
    last = acc[3].clone()
    out, n = r.top_up(u, cams[3], ext, last, {"id": aov["id"][3]}, n_min=2, extra_spp=24, frame_key=2**20 + 3)
    assert out is last and n == int(sel.sum())
    assert r.last_call() == calls + 1  # one trace call (the blend takes no call number)
    after = out.cpu().numpy()
    # (a)
    assert np.array_equal(after[sel][:, 3], before[sel][:, 3] + np.float32(3.0))
    assert np.array_equal(_bits(after[~sel]), _bits(before[~sel]))
    # (b)
    truth, _ = r.trace_tile(_with_cam(u, cams[3]), make_ext(512, 8, 8, frame=777), 0, 0, vw, vh)
    t = truth.cpu().numpy().astype(np.float64)[sel][:, :3]
    mse_before = ((before.astype(np.float64)[sel][:, :3] - t) ** 2).mean()
    mse_after = ((after.astype(np.float64)[sel][:, :3] - t) ** 2).mean()
    print(f"selected {n}, MSE before {mse_before:.6g}, after {mse_after:.6g}, ratio {mse_after / mse_before:.4f}")
    assert mse_before > 0 and mse_after / mse_before < 0.5


def test_top_up_of_a_window_and_of_nothing(walk):
    """A window of the accumulated frame topped up on its own ends with the
    bits the whole frame's top-up gives those pixels (the trace is keyed on the
    pixel, the blend is per pixel); with no pixel short nothing is launched."""
    r, u, cams, ext, aov, acc = walk
    whole = acc[3].clone()
    r.top_up(u, cams[3], ext, whole, aov["id"][3], 2, 24, 2**20 + 3)
    x0, y0, w, h = 93, 30, 64, 48  # the turn's new columns are on the right
    part = acc[3][y0:y0 + h, x0:x0 + w].contiguous()
    ids = aov["id"][3][y0:y0 + h, x0:x0 + w].contiguous()
    part, n = r.top_up(u, cams[3], ext, part, ids, 2, 24, 2**20 + 3, x0=x0, y0=y0)
    assert 0 < n < w * h
    assert np.array_equal(_bits(part.cpu().numpy()), _bits(whole[y0:y0 + h, x0:x0 + w].cpu().numpy()))
    calls = r.last_call()
    same, n = r.top_up(u, cams[3], ext, whole, aov["id"][3], 1.0, 24, 2**20 + 4)  # N >= 1 everywhere
    assert n == 0 and same is whole and r.last_call() == calls


def test_a_failed_list_call_is_reported_by_name(walk):
    """The call tracker numbers a list call and names it: the function, the
    frame, the entries and the spp (the error path's switch, MM_OPT_FAULT_INJECT
    1, sets an error bit in the launch; the results are then not used)."""
    from mirror_maze import MMError, make_ext
    from mirror_maze._lib import MM_OPT_FAULT_INJECT

    r, u, cams, ext, aov, acc = walk
    px = np.array([[3, 4], [5, 6], [159, 119]], np.uint32)
    r.sync()
    r.set_option(MM_OPT_FAULT_INJECT, 1)
    r.trace_pixels(u, make_ext(8, 8, 8, frame=41), px)
    r.set_option(MM_OPT_FAULT_INJECT, 0)
    with pytest.raises(MMError) as ei:
        r.sync()
    assert f"call #{r.last_call()} (mm_trace_pixels, frame 41, 3 pixels, 8 spp)" in str(ei.value)
    assert "injected fault" in str(ei.value)
    r.sync()
    again, _ = r.trace_pixels(u, make_ext(8, 8, 8, frame=41), px)  # the context is clean again
    tile, _ = r.trace_tile(u, make_ext(8, 8, 8, frame=41), 159, 119, 1, 1)
    assert np.array_equal(_bits(again.cpu().numpy()[2]), _bits(tile.cpu().numpy()[0, 0]))
