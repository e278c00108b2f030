"""The rejection sampling's trial window on the GPU (mm_trace.h shade_step, predraw_trials;
tests/test_predraw_model.py is its CPU statement): windows of the N = 10 maze through the wave-persistent
kernel, two frames in one trace_tile_frames launch, 0 ulp against the oracle on the same tiles -- at every
pre-pass length K that takes another path (none, one trial, a few, the plan's default, the full window), with
the tail rings forced on (tail records carry the window) and off, with bounce limits at which the windows run
out on the device and are re-filled in the bounces, and through the staged resolve (64 % spp != 0).

128 x 64 x 8 spp is 1024 chunks: blocks with several waves parking, the smallest shape at which the rings, the
record format and the pre-pass can all go wrong."""
from __future__ import annotations

import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MM_OPT_DEFER, MM_OPT_DEFER_MIN, MM_OPT_PREDRAW = 21, 22, 27
VIEW = (640, 480)
ORIGIN = (288, 224)  # the horizon down the corridors
FRAMES = 2
RINGS = {"rings": {MM_OPT_DEFER: 32, MM_OPT_DEFER_MIN: 0}, "no-rings": {MM_OPT_DEFER: 0}}


def _bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _scene():
    from mirror_maze import Scene

    return Scene.build(10, 0)


@functools.lru_cache(maxsize=None)
def _reference(w, h, spp, bl, ml):
    """The oracle's frames 1 .. FRAMES of the window, computed once per shape and shared (read-only)."""
    from mirror_maze import default_uniform, make_ext
    from oracle.oracle import Oracle

    o = Oracle.from_scene(_scene())
    u = default_uniform(*VIEW, 0)
    frames = [o.trace_tile(u, make_ext(spp, bl, ml, frame=1 + f), *ORIGIN, w, h)[0] for f in range(FRAMES)]
    ref = np.stack(frames)
    ref.setflags(write=False)
    return ref


def _run(opts, w, h, spp, bl, ml):
    from mirror_maze import MM_INFO_LAST_DEFER, MM_INFO_LAST_FORM, Renderer, default_uniform, make_ext

    r = Renderer(0)
    for k, v in opts.items():
        r.set_option(k, v)
    r.upload_scene(_scene())
    got, _ = r.trace_tile_frames(default_uniform(*VIEW, 0), make_ext(spp, bl, ml, frame=1), FRAMES, *ORIGIN, w, h)
    r.sync()
    info = (r.scene_info(MM_INFO_LAST_FORM), r.scene_info(MM_INFO_LAST_DEFER))
    r.close()
    return got, info


@pytest.mark.parametrize("K", [0, 1, 5, None, 31], ids=["K0", "K1", "K5", "Kdefault", "K31"])
@pytest.mark.parametrize("rings", sorted(RINGS))
def test_window_bit_exact_at_every_prepass_length(gpu, rings, K):
    """(bounce_limit, mirror_limit) = (8, 8) at 128 x 64, 8 spp: the result never depends on K."""
    opts = dict(RINGS[rings])
    if K is not None:
        opts[MM_OPT_PREDRAW] = K
    got, (form, defer) = _run(opts, 128, 64, 8, 8, 8)
    bad = int((_bits(got) != _bits(_reference(128, 64, 8, 8, 8))).sum())
    assert bad == 0, (rings, K, bad)
    assert form == 11.0 and defer == (1.0 if rings == "rings" else 0.0)


@pytest.mark.parametrize("limits", [(40, 40), (8, 200)], ids=["b40m40", "b8m200"])
def test_windows_run_out_and_tails_carry_them(gpu, limits):
    """Long paths at 64 x 32, rings forced: 40 diffuse bounces need ~75 trials per path where a window holds
    31, and mirror chains of up to 200 bounces go through the tail records again and again."""
    bl, ml = limits
    got, (form, defer) = _run(RINGS["rings"], 64, 32, 8, bl, ml)
    bad = int((_bits(got) != _bits(_reference(64, 32, 8, bl, ml))).sum())
    assert bad == 0, (limits, bad)
    assert form == 11.0 and defer == 1.0


def test_staged_resolve_bit_exact(gpu):
    """24 spp (64 % spp != 0): a chunk's 64 paths are no whole pixels, samples are staged and k_resolve
    reduces them; 64 x 32, rings forced."""
    got, (form, defer) = _run(RINGS["rings"], 64, 32, 24, 8, 8)
    bad = int((_bits(got) != _bits(_reference(64, 32, 24, 8, 8))).sum())
    assert bad == 0, bad
    assert form == 11.0 and defer == 1.0
