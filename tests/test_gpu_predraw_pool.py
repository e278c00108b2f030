"""The pre-pass's pooled top-up rounds on the GPU (mm_trace.h pool_trials, MM_OPT_PREDRAW_POOL;
tests/test_predraw_pool_model.py is the CPU statement): windows of the N = 10 maze through the wave-persistent
kernel, 0 ulp against the oracle and equal to the launch without pooling -- at 64 x 16 (whole waves) and 37 x 5
(a last chunk with inactive lanes: 8 of 64 at 8 spp, 43 at 3 spp), at 8 spp (fused resolve) and 3 spp (staged
samples), at every number of own rounds K1 that takes another path (none: everything pooled; one; a few; the
plan's 12; the full window: no lane needy), at bounce limits whose need is 0, 1, 7, 15 and beyond the window,
with the tail rings on (tail chunks run no pre-pass, their records carry the window) and off, two frames per
launch.  Shapes are the smallest with more than one block's worth of chunks in flight and a partial chunk."""
from __future__ import annotations

import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MM_OPT_DEFER, MM_OPT_DEFER_MIN, MM_OPT_PREDRAW, MM_OPT_PREDRAW_POOL = 21, 22, 27, 28
VIEW = (640, 480)
ORIGIN = (288, 224)  # the horizon down the corridors
FRAMES = 2
ML = 8
RINGS = {"rings": {MM_OPT_DEFER: 32, MM_OPT_DEFER_MIN: 0}, "no-rings": {MM_OPT_DEFER: 0}}
SHAPES = {"64x16": (64, 16), "37x5": (37, 5)}


def _bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _scene():
    from mirror_maze import Scene

    return Scene.build(10, 0)


@functools.lru_cache(maxsize=None)
def _reference(w, h, spp, bl):
    """The oracle's frames 1 .. FRAMES of the window, computed once per shape and shared (read-only)."""
    from mirror_maze import default_uniform, make_ext
    from oracle.oracle import Oracle

    o = Oracle.from_scene(_scene())
    u = default_uniform(*VIEW, 0)
    ref = np.stack([o.trace_tile(u, make_ext(spp, bl, ML, frame=1 + f), *ORIGIN, w, h)[0] for f in range(FRAMES)])
    ref.setflags(write=False)
    return ref


def _run(rings, K1, pool, w, h, spp, bl):
    """Frames 1 .. FRAMES: one trace_tile_frames launch, or (no rings and no fused resolve: a multi-frame
    launch needs one of them) one trace_tile launch per frame."""
    from mirror_maze import MM_INFO_LAST_FORM, Renderer, default_uniform, make_ext

    r = Renderer(0)
    for k, v in RINGS[rings].items():
        r.set_option(k, v)
    if K1 is not None:
        r.set_option(MM_OPT_PREDRAW, K1)
    r.set_option(MM_OPT_PREDRAW_POOL, pool)
    r.upload_scene(_scene())
    u = default_uniform(*VIEW, 0)
    if rings == "rings" or 64 % spp == 0:
        got, _ = r.trace_tile_frames(u, make_ext(spp, bl, ML, frame=1), FRAMES, *ORIGIN, w, h)
        r.sync()
        got = _bits(got)
    else:
        frames = []
        for f in range(FRAMES):
            g, _ = r.trace_tile(u, make_ext(spp, bl, ML, frame=1 + f), *ORIGIN, w, h)
            r.sync()
            frames.append(_bits(g))
        got = np.stack(frames)
    form = r.scene_info(MM_INFO_LAST_FORM)
    r.close()
    assert form == 11.0
    return got


@functools.lru_cache(maxsize=None)
def _unpooled(rings, w, h, spp, bl):
    """MM_OPT_PREDRAW_POOL 0 at the plan's own rounds: the pre-pass before the pooled rounds existed."""
    got = _run(rings, None, 0, w, h, spp, bl)
    got.setflags(write=False)
    return got


def _check(rings, K1, w, h, spp, bl):
    got = _run(rings, K1, 1, w, h, spp, bl)
    ref = _bits(_reference(w, h, spp, bl)).reshape(got.shape)
    bad_ref = int((got != ref).sum())
    bad_ab = int((got != _unpooled(rings, w, h, spp, bl)).sum())
    print(f"rings={rings} K1={K1} {w}x{h} spp={spp} bl={bl}: words off the oracle {bad_ref}, off pool=0 {bad_ab}")
    assert bad_ref == 0 and bad_ab == 0, (rings, K1, w, h, spp, bl, bad_ref, bad_ab)


@pytest.mark.parametrize("K1", [0, 1, 5, 12, 31], ids=lambda k: f"K{k}")
@pytest.mark.parametrize("spp", [8, 3], ids=lambda s: f"spp{s}")
@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("rings", sorted(RINGS))
def test_pooled_rounds_bit_exact_at_every_own_round_count(gpu, rings, shape, spp, K1):
    """bounce_limit 8 (need 7): the result depends on neither K1 nor the pooling."""
    _check(rings, K1, *SHAPES[shape], spp, 8)


@pytest.mark.parametrize("bl", [1, 2, 16, 40], ids=lambda b: f"b{b}")
@pytest.mark.parametrize("K1", [1, None], ids=["K1", "Kdefault"])
@pytest.mark.parametrize("spp", [8, 3], ids=lambda s: f"spp{s}")
@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("rings", sorted(RINGS))
def test_pooled_rounds_bit_exact_at_every_need(gpu, rings, shape, spp, K1, bl):
    """need = min(bounce_limit - 1, 31): 0 (no pooled round), 1, 15, and 39 -> 31, beyond what a window of
    31 trials can hold (the pooled rounds fill the windows, the in-bounce rounds refill them); with one own
    round (nearly everything pooled) and the plan's own rounds."""
    _check(rings, K1, *SHAPES[shape], spp, bl)
