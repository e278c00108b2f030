"""The trimmed bounce block and chunk prologue of the wave-persistent trace
kernel (shade_step's shared tail, msign / rsq on the bits, the float start
cell, the division-free prologue) through the default pipeline against the CPU
oracle, bit for bit, on the smallest shapes that reach each path.  Tail
deferral is forced where stated (MM_OPT_DEFER 32 lanes, MM_OPT_DEFER_MIN 0):
that is the kernel bench.py times."""
from __future__ import annotations

import numpy as np
import pytest

from conftest import oracle_tile

pytestmark = pytest.mark.gpu

DEFER = {21: 32, 22: 0}
_CACHE: dict = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _maze():
    """(Scene, Oracle) of the N=10 maze; built once, read-only."""
    if "maze" not in _CACHE:
        from mirror_maze import Scene
        from oracle.oracle import Oracle

        s = Scene.build(10, 0)
        _CACHE["maze"] = (s, Oracle.from_scene(s))
    return _CACHE["maze"]


def _corridor():
    if "corridor" not in _CACHE:
        import aov_support as A
        from oracle.oracle import Oracle

        s, u = A.corridor()
        _CACHE["corridor"] = (s, Oracle.from_scene(s), u)
    return _CACHE["corridor"]


def _renderer(scene, opts):
    from mirror_maze import MM_PIPE_AUTO, Renderer

    r = Renderer(0)
    r.set_pipeline(MM_PIPE_AUTO)
    for k, v in opts.items():
        r.set_option(k, v)
    r.upload_scene(scene)
    return r


@pytest.mark.parametrize("frames", [1, 3])
def test_maze_tile_through_the_rings(gpu, frames):
    """N=10 maze, a 64x8 tile at 8 spp, 8/8 bounces, forced deferral: one frame,
    and three frames in one launch (the prologue's frame cursor crosses two
    frame boundaries; 64 chunks a frame)."""
    from mirror_maze import default_uniform, make_ext

    s, o = _maze()
    u = default_uniform(96, 54, 0)
    r = _renderer(s, DEFER)
    if frames == 1:
        got, st = r.trace_tile(u, make_ext(8, 8, 8, frame=2), 16, 23, 64, 8, stats=True)
        got = got.cpu().numpy()[None]
    else:
        got, st = r.trace_tile_frames(u, make_ext(8, 8, 8, frame=2), frames, 16, 23, 64, 8, stats=True)
        got = got.cpu().numpy()
    rays = 0
    for f in range(frames):
        ref, n = oracle_tile(o, u, make_ext(8, 8, 8, frame=2 + f), 16, 23, 64, 8)
        rays += n
        assert np.array_equal(_bits(got[f]), _bits(ref)), f"frame {f}"
    assert st.rays == rays
    r.close()


@pytest.mark.parametrize("opts", [DEFER, {}], ids=["rings", "default"])
def test_mirror_corridor(gpu, opts):
    """The AOV tests' corridor between two facing mirrors, a 64x8 tile of its
    67x48 view: waves that mix diffuse and mirror lanes, and mirror chains to
    the limit through the rings."""
    from mirror_maze import make_ext

    s, o, u = _corridor()
    e = make_ext(8, 8, 8, frame=1)
    ref, n = oracle_tile(o, u, e, 2, 20, 64, 8)
    r = _renderer(s, opts)
    got, st = r.trace_tile(u, e, 2, 20, 64, 8, stats=True)
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(ref))
    assert st.rays == n
    r.close()


@pytest.mark.parametrize("opts", [DEFER, {}], ids=["rings", "default"])
def test_spp_not_a_power_of_two(gpu, opts):
    """spp 6 at 40x5: the prologue's plain path / spp, and chunks that hold
    parts of pixels (64 % 6 != 0)."""
    from mirror_maze import default_uniform, make_ext

    s, o = _maze()
    u = default_uniform(96, 54, 0)
    e = make_ext(6, 8, 8, frame=4)
    ref, n = oracle_tile(o, u, e, 28, 25, 40, 5)
    r = _renderer(s, opts)
    got, st = r.trace_tile(u, e, 28, 25, 40, 5, stats=True)
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(ref))
    assert st.rays == n
    r.close()


@pytest.mark.parametrize("opts", [DEFER, {}], ids=["rings", "default"])
def test_strided_ragged_tile(gpu, opts):
    """x0 = 5, y0 = 3, every third row, 61 pixels wide, 7 rows: 8 spp chunks hold
    8 pixels, so most rows end inside a chunk (61 % 8 != 0)."""
    from mirror_maze import default_uniform, make_ext

    s, o = _maze()
    u = default_uniform(96, 54, 0)
    e = make_ext(8, 8, 8, frame=3)
    ref, n = oracle_tile(o, u, e, 5, 3, 61, 7, y_stride=3)
    r = _renderer(s, opts)
    got, st = r.trace_tile(u, e, 5, 3, 61, 7, y_stride=3, stats=True)
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(ref))
    assert st.rays == n
    r.close()
