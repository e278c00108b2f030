"""Moving-camera sequences, host side (CPU only): the mm_trace_tile_cameras
symbol, scene.walk_cameras against a Player stepped by hand, and the camera
path scripts/flythrough.py prints.  The GPU side is
tests/test_gpu_camera_sequence.py."""
from __future__ import annotations

import ctypes as C
import importlib.util
import sys
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def scene():
    from mirror_maze import Scene

    return Scene.build(10, 0)


def _cam_row(u):
    return np.frombuffer(bytes(u.cam), dtype=np.float32)


def test_null_context_is_invalid_without_a_gpu():
    from mirror_maze import lib
    from mirror_maze._lib import MM_ERR_INVALID, mm_camera, mm_ext, mm_uniform

    u, e, cam = mm_uniform(), mm_ext(8, 8, 8, 0, 0, 0), mm_camera()
    rc = lib().mm_trace_tile_cameras(None, C.byref(u), C.addressof(cam), C.byref(e), 1, 0, 0, 1, 1, 1, None, None)
    assert rc == MM_ERR_INVALID


def _script():
    """30 frames from the spawn cell: sideways into the cell's wall (12 key
    events per frame = 1 unit; the wall stops the player from frame 4 on), a
    mouse turn, then forward with a second turn."""
    from mirror_maze import Player

    s = [([Player.KEY_A] * 12, []) for _ in range(7)]
    s += [([], [35.0, -4.0])]
    s += [([Player.KEY_W], []) for _ in range(10)]
    s += [([Player.KEY_W, Player.KEY_D], [-20.0])]
    s += [([Player.KEY_W] * 3, []) for _ in range(11)]
    assert len(s) == 30
    return s


def test_walk_cameras_equals_a_player_stepped_by_hand(scene):
    from mirror_maze import Player, walk_cameras
    from mirror_maze._lib import MM_PLAYER_COLLIDED, MM_PLAYER_ROTATED, mm_camera

    script = _script()
    cams = walk_cameras(Player(scene, 320, 180), script)
    assert cams.shape == (30, 10) and cams.dtype == np.float32
    assert cams.strides[0] == 40 == C.sizeof(mm_camera) and cams.flags.c_contiguous
    p = Player(scene, 320, 180)
    flags = 0
    for f, (keys, mouse) in enumerate(script):
        flags |= p.step(keys, mouse)
        want = _cam_row(p.uniform())   # the camera AFTER the step
        assert np.array_equal(cams[f].view(np.uint32), want.view(np.uint32)), f
    assert flags & MM_PLAYER_COLLIDED and flags & MM_PLAYER_ROTATED
    # the walk moved and turned the camera: no two consecutive frames of the forward leg are equal
    assert all(not np.array_equal(cams[f], cams[f + 1]) for f in range(8, 29))
    # focal and viewport are the view's (mm_uniform_default)
    assert np.array_equal(cams[:, 3], np.full(30, cams[0, 3])) and cams[0, 8] == np.float32(2.0 * 320 / 180)


def test_renderer_accepts_cameras_uniforms_and_arrays(scene):
    """The three forms of `cameras` give the same (n, 10) records."""
    from mirror_maze import Player, Renderer

    p = Player(scene, 64, 48)
    us = []
    for k in (Player.KEY_W, Player.KEY_D, Player.KEY_S):
        p.step([k], [5.0])
        us.append(p.uniform())
    rows = np.stack([_cam_row(u) for u in us])
    assert np.array_equal(Renderer._cameras(us), rows)
    assert np.array_equal(Renderer._cameras([u.cam for u in us]), rows)
    assert np.array_equal(Renderer._cameras(rows.astype(np.float64)), rows)
    with pytest.raises(ValueError):
        Renderer._cameras(np.zeros((3, 9), dtype=np.float32))


def test_flythrough_no_render_prints_the_walk(scene, capsys):
    """scripts/flythrough.py --no-render: the camera path of its key script,
    the one walk_cameras gives (floats printed as %.9g: exact for float32)."""
    from mirror_maze import Player, walk_cameras

    spec = importlib.util.spec_from_file_location("flythrough", REPO / "scripts" / "flythrough.py")
    fly = importlib.util.module_from_spec(spec)
    path0 = list(sys.path)
    try:
        spec.loader.exec_module(fly)
        rc = fly.main(["--maze", "10", "--frames", "30", "--turn-every", "4", "--turn-dx", "55", "--width", "320",
                       "--height", "180", "--no-render"])
    finally:
        sys.path[:] = path0
    assert rc == 0
    lines = [ln.split() for ln in capsys.readouterr().out.splitlines() if ln.startswith("frame ")]
    assert [int(ln[1]) for ln in lines] == list(range(30))
    got = np.array([[ln[3], ln[4], ln[5], ln[7], ln[8], ln[9], ln[10]] for ln in lines], dtype=np.float32)
    cams = walk_cameras(Player(scene, 320, 180), fly.key_script(30, 4, 55.0))
    assert np.array_equal(got.view(np.uint32), cams[:, [0, 1, 2, 4, 5, 6, 7]].view(np.uint32))
    assert not np.array_equal(cams[0, 4:8], cams[29, 4:8])  # it turned
