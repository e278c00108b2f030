"""Moving-camera sequences in one launch (mm_trace_tile_cameras,
Renderer.trace_tile_cameras): frame f of a launch is traced with cameras[f] and
RNG frame ext.frame + f, and must equal, on float bits with zero differing
pixels, the single-frame trace with that camera -- the CPU oracle's
(oracle_tile with uniform.cam = cameras[f]) or, where no oracle is needed,
Renderer.trace_tile's.  Cameras: a seeded Player walk (scene.walk_cameras) plus
seeded cameras inside the maze as tests/test_gpu_frames.py::test_camera_sweep
draws them, with focal and viewport varied on some so that every field of the
device record is read.  Each oracle set is computed once per module and shared
by the kernel options that render it."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from conftest import oracle_tile

pytestmark = pytest.mark.gpu

FUSED, RINGS = {}, {21: 32, 22: 0}  # fused resolve; tail rings on launches of any size, samples staged
MM_INFO_LAST_LDS_MODE, MM_INFO_LAST_DEFER = 12, 14


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


def _renderer(scene, opts=FUSED):
    from mirror_maze import MM_PIPE_AUTO, Renderer

    r = Renderer(0)
    r.set_pipeline(MM_PIPE_AUTO)
    for k, v in opts.items():
        r.set_option(k, v)
    r.upload_scene(scene)
    return r


def _with_cam(u, row):
    """A copy of uniform `u` whose camera is the (10,) float32 record `row`."""
    from mirror_maze import mm_camera, mm_uniform

    v = mm_uniform.from_buffer_copy(u)
    v.cam = mm_camera.from_buffer_copy(np.ascontiguousarray(row, dtype=np.float32).tobytes())
    return v


def _cameras(maze_n, view_w, view_h, n_walk, n_maze, seed):
    """n_walk cameras of a seeded Player walk into the maze (several key events
    and a mouse move per frame, so consecutive cameras differ visibly), then
    n_maze seeded cameras inside it; the last of each kind with its own focal
    and viewport."""
    from mirror_maze import Player, calculate_quaternion, default_uniform, walk_cameras

    rng = np.random.default_rng(seed)
    script = [([Player.KEY_W] * int(rng.integers(6, 40)) + [Player.KEY_D] * int(rng.integers(0, 6)),
               [float(rng.normal(0, 60))]) for _ in range(n_walk)]
    walk = walk_cameras(Player(_scene(maze_n), view_w, view_h), script)
    base = -10.0 * (maze_n / 2)
    rows = []
    for _ in range(n_maze):
        u = default_uniform(view_w, view_h, 0)
        cx, cz = rng.integers(0, maze_n, size=2)
        u.cam.center[0] = base + 10.0 * cx + 5.0 + rng.uniform(-3, 3)
        u.cam.center[1] = rng.uniform(-6.0, 1.5)
        u.cam.center[2] = base + 10.0 * cz + 5.0 + rng.uniform(-3, 3)
        q = calculate_quaternion(rng.normal(size=3).astype(np.float32))
        for i in range(4):
            u.cam.quat[i] = float(q[i])
        rows.append(np.frombuffer(bytes(u.cam), dtype=np.float32))
    cams = np.concatenate([walk, np.stack(rows)]) if n_maze else walk.copy()
    for k in {n_walk - 1, len(cams) - 1}:
        cams[k, 3] = np.float32(rng.uniform(0.6, 1.7))                       # focal
        cams[k, 8:10] *= rng.uniform(0.5, 1.4, size=2).astype(np.float32)    # viewport
    assert len({c.tobytes() for c in cams}) == len(cams)
    return cams


class _Set:
    """A camera sequence and its oracle frames."""

    def __init__(self, maze_n, view, tile, spp, bl, ml, frame, cams):
        from mirror_maze import default_uniform, make_ext
        from oracle.oracle import Oracle

        self.scene = _scene(maze_n)
        self.u = default_uniform(view[0], view[1], 0)
        self.tile, self.cams, self.frame = tile, cams, frame
        self.ext = make_ext(spp, bl, ml, frame=frame)
        o = Oracle.from_scene(self.scene)
        x0, y0, w, h = tile
        self.refs, self.rays = [], 0
        for f, cam in enumerate(cams):
            ref, n = oracle_tile(o, _with_cam(self.u, cam), make_ext(spp, bl, ml, frame=frame + f), x0, y0, w, h)
            self.refs.append(ref)
            self.rays += n

    def check(self, opts, defer=None, lds_mode=None):
        r = _renderer(self.scene, opts)
        got, st = r.trace_tile_cameras(self.u, self.cams, self.ext, *self.tile, stats=True)
        got = got.cpu().numpy()
        assert got.shape == (len(self.cams), self.tile[3], self.tile[2], 4)
        for f, ref in enumerate(self.refs):
            assert _diff(got[f], ref) == 0, f"frame {f}: {_diff(got[f], ref)} pixels differ ({opts})"
        assert st.rays == self.rays and st.paths == len(self.cams) * self.tile[2] * self.tile[3] * self.ext.spp
        if defer is not None:
            assert bool(r.scene_info(MM_INFO_LAST_DEFER)) == defer
        if lds_mode is not None:
            assert int(r.scene_info(MM_INFO_LAST_LDS_MODE)) == lds_mode
        r.close()


@pytest.fixture(scope="module")
def ragged(gpu):
    """Case 1: 37 x 5 pixels x 8 spp = 1480 paths per frame -- not a multiple
    of 64: 24 chunks per frame, the last one padded."""
    return _Set(32, (320, 180), (11, 7, 37, 5), 8, 8, 8, 5, _cameras(32, 320, 180, 3, 3, seed=101))


@pytest.mark.parametrize("opts", [FUSED, RINGS], ids=["fused-resolve", "tail-rings"])
def test_ragged_frames_both_resolves(ragged, opts):
    assert (37 * 5 * 8) % 64 != 0 and -(-37 * 5 * 8 // 64) == 24
    ragged.check(opts, defer=bool(opts))


def test_staged_samples_when_spp_does_not_divide_64(gpu):
    """Case 2: 24 spp -- no fused resolve: the frames' samples are staged (the
    tail rings' path, by default on where 64 % spp != 0; MM_OPT_DEFER_MIN 0
    lets a launch this small take it) and resolved in one pass."""
    s = _Set(32, (320, 180), (100, 60, 40, 9), 24, 8, 8, 2, _cameras(32, 320, 180, 2, 1, seed=102))
    s.check({22: 0}, defer=True)


@pytest.fixture(scope="module")
def straddle(gpu):
    """Case 3: whole 240x135 frames at 8 spp: cpf = 4050 chunks per frame, 4050 %
    4 = 2, so 4-chunk claims cross frame boundaries.  Claims are 4 chunks while
    more than (resident waves x 256) paths remain (dequeue, MM_CLAIM_TAIL = 1):
    512 resident blocks on the MI355X (2 per CU x 256 CUs) = 8192 waves =
    2,097,152 paths, and 12 frames hold 3,110,400.  On a GPU with another CU
    count the resident grid differs: the frame count is then scaled so that the
    queue still exceeds that tail by more than three frames."""
    import torch

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    per_frame = 240 * 135 * 8
    assert per_frame // 64 == 4050 and 4050 % 4 == 2
    tail = 2 * cus * 16 * 256
    n = 12 if cus == 256 else -(-tail // per_frame) + 4
    assert n * per_frame > tail + 3 * per_frame
    return _Set(32, (240, 135), (0, 0, 240, 135), 8, 8, 8, 40, _cameras(32, 240, 135, n // 2, n - n // 2, seed=103))


@pytest.mark.parametrize("opts", [FUSED, RINGS], ids=["fused-resolve", "tail-rings"])
def test_claims_that_straddle_frames(straddle, opts):
    straddle.check(opts, defer=bool(opts))


def test_n64_scene_plain_cells_boxes_through_cache(gpu):
    """Case 4: the N=64 maze runs LDS mode 14 (plain cell words, leaf boxes read
    through L1/L2); 64 spp: one pixel per wave."""
    s = _Set(64, (3840, 2160), (700, 1500, 32, 16), 64, 16, 16, 7, _cameras(64, 3840, 2160, 2, 1, seed=104))
    s.check(FUSED, lds_mode=14)


def test_row_split_equals_one_tile(ragged):
    """Case 5: the rows of a 96x54 frame split two ways (row_shard, y_stride 2),
    interleaved, are the one-tile sequence."""
    from mirror_maze import default_uniform
    from mirror_maze.dist import row_shard

    u = default_uniform(96, 54, 0)
    r = _renderer(ragged.scene)
    whole, _ = r.trace_tile_cameras(u, ragged.cams, ragged.ext, 0, 0, 96, 54)
    whole = whole.cpu().numpy()
    woven = np.zeros_like(whole)
    for rank in range(2):
        y0, stride, rows = row_shard(54, 2, rank)
        part, _ = r.trace_tile_cameras(u, ragged.cams, ragged.ext, 0, y0, 96, rows, y_stride=stride)
        woven[:, y0::stride] = part.cpu().numpy()
    assert np.array_equal(_bits(woven), _bits(whole))
    assert len({whole[f].tobytes() for f in range(len(whole))}) == len(whole)  # the cameras differ: so do the frames
    r.close()


def test_rgba8_sequence_is_the_quantized_float_sequence(ragged):
    """Case 6."""
    import torch

    r = _renderer(ragged.scene)
    f32, _ = r.trace_tile_cameras(ragged.u, ragged.cams, ragged.ext, *ragged.tile)
    u8, _ = r.trace_tile_cameras(ragged.u, ragged.cams, ragged.ext, *ragged.tile, rgba8=True)
    assert u8.dtype == torch.uint8 and u8.shape == f32.shape
    assert torch.equal(u8, r.quantize(f32))
    assert int(u8[..., :3].max()) > 0
    r.close()


def test_back_to_back_calls_keep_their_own_cameras(ragged):
    """Case 7: call A (3 cameras) and call B (9 other cameras: more than the
    context's camera records held so far, so they are re-allocated) with no sync
    between them; every frame of both equals trace_tile with its camera."""
    r = _renderer(ragged.scene)
    cams_a = ragged.cams[:3]
    cams_b = _cameras(32, 320, 180, 5, 4, seed=107)
    assert not {c.tobytes() for c in cams_a} & {c.tobytes() for c in cams_b}
    tile, u = ragged.tile, ragged.u
    from mirror_maze import make_ext

    e_a, e_b = make_ext(8, 8, 8, frame=11), make_ext(8, 8, 8, frame=50)
    out_a, _ = r.trace_tile_cameras(u, cams_a, e_a, *tile)
    out_b, _ = r.trace_tile_cameras(u, cams_b, e_b, *tile)
    r.sync()
    for cams, e, out in ((cams_a, e_a, out_a), (cams_b, e_b, out_b)):
        out = out.cpu().numpy()
        for f, cam in enumerate(cams):
            one, _ = r.trace_tile(_with_cam(u, cam), make_ext(8, 8, 8, frame=e.frame + f), *tile)
            assert np.array_equal(_bits(out[f]), _bits(one.cpu().numpy())), (e.frame, f)
    r.close()


def test_degenerate_sequences(ragged):
    """Case 8: equal cameras give trace_tile_frames' frames; one camera gives
    trace_tile's."""
    r = _renderer(ragged.scene)
    u, tile = _with_cam(ragged.u, ragged.cams[1]), ragged.tile
    same, _ = r.trace_tile_cameras(ragged.u, [u] * 4, ragged.ext, *tile)
    frames, _ = r.trace_tile_frames(u, ragged.ext, 4, *tile)
    assert np.array_equal(_bits(same.cpu().numpy()), _bits(frames.cpu().numpy()))
    one, _ = r.trace_tile_cameras(ragged.u, [u.cam], ragged.ext, *tile)
    single, _ = r.trace_tile(u, ragged.ext, *tile)
    assert one.shape == (1, tile[3], tile[2], 4)
    assert np.array_equal(_bits(one.cpu().numpy()[0]), _bits(single.cpu().numpy()))
    r.close()


def test_errors(ragged):
    """Case 9."""
    import torch

    from mirror_maze import MM_PIPE_REFERENCE, MMError, lib, make_ext
    from mirror_maze._lib import MM_ERR_INVALID, MM_ERR_UNSUPPORTED, MM_EXT_ACCUMULATE, MM_OPT_FAULT_INJECT

    r = _renderer(ragged.scene)
    u, cams, e, tile = ragged.u, ragged.cams, ragged.ext, ragged.tile
    out = torch.zeros((2, tile[3], tile[2], 4), dtype=torch.float32, device="cuda")
    rows = np.ascontiguousarray(cams[:2])

    def raw(cams_ptr, n, ext):
        return lib().mm_trace_tile_cameras(r._ctx, C.byref(u), cams_ptr, C.byref(ext), n, *tile, 1, out.data_ptr(),
                                           None)

    assert raw(rows.ctypes.data, 0, e) == MM_ERR_INVALID
    assert raw(None, 2, e) == MM_ERR_INVALID
    assert raw(rows.ctypes.data, 2, make_ext(8, 8, 8, frame=5, flags=MM_EXT_ACCUMULATE)) == MM_ERR_INVALID
    with pytest.raises(MMError) as ei:
        r.trace_tile_cameras(u, rows[:0], e, *tile)
    assert ei.value.code == MM_ERR_INVALID
    r.set_pipeline(MM_PIPE_REFERENCE)
    with pytest.raises(MMError) as ei:
        r.trace_tile_cameras(u, rows, e, *tile)
    assert ei.value.code == MM_ERR_UNSUPPORTED
    r.set_pipeline(0)
    assert r.last_call() == 0  # none of the refused calls was enqueued
    # the error path's switch: the launch sets an error bit; the report names the call and its function
    r.set_option(MM_OPT_FAULT_INJECT, 1)
    r.trace_tile_cameras(u, rows, e, *tile)
    r.set_option(MM_OPT_FAULT_INJECT, 0)
    with pytest.raises(MMError) as ei:
        r.sync()
    assert f"call #{r.last_call()} (mm_trace_tile_cameras, frames 5..6" in str(ei.value)
    assert "injected fault" in str(ei.value)
    r.sync()
    got, _ = r.trace_tile_cameras(u, rows, e, *tile)  # the context is clean again
    assert _diff(got.cpu().numpy()[1], ragged.refs[1]) == 0
    r.close()


def test_camera_ring_wraps_at_its_full_size(gpu):
    """Four calls of 2048 cameras each on a 4x2 tile: by the staging ring's policy (mm_stage_ring.h ring_place;
    tests/trace_args pins this very sequence) the first call allocates 2048 records, the second grows the ring
    to its full 4096, the third takes the upper half and the fourth finds the ring full: it waits for the
    device and lands at record 0 again, without growing.  No sync between the last two calls; the first, a
    middle and the last frame of each equal trace_tile with that frame's camera."""
    from mirror_maze import default_uniform, make_ext

    n, tile = 2048, (158, 88, 4, 2)
    u = default_uniform(320, 180, 0)
    base = _cameras(10, 320, 180, 2, 6, seed=111)
    r = _renderer(_scene(10))
    calls = []
    for k in range(4):
        cams = np.ascontiguousarray(base[(np.arange(n) + k) % len(base)])
        cams[:, 0] += (np.arange(n) * 1e-3 + 0.37 * k).astype(np.float32)  # every record of every call its own
        e = make_ext(8, 8, 8, frame=1000 * k)
        calls.append((cams, e, r.trace_tile_cameras(u, cams, e, *tile)[0]))
    r.sync()
    assert len({c.tobytes() for cams, _, _ in calls for c in cams[[0, n // 2 - 1, n - 1]]}) == 12
    for cams, e, out in calls[2:]:
        out = out.cpu().numpy()
        assert out.shape == (n, 2, 4, 4)
        for f in (0, n // 2 - 1, n - 1):
            one, _ = r.trace_tile(_with_cam(u, cams[f]), make_ext(8, 8, 8, frame=e.frame + f), *tile)
            assert np.array_equal(_bits(out[f]), _bits(one.cpu().numpy())), (e.frame, f)
    r.close()
