"""mm_query_rays and mm_trace_aov on the GPU against tests/aov_ref.c (the same
definitions over the oracle's reference walk): every comparison is on bits,
with zero differing elements and no case excluded -- the certified grid search
hands ties and uncertified answers to the walk, so there is nothing to excuse.
The input conditions (what the corridor scene covers) are tests/test_aov.py's."""
from __future__ import annotations

import ctypes as C
import itertools

import numpy as np
import pytest

import aov_support as A

pytestmark = pytest.mark.gpu

MM_OPT_LDS_NODES, MM_OPT_TRAVERSAL = 1, 7
MM_INFO_GRID_OK, MM_INFO_LEAN = 1, 8
NAMES = ("normal_depth", "albedo", "id")
VIEW = (80, 60)           # the mazes' frame
VIEW_CORRIDOR = (70, 16)  # the corridor's: the tiles' rows span its camera's whole field of view
VIEW_WIDE = (192, 108)    # the soup's and the N=64 maze's: a 67-pixel row spans a third of the view
# x0, y0, w, h, y_stride: a ragged last wave; one whole wave; one lane
TILES = [(3, 2, 67, 5, 3), (5, 11, 64, 1, 1), (41, 9, 1, 1, 1)]
WIDE_TILES = [(0, 0, 67, 3, 1), (94, 53, 67, 3, 5), (125, 98, 67, 3, 3)]
LIMITS = [0, 1, 2, 15, 200]
# query policies: MM_OPT_TRAVERSAL 11 / 7 / 5 with MM_OPT_LDS_NODES 1 / 0, and MM_PIPE_REFERENCE
POLICIES = {f"trav{t}-lds{l}": {MM_OPT_TRAVERSAL: t, MM_OPT_LDS_NODES: l} for t in (11, 7, 5) for l in (1, 0)}
POLICIES["auto"] = {}
POLICIES["reference"] = "reference"


@pytest.fixture(scope="module")
def ref_lib(tmp_path_factory):
    return A.build_ref(tmp_path_factory.mktemp("aov_ref"))


_CACHE = {}


def _scene(name):
    """(Scene, uniform at VIEW) by name, built once."""
    from mirror_maze import Scene, default_uniform

    if name not in _CACHE:
        if name == "corridor":
            s, u = A.corridor()
            u.view_w, u.view_h = VIEW_CORRIDOR
        elif name in ("soup", "lattice"):
            from test_gpu_random_scene import random_scene

            s = random_scene(3000, 11, True) if name == "lattice" else random_scene(3000, 7, False)
            u = default_uniform(*VIEW_WIDE, 0)
        elif name == "maze64":
            s, u = Scene.build(64, 0), default_uniform(*VIEW_WIDE, 0)
        elif name == "wide-slow-soup":
            import variant_census_support as vc

            s, u = vc.scene(vc.WIDE_SLOW_SOUP[0]), vc.uniform(vc.WIDE_SLOW_SOUP[0], 0)
            u.view_w, u.view_h = VIEW_WIDE
        else:
            s, u = Scene.build(int(name[4:]), 0), default_uniform(*VIEW, 0)
        _CACHE[name] = (s, u)
    return _CACHE[name]


def _ref(ref_lib, name):
    if ("ref", name) not in _CACHE:
        _CACHE[("ref", name)] = A.Ref(ref_lib, _scene(name)[0])
    return _CACHE[("ref", name)]


def _ref_tile(ref_lib, name, u, limit, tile):
    """The reference buffers of a tile, computed once and shared (read-only)."""
    key = ("tile", name, bytes(u), limit, tile)
    if key not in _CACHE:
        x0, y0, w, h, ys = tile
        t = _ref(ref_lib, name).tile(u, limit, x0, y0, w, h, ys)
        for v in t.values():
            v.setflags(write=False)
        _CACHE[key] = t
    return _CACHE[key]


def _renderer(scene, policy):
    from mirror_maze import MM_PIPE_REFERENCE, Renderer

    r = Renderer(0)
    if policy == "reference":
        r.set_pipeline(MM_PIPE_REFERENCE)
    else:
        for k, v in policy.items():
            r.set_option(k, v)
    r.upload_scene(scene)
    return r


def _unsupported(r, policy):
    """Whether the scene lacks what the policy's query method needs."""
    if policy == "reference":
        return False
    t = policy.get(MM_OPT_TRAVERSAL)
    return (t == 11 and r.scene_info(MM_INFO_GRID_OK) == 0.0) or (t == 7 and r.scene_info(MM_INFO_LEAN) == 0.0)


def _bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint32)


def _diffs(got, ref, frame=0):
    """Differing elements per buffer between a trace_aov result and a reference tile."""
    return {k: int((_bits(got[k])[frame] != _bits(ref[k])).sum()) for k in got}


def _trace(r, u, limit, tile, cameras=None, **kw):
    x0, y0, w, h, ys = tile
    return r.trace_aov(u, cameras, limit, x0=x0, y0=y0, w=w, h=h, y_stride=ys, **kw)


# ---- AOV ---------------------------------------------------------------------
@pytest.mark.parametrize("policy", sorted(POLICIES))
@pytest.mark.parametrize("name", ["maze4", "corridor"])
def test_aov_tiles_limits_policies_bit_exact(gpu, ref_lib, name, policy):
    from mirror_maze import MMError, _lib

    s, u = _scene(name)
    r = _renderer(s, POLICIES[policy])
    if _unsupported(r, POLICIES[policy]):
        with pytest.raises(MMError) as e:
            _trace(r, u, 15, TILES[0])
        assert e.value.code == _lib.MM_ERR_UNSUPPORTED
        r.close()
        return
    seen = set()
    for tile in TILES:
        for limit in LIMITS:
            got = _trace(r, u, limit, tile)
            ref = _ref_tile(ref_lib, name, u, limit, tile)
            d = _diffs(got, ref)
            assert not any(d.values()), (name, policy, tile, limit, d)
            seen |= {int(x) for x in np.unique(np.minimum(ref["id"] >> 30, 3))}
    r.sync()
    assert 1 in seen and 3 in seen, seen  # surfaces and misses were compared
    r.close()


@pytest.mark.parametrize("limit", [15, 200])
def test_aov_corridor_whole_view_bit_exact(gpu, ref_lib, limit):
    """The 67x48 view test_aov.py's input conditions are stated on: MISS,
    SURFACE and MIRROR_END pixels, and chains of up to 199 mirror hits."""
    s, u = A.corridor()
    tile = (0, 0, 67, 48, 1)
    ref = _ref_tile(ref_lib, "corridor", u, limit, tile)
    assert all(m.any() for m in A.kinds(ref["id"])) and ref["albedo"][..., 3].max() >= min(limit - 1, 50)
    r = _renderer(s, {})
    d = _diffs(_trace(r, u, limit, tile), ref)
    assert not any(d.values()), d
    r.close()


def test_aov_maze64_default_mode_bit_exact(gpu, ref_lib):
    s, u = _scene("maze64")
    r = _renderer(s, {})
    assert r.scene_info(MM_INFO_GRID_OK) == 1.0
    for tile in WIDE_TILES:
        d = _diffs(_trace(r, u, 15, tile), _ref_tile(ref_lib, "maze64", u, 15, tile))
        assert not any(d.values()), (tile, d)
    r.close()


@pytest.mark.parametrize("policy", ["auto", "trav5-lds1", "trav11-lds0", "trav7-lds1", "reference"])
def test_aov_random_scene_with_slow_records_bit_exact(gpu, ref_lib, policy):
    """A seeded soup of 3000 rects whose normals are not exactly +-1 (SLOW
    records: general rect tests in the grid search, no loop form 7)."""
    from mirror_maze import MMError, _lib

    s, u = _scene("soup")
    r = _renderer(s, POLICIES[policy])
    assert r.scene_info(MM_INFO_GRID_OK) == 1.0 and r.scene_info(MM_INFO_LEAN) == 0.0
    if policy == "trav7-lds1":
        with pytest.raises(MMError) as e:
            _trace(r, u, 15, WIDE_TILES[0])
        assert e.value.code == _lib.MM_ERR_UNSUPPORTED
        r.close()
        return
    for tile in WIDE_TILES:
        for limit in (1, 15):
            d = _diffs(_trace(r, u, limit, tile), _ref_tile(ref_lib, "soup", u, limit, tile))
            assert not any(d.values()), (policy, tile, limit, d)
    r.close()


# ---- sequence ----------------------------------------------------------------
def test_aov_camera_sequence_equals_single_calls_and_the_reference(gpu, ref_lib):
    """3 cameras of a Player walk and 2 inside the maze (two with their own
    focal and viewport) in one call = five single-camera calls = the helper."""
    from test_gpu_camera_sequence import _cameras, _with_cam

    s, u = _scene("maze10")
    cams = _cameras(10, VIEW[0], VIEW[1], 3, 2, seed=5)
    tile = TILES[0]
    r = _renderer(s, {})
    got = _trace(r, u, 15, tile, cameras=cams)
    assert got["normal_depth"].shape == (5, 5, 67, 4) and got["id"].shape == (5, 5, 67)
    for f, cam in enumerate(cams):
        uf = _with_cam(u, cam)
        ref = _ref_tile(ref_lib, "maze10", uf, 15, tile)
        d = _diffs(got, ref, f)
        assert not any(d.values()), (f, d)
        one = _trace(r, uf, 15, tile)
        assert all(np.array_equal(_bits(one[k])[0], _bits(got[k])[f]) for k in NAMES), f
        one = _trace(r, u, 15, tile, cameras=cams[f:f + 1])
        assert all(np.array_equal(_bits(one[k])[0], _bits(got[k])[f]) for k in NAMES), f
    r.close()


def test_aov_output_subsets_leave_the_other_buffers_untouched(gpu, ref_lib):
    import torch

    s, u = _scene("corridor")
    tile = TILES[0]
    ref = _ref_tile(ref_lib, "corridor", u, 15, tile)
    r = _renderer(s, {})
    for n in (1, 2, 3):
        for want in itertools.combinations(NAMES, n):
            # one allocation, the three buffers back to back: a store past a wanted buffer lands in a sentinel
            raw = torch.full((5 * 67 * 9 + 8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
            px = 5 * 67
            out = {"normal_depth": raw[:4 * px].view(torch.float32).view(1, 5, 67, 4),
                   "albedo": raw[4 * px:8 * px].view(torch.float32).view(1, 5, 67, 4),
                   "id": raw[8 * px:9 * px].view(1, 5, 67)}
            got = _trace(r, u, 15, tile, want=want, out=out)
            assert sorted(got) == sorted(want)
            d = _diffs(got, {k: ref[k] for k in want})
            assert not any(d.values()), (want, d)
            for k in NAMES:
                if k not in want:
                    assert (_bits(out[k]) == 0x5A5A5A5A).all(), (want, k)
            assert (_bits(raw[9 * px:]) == 0x5A5A5A5A).all()
    r.close()


# ---- query --------------------------------------------------------------------
def _rays(scene, n, seed):
    """n seeded rays, eight kinds in turn: origins inside the scene; outside its
    box aimed in, and aimed away; on a wall's plane; one and two zero direction
    components; unnormalised directions; rays along the scene box's faces."""
    rng = np.random.default_rng(seed)
    r = scene.rects.astype(np.float64)
    corners = np.concatenate([r[:, 0:3], r[:, 0:3] + r[:, 3:6], r[:, 0:3] + r[:, 6:9], r[:, 0:3] + r[:, 3:6] + r[:, 6:9]])
    lo, hi = corners.min(axis=0), corners.max(axis=0)
    rays = np.zeros((n, 2, 4), np.float32)
    rays[:, :, 3] = rng.normal(size=(n, 2))  # the w components are ignored
    for i in range(n):
        kind = i % 8
        o = rng.uniform(lo, hi)
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        if kind in (1, 2):
            a = int(rng.integers(3))
            o[a] = hi[a] + rng.uniform(1, 50) if rng.random() < 0.5 else lo[a] - rng.uniform(1, 50)
            d = rng.uniform(lo, hi) - o
            d /= np.linalg.norm(d)
            if kind == 2:
                d = -d
        elif kind == 3:
            k = int(rng.integers(len(r)))
            o = r[k, 0:3] + rng.uniform(0, 1) * r[k, 3:6] + rng.uniform(0, 1) * r[k, 6:9]
        elif kind == 4:
            d[int(rng.integers(3))] = 0.0
        elif kind == 5:
            a = int(rng.integers(3))
            d = np.zeros(3)
            d[a] = rng.choice([-1.0, 1.0])
        elif kind == 6:
            d *= 10.0 ** rng.uniform(-3, 3)
        elif kind == 7:
            a, b = rng.choice(3, size=2, replace=False)
            o[a] = (lo, hi)[int(rng.integers(2))][a]  # on a face of the scene box,
            d[a] = 0.0                                  # moving within it
            if rng.random() < 0.5:
                o[b] = (lo, hi)[int(rng.integers(2))][b]  # along an edge
                d[b] = 0.0
        rays[i, 0, :3], rays[i, 1, :3] = o, d
    return rays


@pytest.mark.parametrize("policy", ["auto", "trav7-lds1", "trav5-lds0", "reference"])
@pytest.mark.parametrize("name", ["maze10", "corridor", "soup", "lattice"])
def test_query_rays_bit_exact(gpu, ref_lib, name, policy):
    """soup and lattice: the 3-D walk, the general (SLOW) rect test and the
    lattice's tie fallback under caller-supplied rays (tests/test_grid_stress.py
    has the share of each ray kind the search answers)."""
    from mirror_maze import MMError, _lib

    s, _ = _scene(name)
    r = _renderer(s, POLICIES[policy])
    if _unsupported(r, POLICIES[policy]):
        with pytest.raises(MMError) as e:
            r.query_rays(_rays(s, 64, seed=1))
        assert e.value.code == _lib.MM_ERR_UNSUPPORTED
        r.close()
        return
    ref = _ref(ref_lib, name)
    hit = 0
    for n in (1, 63, 64, 4096 + 37):
        rays = _rays(s, n, seed=100 + n)
        key = ("rays", name, n)
        if key not in _CACHE:
            _CACHE[key] = ref.query(rays)
        t_ref, k_ref = _CACHE[key]
        t, k = r.query_rays(rays)
        assert t.shape == (n,) and k.shape == (n,)
        bad = (_bits(t) != t_ref.view(np.uint32)) | (_bits(k) != k_ref)
        assert not bad.any(), (name, policy, n, np.flatnonzero(bad)[:8])
        hit += int((k_ref != A.MISS).sum())
        assert ((k_ref == A.MISS) == (t_ref == np.float32(1e30))).all()
    assert hit > 500  # both answers occur
    r.sync()
    r.close()


# The variant census's scenes (tests/variant_census_support.py) whose grids no other test here reads: name ->
# (upload options, MM_INFO_* facts that pick the query policy among MM_AOV_POLICIES: grid + flat, the general
# grid form on a maze, grid + wide + slow)
MM_INFO_GRID_FACES, MM_INFO_GRID_FLAT = 13, 19
CENSUS_SCENES = {
    "maze80": ({}, {MM_INFO_GRID_FLAT: 1.0, MM_INFO_GRID_FACES: 0.0, MM_INFO_LEAN: 1.0}),
    "maze128": ({}, {MM_INFO_GRID_FLAT: 0.0, MM_INFO_GRID_FACES: 0.0, MM_INFO_LEAN: 1.0}),
    "wide-slow-soup": (None, {MM_INFO_GRID_FLAT: 0.0, MM_INFO_GRID_FACES: 1.0, MM_INFO_LEAN: 0.0}),
}


@pytest.mark.parametrize("name", sorted(CENSUS_SCENES))
def test_census_scenes_queries_and_aov_bit_exact(gpu, ref_lib, name):
    """mm_query_rays (the eight ray kinds) and mm_trace_aov on N = 80 (flat, plain words, beyond N = 64's size),
    N = 128 (a maze in the general form, coarse cells) and the census's smallest wide slow soup."""
    opts, facts = CENSUS_SCENES[name]
    if opts is None:
        import variant_census_support as vc

        opts = vc.WIDE_SLOW_SOUP[1]
    s, u = _scene(name)
    r = _renderer(s, opts)
    assert r.scene_info(MM_INFO_GRID_OK) == 1.0
    assert {k: r.scene_info(k) for k in facts} == facts
    ref = _ref(ref_lib, name)
    hit = total = 0
    for n in (63, 4096 + 37):
        rays = _rays(s, n, seed=100 + n)
        t_ref, k_ref = ref.query(rays)
        t, k = r.query_rays(rays)
        bad = (_bits(t) != t_ref.view(np.uint32)) | (_bits(k) != k_ref)
        assert not bad.any(), (name, n, np.flatnonzero(bad)[:8])
        hit, total = hit + int((k_ref != A.MISS).sum()), total + n
    assert 0.05 * total < hit < 0.95 * total, (hit, total)  # both answers occur (the soup is sparse: 333 hits)
    seen = set()
    for tile in (TILES if u.view_w == VIEW[0] else WIDE_TILES):
        for limit in (1, 15):
            tref = _ref_tile(ref_lib, name, u, limit, tile)
            d = _diffs(_trace(r, u, limit, tile), tref)
            assert not any(d.values()), (name, tile, limit, d)
            seen |= {int(x) for x in np.unique(np.minimum(tref["id"] >> 30, 3))}
    assert 1 in seen, seen  # surfaces were compared
    r.sync()
    r.close()


def test_query_rays_n0_is_ok_without_a_launch(gpu):
    from mirror_maze import _lib

    s, _ = _scene("maze4")
    r = _renderer(s, {})
    before = r.last_call()
    t, k = r.query_rays(np.zeros((0, 2, 4), np.float32))
    assert t.shape == (0,) and k.shape == (0,)
    assert _lib.lib().mm_query_rays(r._ctx, None, 0, None) == _lib.MM_OK
    assert r.last_call() == before
    r.close()


# ---- ordering -------------------------------------------------------------------
def test_aov_calls_around_a_trace_without_a_sync(gpu, ref_lib):
    """AOV call, mm_trace_tile, AOV call back to back on the stream: the traced
    image is the one traced alone, the buffers are the reference's, and each of
    the three numbered calls ends MM_OK."""
    from mirror_maze import make_ext

    s, u = _scene("maze10")
    tile = TILES[0]
    x0, y0, w, h, ys = tile
    cams = np.stack([np.frombuffer(bytes(u.cam), dtype=np.float32)] * 2).copy()
    cams[1, 0] += 1.5
    e = make_ext(8, 8, 8, frame=2)
    r = _renderer(s, {})
    c0 = r.last_call()
    a1 = _trace(r, u, 15, tile, cameras=cams)
    img, _ = r.trace_tile(u, e, x0, y0, w, h, ys)
    a2 = _trace(r, u, 2, tile)
    assert r.last_call() == c0 + 3
    r.sync()
    assert all(r.call_status(c0 + i) for i in (1, 2, 3))
    alone, _ = r.trace_tile(u, e, x0, y0, w, h, ys)
    assert np.array_equal(_bits(img), _bits(alone))
    from test_gpu_camera_sequence import _with_cam

    for f in range(2):
        d = _diffs(a1, _ref_tile(ref_lib, "maze10", _with_cam(u, cams[f]), 15, tile), f)
        assert not any(d.values()), (f, d)
    d = _diffs(a2, _ref_tile(ref_lib, "maze10", u, 2, tile))
    assert not any(d.values()), d
    r.close()


# ---- errors ---------------------------------------------------------------------
def test_error_returns(gpu):
    import torch

    from mirror_maze import Renderer, _lib

    L = _lib.lib()
    s, u = _scene("maze4")
    buf = torch.ones(4096, dtype=torch.float32, device="cuda:0")
    p = buf.data_ptr()
    cam = (_lib.mm_camera * 2)(u.cam, u.cam)

    def aov(ctx, nd=p, al=None, ids=None, cams=None, n=1, tile=(0, 0, 8, 4, 1), limit=15, uni=u):
        a = _lib.mm_aov(nd, al, ids)
        return L.mm_trace_aov(ctx, C.byref(uni), cams, n, limit, *tile, C.byref(a))

    with Renderer(0) as r0:  # no scene uploaded
        assert aov(r0._ctx) == _lib.MM_ERR_NO_SCENE
        assert L.mm_query_rays(r0._ctx, p, 4, p + 1024) == _lib.MM_ERR_NO_SCENE
    r = _renderer(s, {})
    ctx = r._ctx
    inv = _lib.MM_ERR_INVALID
    assert aov(None) == inv                                         # null context
    assert L.mm_query_rays(None, p, 4, p + 1024) == inv
    assert aov(ctx, nd=None) == inv                                 # all three outputs NULL
    assert aov(ctx, n=0) == inv and aov(ctx, n=0, cams=cam) == inv  # no frames
    assert aov(ctx, n=2) == inv                                     # cams = NULL with n_frames > 1
    for tile in [(77, 0, 8, 4, 1), (0, 58, 8, 4, 1), (0, 50, 8, 4, 4), (0, 0, 0, 4, 1), (0, 0, 8, 4, 0)]:
        assert aov(ctx, tile=tile) == inv, tile                     # tile outside the 80x60 frame / empty
    assert aov(ctx, nd=p + 4) == inv and aov(ctx, al=p + 8) == inv and aov(ctx, ids=p + 2) == inv  # misaligned
    assert aov(ctx, limit=32768) == inv
    assert L.mm_query_rays(ctx, p + 4, 4, p + 1024) == inv and L.mm_query_rays(ctx, p, 4, p + 1028) == inv
    assert L.mm_query_rays(ctx, None, 4, p) == inv and L.mm_query_rays(ctx, p, 4, None) == inv
    assert b"mm_query_rays" in L.mm_last_error(ctx)
    # none of these was enqueued or numbered; valid calls still work
    assert r.last_call() == 0
    assert aov(ctx) == _lib.MM_OK and aov(ctx, cams=cam, n=2, nd=None, ids=p) == _lib.MM_OK
    assert L.mm_query_rays(ctx, p, 4, p + 1024) == _lib.MM_OK
    r.sync()
    assert r.last_call() == 3
    r.close()
