"""mm_denoise_frames on the GPU against tests/denoise_ref.c on the same inputs:
every comparison is on bits, zero differing elements, nothing excluded -- the
filter is specified operation by operation (include/mm_api.h), so there is
nothing to excuse.  The input conditions (what the synthetic guides and the
two scenes make the filter's clauses decide) are tests/test_denoise.py's."""
from __future__ import annotations

import ctypes as C
import itertools

import numpy as np
import pytest

import denoise_support as D

pytestmark = pytest.mark.gpu

NAMES = ("normal_depth", "albedo", "id")
# the tiles the real guides are traced over, one per scene and D.SHAPES entry: (x0, y0, y_stride) inside VIEW
VIEW = {"maze4": (160, 120), "corridor": (140, 48)}
# around the horizon, where walls, floor and (in the corridor) the mirror chains and the open end meet
ORIGIN = {"maze4": {(67, 5): (40, 54, 3), (64, 1): (50, 61, 1), (1, 1): (80, 63, 1), (3, 40): (78, 40, 1),
                    (130, 9): (15, 50, 2)},
          "corridor": {(67, 5): (40, 18, 3), (64, 1): (50, 25, 1), (1, 1): (70, 25, 1), (3, 40): (70, 4, 1),
                       (130, 9): (6, 16, 2)}}
N_FRAMES = 3
GUIDES = ["maze4", "corridor", "synthetic"]
_CACHE = {}


@pytest.fixture(scope="module")
def dn_lib(tmp_path_factory):
    return D.build_ref(tmp_path_factory.mktemp("denoise_ref"))


@pytest.fixture(scope="module")
def renderer(gpu):
    """One context for the whole module: its scratch is reused and regrown
    across every call below, in whatever order the tests run."""
    from mirror_maze import Renderer

    r = Renderer(0)
    yield r
    r.close()


def _inputs(name, shape):
    """(color (3, h, w, 4) CUDA tensor, aov dict of CUDA tensors, the same as
    numpy arrays), three frames with different content; built once, read-only."""
    import torch

    key = (name, shape)
    if key in _CACHE:
        return _CACHE[key]
    w, h = shape
    if name == "synthetic":
        color, g = D.synthetic(N_FRAMES, h, w, seed=w * 1000 + h)
        dev = torch.device("cuda:0")
        tc = torch.from_numpy(color).to(dev)
        ta = {k: torch.from_numpy(g[k].view(np.int32) if k == "id" else g[k]).to(dev) for k in NAMES}
    else:
        from mirror_maze import Renderer, make_ext

        s, u = (D.maze_view if name == "maze4" else D.corridor_view)(*VIEW[name])
        base = np.frombuffer(bytes(u.cam), dtype=np.float32)
        cams = np.tile(base, (N_FRAMES, 1))
        cams[:, 0] += 0.013 * np.arange(N_FRAMES, dtype=np.float32)  # a few centimetres per frame
        cams[:, 2] += 0.021 * np.arange(N_FRAMES, dtype=np.float32)
        x0, y0, ys = ORIGIN[name][shape]
        with Renderer(0) as r:
            r.upload_scene(s)
            tc, _ = r.trace_tile_cameras(u, cams, make_ext(8, 8, 8, frame=3), x0, y0, w, h, ys)
            ta = r.trace_aov(u, cams, 8, x0=x0, y0=y0, w=w, h=h, y_stride=ys)
            r.sync()
        color = tc.cpu().numpy()
        g = {k: ta[k].cpu().numpy() for k in NAMES}
        g["id"] = g["id"].view(np.uint32)
    for a in (color, *g.values()):
        a.setflags(write=False)
    _CACHE[key] = (tc, ta, color, g)
    return _CACHE[key]


def _ref(dn_lib, name, shape, n, n_passes, sigma_z, sigma_l):
    """The reference result of the first n frames, computed once and shared (read-only)."""
    key = ("ref", name, shape, n, n_passes, sigma_z, sigma_l)
    if key not in _CACHE:
        _, _, color, g = _inputs(name, shape)
        out, _ = D.filter_ref(dn_lib, color[:n], {k: g[k][:n] for k in NAMES}, n_passes, sigma_z, sigma_l)
        out.setflags(write=False)
        _CACHE[key] = out
    return _CACHE[key]


def _bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint32)


def _first(tc, ta, n):
    return tc[:n], {k: ta[k][:n] for k in NAMES}


def _unchanged(name, shape):
    tc, ta, color, g = _inputs(name, shape)
    return np.array_equal(_bits(tc), _bits(color)) and all(np.array_equal(_bits(ta[k]), _bits(g[k])) for k in NAMES)


@pytest.mark.parametrize("shape", D.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", GUIDES)
def test_passes_and_frames_bit_exact(renderer, dn_lib, name, shape):
    """n_passes 1..5 and 8, one frame and three: zero differing bits.  Frame
    f of a three-frame call must not see frame f +- 1: the reference filters
    every frame on its own, and the frames differ."""
    tc, ta, color, _ = _inputs(name, shape)
    assert not np.array_equal(color[0], color[1]) or shape == (1, 1)
    for n, n_passes in itertools.product((1, N_FRAMES), D.PASSES):
        c, a = _first(tc, ta, n)
        got = renderer.denoise(c, a, n_passes=n_passes)
        ref = _ref(dn_lib, name, shape, n, n_passes, 0.02, 0.5)
        assert got.shape == c.shape
        bad = int((_bits(got) != _bits(ref)).sum())
        assert bad == 0, (name, shape, n, n_passes, bad)
    assert _unchanged(name, shape)


@pytest.mark.parametrize("name", GUIDES)
def test_a_single_frame_tensor_is_one_frame(renderer, dn_lib, name):
    shape = (67, 5)
    tc, ta, _, _ = _inputs(name, shape)
    got = renderer.denoise(tc[0], {k: v[:1] for k, v in ta.items()})
    assert got.shape == tc[0].shape
    assert np.array_equal(_bits(got), _bits(_ref(dn_lib, name, shape, 1, 4, 0.02, 0.5))[0])


@pytest.mark.parametrize("sigma_z,sigma_l", [(0.02, 0.5), (0.0, 0.5), (0.02, 0.0), (-1.0, -0.5), (0.3, 0.05)])
@pytest.mark.parametrize("name", GUIDES)
def test_terms_on_and_off_bit_exact(renderer, dn_lib, name, sigma_z, sigma_l):
    for shape in ((67, 5), (130, 9)):
        tc, ta, _, _ = _inputs(name, shape)
        got = renderer.denoise(tc, ta, n_passes=3, sigma_z=sigma_z, sigma_l=sigma_l)
        ref = _ref(dn_lib, name, shape, N_FRAMES, 3, sigma_z, sigma_l)
        bad = int((_bits(got) != _bits(ref)).sum())
        assert bad == 0, (name, shape, sigma_z, sigma_l, bad)
    if name == "synthetic":  # the terms matter on these inputs: turning one off changes the result
        on = _ref(dn_lib, name, (130, 9), N_FRAMES, 3, 0.02, 0.5)
        assert not np.array_equal(on, _ref(dn_lib, name, (130, 9), N_FRAMES, 3, 0.0, 0.5))
        assert not np.array_equal(on, _ref(dn_lib, name, (130, 9), N_FRAMES, 3, 0.02, 0.0))


@pytest.mark.parametrize("name", GUIDES)
def test_rgba8_output_is_quantize_of_the_float_output(renderer, dn_lib, name):
    import torch

    for shape, n_passes in itertools.product(D.SHAPES, (1, 2, 4)):
        tc, ta, _, _ = _inputs(name, shape)
        f = renderer.denoise(tc, ta, n_passes=n_passes)
        q = renderer.denoise(tc, ta, n_passes=n_passes, rgba8=True)
        assert q.dtype == torch.uint8 and q.shape == tc.shape
        assert torch.equal(q, renderer.quantize(f)), (name, shape, n_passes)
        into = torch.zeros(tc.shape, dtype=torch.uint8, device=tc.device)
        assert renderer.denoise(tc, ta, n_passes=n_passes, out=into) is into and torch.equal(into, q)
        assert np.array_equal(_bits(f), _bits(_ref(dn_lib, name, shape, N_FRAMES, n_passes, 0.02, 0.5)))
    # alpha passes through the filter; the trace writes 1
    assert int(q[..., 3].min()) == 255


def test_scratch_regrows_and_is_reused_without_a_sync(gpu, dn_lib):
    """A small call, a larger one (the scratch regrows), the small one again,
    back to back on a fresh context with no sync in between: the first and the
    third result are equal, all three equal the reference, and the inputs are
    as they were."""
    from mirror_maze import Renderer

    small, large = ("synthetic", (67, 5)), ("corridor", (130, 9))
    (sc, sa, _, _), (lc, la, _, _) = _inputs(*small), _inputs(*large)
    with Renderer(0) as r:
        one = r.denoise(*_first(sc, sa, 1), n_passes=5)
        two = r.denoise(lc, la, n_passes=5)
        three = r.denoise(*_first(sc, sa, 1), n_passes=5)
        r.sync()
        assert np.array_equal(_bits(one), _bits(three))
        assert np.array_equal(_bits(one), _bits(_ref(dn_lib, *small, 1, 5, 0.02, 0.5)))
        assert np.array_equal(_bits(two), _bits(_ref(dn_lib, *large, N_FRAMES, 5, 0.02, 0.5)))
        assert np.array_equal(_bits(three), _bits(_ref(dn_lib, *small, 1, 5, 0.02, 0.5)))
    assert _unchanged(*small) and _unchanged(*large)


def test_calls_on_two_streams_share_the_scratch_in_order(gpu, dn_lib):
    """The renderer follows torch's current stream; calls alternating between
    two streams still take turns on the context's scratch."""
    import torch

    from mirror_maze import Renderer

    name, shape = "synthetic", (130, 9)
    tc, ta, _, _ = _inputs(name, shape)
    ref = _ref(dn_lib, name, shape, N_FRAMES, 5, 0.02, 0.5)
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = []
    with Renderer(0) as r:
        for i in range(6):
            with torch.cuda.stream(streams[i & 1]):
                outs.append(r.denoise(tc, ta, n_passes=5))
        torch.cuda.synchronize()
        assert all(np.array_equal(_bits(o), _bits(ref)) for o in outs)


def test_errors_with_a_context(renderer):
    """Overlapping out / color, misaligned pointers and the null and range
    mistakes return MM_ERR_INVALID from a real context; Renderer.denoise
    raises on mismatched shapes, dtypes and devices before calling the library."""
    import torch

    from mirror_maze import _lib

    L, inv, ctx = _lib.lib(), _lib.MM_ERR_INVALID, renderer._ctx
    tc, ta, _, _ = _inputs("synthetic", (67, 5))
    n, h, w = tc.shape[:3]
    out = torch.empty_like(tc)
    a = _lib.mm_aov(*[ta[k].data_ptr() for k in NAMES])
    ok = _lib.mm_denoise_params(4, 0.02, 0.5, 0)
    r8 = _lib.mm_denoise_params(4, 0.02, 0.5, _lib.MM_DN_RGBA8)

    def call(color=tc.data_ptr(), aov=a, p=ok, n=n, w=w, h=h, o=out.data_ptr()):
        return L.mm_denoise_frames(ctx, color, C.byref(aov) if aov is not None else None,
                                   C.byref(p) if p is not None else None, n, w, h, o)

    assert call() == _lib.MM_OK
    # overlap: in place, and an output that starts inside the colour buffer
    assert call(o=tc.data_ptr()) == inv
    two = torch.cat([tc[:1], tc[:1]])  # a colour frame with room for one more behind it
    assert call(color=two.data_ptr(), n=1, o=two.data_ptr() + 16 * w * h - 16) == inv
    assert call(color=two.data_ptr(), n=1, o=two.data_ptr() + 16 * w * h) == _lib.MM_OK  # beside it: no overlap
    assert call(color=two.data_ptr(), n=1, p=r8, o=two.data_ptr() + 16 * w * h - 4) == inv
    assert call(color=two.data_ptr() + 16 * w * h, n=1, o=two.data_ptr() + 16) == inv
    assert torch.equal(two[0], tc[0])
    assert call(o=ta["normal_depth"].data_ptr()) == inv
    # misaligned: float4 buffers need 16 bytes, the id buffer and an RGBA8 output 4
    assert call(color=tc.data_ptr() + 4, n=1) == inv
    assert call(o=out.data_ptr() + 8, n=1) == inv
    assert call(p=r8, o=out.data_ptr() + 2, n=1) == inv
    assert call(p=r8, o=out.data_ptr() + 4, n=1) == _lib.MM_OK
    for k, off in (("normal_depth", 8), ("albedo", 4), ("id", 2)):
        ptrs = {m: ta[m].data_ptr() for m in NAMES}
        ptrs[k] += off
        assert call(aov=_lib.mm_aov(*[ptrs[m] for m in NAMES]), n=1) == inv, k
    # nulls and ranges, as tests/test_denoise.py has them without a context
    assert call(color=None) == inv and call(o=None) == inv and call(aov=None) == inv and call(p=None) == inv
    assert call(aov=_lib.mm_aov(ta["normal_depth"].data_ptr(), None, ta["id"].data_ptr())) == inv
    for bad in ((0, 0), (9, 0), (4, 2), (4, 0x10)):
        assert call(p=_lib.mm_denoise_params(bad[0], 0.02, 0.5, bad[1])) == inv
    assert call(n=0) == inv and call(w=0) == inv and call(h=0) == inv
    assert b"mm_denoise_frames" in L.mm_last_error(ctx)
    renderer.sync()
    assert _unchanged("synthetic", (67, 5))
    # the Python wrapper
    with pytest.raises(ValueError):
        renderer.denoise(tc, {k: v[:1] for k, v in ta.items()})          # frame counts differ
    with pytest.raises(ValueError):
        renderer.denoise(tc[:, :, :-1].contiguous(), ta)                   # widths differ
    with pytest.raises(ValueError):
        renderer.denoise(tc.double(), ta)                                  # dtype
    with pytest.raises(ValueError):
        renderer.denoise(tc, {**ta, "id": ta["id"].to(torch.int64)})       # dtype of a guide
    with pytest.raises(ValueError):
        renderer.denoise(tc, {**ta, "albedo": ta["albedo"].cpu()})         # device
    with pytest.raises(ValueError):
        renderer.denoise(tc, {k: ta[k] for k in NAMES[:2]})                # a guide is missing
    with pytest.raises(ValueError):
        renderer.denoise(tc, ta, out=torch.empty((n, h, w, 3), device=tc.device))
    with pytest.raises(ValueError):
        renderer.denoise(tc, ta, n_passes=9)
