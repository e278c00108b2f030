"""mm_accumulate_frames on the GPU against tests/temporal_ref.c on the same
inputs: every comparison is on bits, zero differing elements, nothing excluded
-- the accumulation is specified operation by operation (include/mm_api.h).
The input conditions (what the sequences make every clause decide) are
tests/test_temporal.py's."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import denoise_support as D
import temporal_support as T

pytestmark = pytest.mark.gpu

NAMES = T.NAMES
_CACHE = {}


@pytest.fixture(scope="module")
def tp_lib(tmp_path_factory):
    return T.build_ref(tmp_path_factory.mktemp("temporal_ref"))


@pytest.fixture(scope="module")
def dn_lib(tmp_path_factory):
    return D.build_ref(tmp_path_factory.mktemp("denoise_ref"))


@pytest.fixture(scope="module")
def renderer(gpu):
    from mirror_maze import Renderer

    r = Renderer(0)
    yield r
    r.close()


def _inputs(name, shape):
    """dict of one case: the view's uniform, (x0, y0), cams, the frames and
    guides as CUDA tensors (tc, ta) and as numpy arrays (color, g); the scene
    sequences are traced on the GPU (8 spp), built once, read-only."""
    import torch

    key = (name, shape)
    if key in _CACHE:
        return _CACHE[key]
    from mirror_maze import Renderer, _lib, make_ext

    w, h = shape
    if name == "synthetic":
        cams, color, g = T.synthetic(shape)
        view, (x0, y0) = T.synthetic_view(shape), T.SYN_ORIGIN
        u = _lib.mm_uniform()
        u.view_w, u.view_h = view
        dev = torch.device("cuda:0")
        tc = torch.from_numpy(color).to(dev)
        ta = {k: torch.from_numpy(g[k].view(np.int32) if k == "id" else g[k]).to(dev) for k in NAMES}
    else:
        s, u = T.scene_view(name)
        view = T.VIEW[name]
        cams = T.scene_cameras(name)
        x0, y0 = T.ORIGIN[name][shape]
        with Renderer(0) as r:
            r.upload_scene(s)
            tc, _ = r.trace_tile_cameras(u, cams, make_ext(8, 8, T.MIRROR_LIMIT, frame=3), x0, y0, w, h, 1)
            ta = r.trace_aov(u, cams, T.MIRROR_LIMIT, x0=x0, y0=y0, w=w, h=h, y_stride=1)
            r.sync()
        color = tc.cpu().numpy()
        g = {k: ta[k].cpu().numpy() for k in NAMES}
        g["id"] = g["id"].view(np.uint32)
    for a in (cams, color, *g.values()):
        a.setflags(write=False)
    _CACHE[key] = dict(u=u, view=(float(view[0]), float(view[1])), x0=x0, y0=y0, cams=cams, tc=tc, ta=ta, color=color, g=g)
    return _CACHE[key]


def _ref(tp_lib, name, shape, lo, hi, with_prev, n_max, tol_z=0.02, w_min=0.25):
    """The reference result of frames lo..hi-1, computed once and shared
    (read-only).  with_prev: the history starts from frame 1 of the two-frame
    reference run without prev (alpha 1..2), its guides and its camera."""
    key = ("ref", name, shape, lo, hi, with_prev, n_max, tol_z, w_min)
    if key not in _CACHE:
        c = _inputs(name, shape)
        prev = _prev_np(tp_lib, name, shape, n_max, tol_z, w_min) if with_prev else None
        out, _ = T.accumulate_ref(tp_lib, c["view"], c["cams"][lo:hi], c["color"][lo:hi],
                                  {k: c["g"][k][lo:hi] for k in NAMES}, prev=prev, n_max=n_max, tol_z=tol_z,
                                  w_min=w_min, x0=c["x0"], y0=c["y0"])
        out.setflags(write=False)
        _CACHE[key] = out
    return _CACHE[key]


def _prev_np(tp_lib, name, shape, n_max, tol_z=0.02, w_min=0.25):
    c = _inputs(name, shape)
    two = _ref(tp_lib, name, shape, 0, 2, False, n_max, tol_z, w_min)
    return two[1], {k: c["g"][k][1:2] for k in NAMES}, c["cams"][1]


def _prev_gpu(tp_lib, name, shape, n_max, tol_z=0.02, w_min=0.25):
    """The same prev as CUDA tensors (the colour uploaded from the reference)."""
    import torch

    c = _inputs(name, shape)
    pc, _, pcam = _prev_np(tp_lib, name, shape, n_max, tol_z, w_min)
    return torch.from_numpy(np.array(pc)).to(c["tc"].device), {k: c["ta"][k][1:2] for k in NAMES}, pcam


def _run(r, c, lo, hi, prev=None, **kw):
    return r.accumulate(c["u"], c["cams"][lo:hi], c["tc"][lo:hi], {k: c["ta"][k][lo:hi] for k in NAMES}, prev=prev,
                        x0=c["x0"], y0=c["y0"], **kw)


def _bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint32)


def _unchanged(name, shape):
    c = _inputs(name, shape)
    return (np.array_equal(_bits(c["tc"]), _bits(c["color"]))
            and all(np.array_equal(_bits(c["ta"][k]), _bits(c["g"][k])) for k in NAMES))


@pytest.mark.parametrize("shape", D.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", T.SEQUENCES)
def test_frames_prev_and_caps_bit_exact(renderer, tp_lib, name, shape):
    """n_frames 1, 2 and 4, with and without prev, n_max 1, 4 and 65535: zero
    differing bits against the reference, every pixel of every frame; the
    inputs are as they were."""
    c = _inputs(name, shape)
    for n_max in T.N_MAX:
        for n in (1, 2, T.N_FRAMES):
            for with_prev in (False, True):
                prev = _prev_gpu(tp_lib, name, shape, n_max) if with_prev else None
                got = _run(renderer, c, 0, n, prev=prev, n_max=n_max)
                ref = _ref(tp_lib, name, shape, 0, n, with_prev, n_max)
                assert got.shape == c["tc"][:n].shape
                bad = int((_bits(got) != _bits(ref)).sum())
                assert bad == 0, (name, shape, n_max, n, with_prev, bad)
    assert _unchanged(name, shape)


@pytest.mark.parametrize("tol_z,w_min", [(0.002, 0.25), (0.3, 1.0), (0.02, 0.9), (1e-6, 1e-6)])
@pytest.mark.parametrize("name", T.SEQUENCES)
def test_tolerances_bit_exact(renderer, tp_lib, name, tol_z, w_min):
    for shape in ((67, 5), (130, 9), (3, 40)):
        c = _inputs(name, shape)
        got = _run(renderer, c, 0, T.N_FRAMES, prev=_prev_gpu(tp_lib, name, shape, 32, tol_z, w_min), n_max=32,
                   tol_z=tol_z, w_min=w_min)
        ref = _ref(tp_lib, name, shape, 0, T.N_FRAMES, True, 32, tol_z, w_min)
        bad = int((_bits(got) != _bits(ref)).sum())
        assert bad == 0, (name, shape, tol_z, w_min, bad)
    if name == "corridor":  # the parameters matter on these inputs
        a = _ref(tp_lib, name, (130, 9), 0, T.N_FRAMES, True, 32, 0.002, 0.25)
        assert not np.array_equal(a, _ref(tp_lib, name, (130, 9), 0, T.N_FRAMES, True, 32, 0.3, 1.0))


@pytest.mark.parametrize("name", T.SEQUENCES)
def test_chaining_on_the_gpu(renderer, tp_lib, name):
    """Frames 0..3 in one call equal frames 0..1, then frames 2..3 with prev
    taken from frame 1 of the first call's output, bit for bit; a single-frame
    tensor is one frame; `out` is written in place."""
    import torch

    for shape in ((130, 9), (67, 5)):
        c = _inputs(name, shape)
        whole = _run(renderer, c, 0, T.N_FRAMES, n_max=3)
        head = _run(renderer, c, 0, 2, n_max=3)
        into = torch.zeros_like(c["tc"][2:])
        tail = _run(renderer, c, 2, T.N_FRAMES, prev=(head[1], {k: c["ta"][k][1] for k in NAMES}, c["cams"][1]),
                    n_max=3, out=into)
        assert tail is into
        assert np.array_equal(_bits(whole), _bits(torch.cat([head, tail])))
        assert np.array_equal(_bits(whole), _bits(_ref(tp_lib, name, shape, 0, T.N_FRAMES, False, 3)))
        one = renderer.accumulate(c["u"], c["cams"][:1], c["tc"][0], {k: c["ta"][k][0] for k in NAMES},
                                  x0=c["x0"], y0=c["y0"])
        assert one.shape == c["tc"][0].shape
        assert np.array_equal(_bits(one)[..., :3], _bits(c["color"][0])[..., :3]) and bool((one[..., 3] == 1.0).all())
    assert _unchanged(name, (130, 9)) and _unchanged(name, (67, 5))


def test_back_to_back_calls_of_different_sizes(gpu, tp_lib):
    """A small call, a larger one, the small one again, back to back on a fresh
    context with no sync in between: the first and the third result are equal,
    all three equal the reference, and the inputs are as they were."""
    from mirror_maze import Renderer

    small, large = ("synthetic", (67, 5)), ("corridor", (130, 9))
    cs, cl = _inputs(*small), _inputs(*large)
    with Renderer(0) as r:
        one = _run(r, cs, 0, 2, n_max=4)
        two = _run(r, cl, 0, T.N_FRAMES, n_max=4)
        three = _run(r, cs, 0, 2, n_max=4)
        r.sync()
        assert np.array_equal(_bits(one), _bits(three))
        assert np.array_equal(_bits(one), _bits(_ref(tp_lib, *small, 0, 2, False, 4)))
        assert np.array_equal(_bits(two), _bits(_ref(tp_lib, *large, 0, T.N_FRAMES, False, 4)))
    assert _unchanged(*small) and _unchanged(*large)


@pytest.mark.parametrize("name", T.SEQUENCES)
def test_accumulate_then_denoise_is_the_two_references_composed(renderer, tp_lib, dn_lib, name):
    shape = (130, 9)
    c = _inputs(name, shape)
    acc = _run(renderer, c, 0, T.N_FRAMES)
    got = renderer.denoise(acc, c["ta"])
    ref_acc = _ref(tp_lib, name, shape, 0, T.N_FRAMES, False, 32)
    ref, _ = D.filter_ref(dn_lib, ref_acc, c["g"], **D.DEFAULTS)
    assert np.array_equal(_bits(acc), _bits(ref_acc))
    # The denoiser is specified for distances > 0 only: the synthetic guides' NaN distances give it NaN colours,
    # whose sign and payload neither its specification nor IEEE 754 fixes (the accumulation itself never lets
    # one through).  A NaN must meet a NaN; every other element is compared on bits.
    got_np = got.cpu().numpy()
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got_np), nan) and (name == "synthetic" or not nan.any())
    assert np.array_equal(_bits(got_np)[~nan], _bits(ref)[~nan])
    assert np.array_equal(_bits(got)[..., 3], _bits(ref_acc)[..., 3])  # the history length passes through
    assert _unchanged(name, shape)


def test_errors_with_a_context(renderer, tp_lib):
    """Overlapping out, misaligned pointers and range mistakes return
    MM_ERR_INVALID from a real context and name the call; Renderer.accumulate
    raises on mismatched shapes before calling the library."""
    import torch

    from mirror_maze import _lib

    L, inv, ctx = _lib.lib(), _lib.MM_ERR_INVALID, renderer._ctx
    c = _inputs("synthetic", (67, 5))
    tc, ta = c["tc"], c["ta"]
    n, h, w = tc.shape[:3]
    out = torch.empty_like(tc)
    cams = np.ascontiguousarray(c["cams"])
    a = _lib.mm_aov(*[ta[k].data_ptr() for k in NAMES])
    ok = _lib.mm_temporal_params(32, 0.02, 0.25, 0)

    def call(color=tc.data_ptr(), aov=a, prev=None, p=ok, n=n, x0=c["x0"], y0=c["y0"], w=w, h=h, o=out.data_ptr()):
        return L.mm_accumulate_frames(ctx, C.byref(c["u"]), cams.ctypes.data, color, C.byref(aov),
                                      None if prev is None else C.byref(prev), C.byref(p), n, x0, y0, w, h, o)

    assert call() == _lib.MM_OK
    assert call(o=tc.data_ptr()) == inv and call(o=ta["albedo"].data_ptr()) == inv
    assert call(n=1, o=tc.data_ptr() + 16 * w * h - 16) == inv
    assert call(n=1, o=out.data_ptr() + 8) == inv and call(color=tc.data_ptr() + 4, n=1) == inv
    first = renderer.accumulate(c["u"], cams[:1], tc[:1], {k: ta[k][:1] for k in NAMES}, x0=c["x0"], y0=c["y0"])
    pa = _lib.mm_aov(*[ta[k].data_ptr() for k in NAMES])
    cam0 = _lib.mm_camera.from_buffer_copy(cams[0].tobytes())
    assert call(prev=_lib.mm_temporal_prev(first.data_ptr(), pa, cam0), n=1, color=tc[1:].data_ptr(),
                aov=_lib.mm_aov(*[ta[k][1:].data_ptr() for k in NAMES])) == _lib.MM_OK
    assert call(prev=_lib.mm_temporal_prev(out.data_ptr(), pa, cam0)) == inv  # prev is this call's output
    assert call(prev=_lib.mm_temporal_prev(None, pa, cam0)) == inv
    for bad in ((0, 0.02, 0.25, 0), (65536, 0.02, 0.25, 0), (32, 0.0, 0.25, 0), (32, 0.02, 1.25, 0), (32, 0.02, 0.25, 4)):
        assert call(p=_lib.mm_temporal_params(*bad)) == inv
    assert call(n=0) == inv and call(w=0) == inv and call(h=0) == inv and call(x0=1 << 24) == inv
    assert b"mm_accumulate_frames" in L.mm_last_error(ctx)
    renderer.sync()
    assert _unchanged("synthetic", (67, 5))
    with pytest.raises(ValueError):
        renderer.accumulate(c["u"], cams[:2], tc, ta)                                    # camera count
    with pytest.raises(ValueError):
        renderer.accumulate(c["u"], cams, tc, {k: v[:1] for k, v in ta.items()})         # frame counts differ
    with pytest.raises(ValueError):
        renderer.accumulate(c["u"], cams, tc.double(), ta)                               # dtype
    with pytest.raises(ValueError):
        renderer.accumulate(c["u"], cams, tc, ta, n_max=0)
    with pytest.raises(ValueError):
        renderer.accumulate(c["u"], cams, tc, ta, prev=(tc[0, :, :-1].contiguous(), ta, cams[0]))
    with pytest.raises(ValueError):
        renderer.accumulate(c["u"], cams, tc, ta, out=torch.empty((n, h, w, 3), device=tc.device))
