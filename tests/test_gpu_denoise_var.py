"""mm_denoise_frames_var on the GPU against tests/denoise_var_ref.c on the same
inputs: every comparison, colour and variance, is on bits, zero differing
elements, nothing excluded -- the filter is specified operation by operation
(include/mm_api.h).  The input conditions (what the synthetic guides and the
synthetic variance make the filter's clauses decide) are tests/test_denoise_var.py's."""
from __future__ import annotations

import ctypes as C
import itertools

import numpy as np
import pytest

import denoise_var_support as V
from test_gpu_denoise import GUIDES, N_FRAMES, NAMES, ORIGIN, VIEW

pytestmark = pytest.mark.gpu

SPP = 8
_CACHE = {}


@pytest.fixture(scope="module")
def dnv_lib(tmp_path_factory):
    return V.build_ref(tmp_path_factory.mktemp("denoise_var_ref"))


@pytest.fixture(scope="module")
def renderer(gpu):
    """One context for the whole module: its scratch is reused and regrown
    across every call below, in whatever order the tests run."""
    from mirror_maze import Renderer

    r = Renderer(0)
    yield r
    r.close()


def _inputs(name, shape):
    """(color (3, h, w, 4), aov dict, var (3, h, w): CUDA tensors; the same as
    numpy arrays), three frames with different content; built once, read-only.
    var is the variance of ONE sample (trace_tile_var's at 8 spp; for the
    synthetic case SPP times the synthetic variance of the mean, which the
    division by SPP, a power of two, gives back exactly)."""
    import torch

    key = (name, shape)
    if key in _CACHE:
        return _CACHE[key]
    w, h = shape
    dev = torch.device("cuda:0")
    if name == "synthetic":
        color, g = V.synthetic(N_FRAMES, h, w, seed=w * 1000 + h)
        var = V.synthetic_var(N_FRAMES, h, w, seed=w * 1000 + h) * np.float32(SPP)
        tc = torch.from_numpy(color).to(dev)
        ta = {k: torch.from_numpy(g[k].view(np.int32) if k == "id" else g[k]).to(dev) for k in NAMES}
        tv = torch.from_numpy(var).to(dev)
    else:
        from mirror_maze import Renderer, make_ext, mm_camera, mm_uniform

        s, u = (V.maze_view if name == "maze4" else V.corridor_view)(*VIEW[name])
        base = np.frombuffer(bytes(u.cam), dtype=np.float32)
        cams = np.tile(base, (N_FRAMES, 1))
        cams[:, 0] += 0.013 * np.arange(N_FRAMES, dtype=np.float32)  # a few centimetres per frame
        cams[:, 2] += 0.021 * np.arange(N_FRAMES, dtype=np.float32)
        x0, y0, ys = ORIGIN[name][shape]
        tc = torch.empty((N_FRAMES, h, w, 4), dtype=torch.float32, device=dev)
        tv = torch.empty((N_FRAMES, h, w), dtype=torch.float32, device=dev)
        with Renderer(0) as r:
            r.upload_scene(s)
            for f in range(N_FRAMES):  # frame by frame: a variance call of several frames of a small tile has no plan
                uf = mm_uniform.from_buffer_copy(u)
                uf.cam = mm_camera.from_buffer_copy(cams[f].tobytes())
                r.trace_tile_var(uf, make_ext(SPP, 8, 8, frame=3 + f), x0, y0, w, h, ys, out=tc[f], var=tv[f])
            ta = r.trace_aov(u, cams, 8, x0=x0, y0=y0, w=w, h=h, y_stride=ys)
            r.sync()
        color, var = tc.cpu().numpy(), tv.cpu().numpy()
        g = {k: ta[k].cpu().numpy() for k in NAMES}
        g["id"] = g["id"].view(np.uint32)
    for a in (color, var, *g.values()):
        a.setflags(write=False)
    _CACHE[key] = (tc, ta, tv, color, g, var)
    return _CACHE[key]


def _ref(dnv_lib, name, shape, n, n_passes, params):
    """The reference (colour, variance) of the first n frames, computed once and shared (read-only)."""
    key = ("ref", name, shape, n, n_passes, params)
    if key not in _CACHE:
        _, _, tv, color, g, _ = _inputs(name, shape)
        vmean = (tv[:n] / SPP).cpu().numpy()  # formed where Renderer.denoise_var forms it
        if name == "synthetic" and n == N_FRAMES:  # the subnormals and the zeros are still there
            assert np.array_equal(vmean, V.synthetic_var(N_FRAMES, shape[1], shape[0], seed=shape[0] * 1000 + shape[1]))
        out, vout, _ = V.filter_ref(dnv_lib, color[:n], {k: g[k][:n] for k in NAMES}, vmean, n_passes, *params)
        out.setflags(write=False)
        vout.setflags(write=False)
        _CACHE[key] = (out, vout)
    return _CACHE[key]


def _bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint32)


def _first(name, shape, n):
    tc, ta, tv = _inputs(name, shape)[:3]
    return tc[:n], {k: ta[k][:n] for k in NAMES}, tv[:n]


def _unchanged(name, shape):
    tc, ta, tv, color, g, var = _inputs(name, shape)
    return (np.array_equal(_bits(tc), _bits(color)) and np.array_equal(_bits(tv), _bits(var))
            and all(np.array_equal(_bits(ta[k]), _bits(g[k])) for k in NAMES))


def _differ(got, ref):
    return int((_bits(got[0]) != _bits(ref[0])).sum()), int((_bits(got[1]) != _bits(ref[1])).sum())


def _run(r, name, shape, n, n_passes, params, **kw):
    c, a, v = _first(name, shape, n)
    return r.denoise_var(c, a, v, SPP, n_passes=n_passes, sigma_z=params[0], sigma_l=params[1], eps_l=params[2], **kw)


@pytest.mark.parametrize("shape", V.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", GUIDES)
def test_passes_and_frames_bit_exact(renderer, dnv_lib, name, shape):
    """n_passes 1, 2, 3, 5 and 8, one frame and three: colour and variance,
    zero differing bits.  Frame f of a three-frame call must not see frame
    f +- 1: the reference filters every frame on its own, and the frames differ."""
    color = _inputs(name, shape)[3]
    assert not np.array_equal(color[0], color[1]) or shape == (1, 1)
    for n, n_passes in itertools.product((1, N_FRAMES), V.PASSES):
        got = _run(renderer, name, shape, n, n_passes, V.MAIN, return_var=True)
        assert got[0].shape == (n, shape[1], shape[0], 4) and got[1].shape == (n, shape[1], shape[0])
        bad = _differ(got, _ref(dnv_lib, name, shape, n, n_passes, V.MAIN))
        assert bad == (0, 0), (name, shape, n, n_passes, bad)
    assert _unchanged(name, shape)


@pytest.mark.parametrize("params", [V.MAIN, (0.0, 4.0, 1e-3), (0.02, 0.0, 0.0), (-1.0, -0.5, -1.0), V.TINY],
                         ids=["both", "l", "z", "none", "tiny-stop"])
@pytest.mark.parametrize("name", GUIDES)
def test_terms_on_and_off_bit_exact(renderer, dnv_lib, name, params):
    """The four combinations of the two terms, and the tiny stop (pixels that
    leave the fast form's ranges; weights and squared weights that underflow).
    With the luminance term off the colour is Renderer.denoise's with
    sigma_l = 0, on all bits."""
    for shape in ((67, 5), (130, 9)):
        got = _run(renderer, name, shape, N_FRAMES, 3, params, return_var=True)
        bad = _differ(got, _ref(dnv_lib, name, shape, N_FRAMES, 3, params))
        assert bad == (0, 0), (name, shape, params, bad)
        if not params[1] > 0:
            c, a, _ = _first(name, shape, N_FRAMES)
            plain = renderer.denoise(c, a, n_passes=3, sigma_z=params[0], sigma_l=0.0)
            assert np.array_equal(_bits(got[0]), _bits(plain)), (name, shape, params)
    if name == "synthetic":  # the terms and the stop matter on these inputs
        on = _ref(dnv_lib, name, (130, 9), N_FRAMES, 3, V.MAIN)
        for other in ((0.0, 4.0, 1e-3), (0.02, 0.0, 0.0), V.TINY):
            off = _ref(dnv_lib, name, (130, 9), N_FRAMES, 3, other)
            assert not np.array_equal(on[0], off[0]) and not np.array_equal(on[1], off[1])


@pytest.mark.parametrize("name", GUIDES)
def test_optional_outputs(renderer, dnv_lib, name):
    """Without a variance output the colour bits are the same; the RGBA8 output
    is quantize of the float output; given tensors are filled and returned."""
    import torch

    for shape, n_passes in itertools.product(V.SHAPES, (1, 2, 5)):
        ref = _ref(dnv_lib, name, shape, N_FRAMES, n_passes, V.MAIN)
        f = _run(renderer, name, shape, N_FRAMES, n_passes, V.MAIN)
        assert torch.is_tensor(f) and np.array_equal(_bits(f), _bits(ref[0])), (name, shape, n_passes)
        q, qv = _run(renderer, name, shape, N_FRAMES, n_passes, V.MAIN, rgba8=True, return_var=True)
        assert q.dtype == torch.uint8 and q.shape == f.shape
        assert torch.equal(q, renderer.quantize(f)) and np.array_equal(_bits(qv), _bits(ref[1]))
        assert torch.equal(_run(renderer, name, shape, N_FRAMES, n_passes, V.MAIN, rgba8=True), q)
        into, vinto = torch.zeros_like(q), torch.full_like(qv, -1.0)
        got = _run(renderer, name, shape, N_FRAMES, n_passes, V.MAIN, out=into, var_out=vinto)
        assert got[0] is into and got[1] is vinto and torch.equal(into, q) and torch.equal(vinto, qv)
    assert int(q[..., 3].min()) == 255  # alpha passes through the filter; the trace writes 1
    assert _unchanged(name, shape)


def test_a_single_frame_tensor_is_one_frame(renderer, dnv_lib):
    shape = (67, 5)
    tc, ta, tv = _inputs("corridor", shape)[:3]
    out, vout = renderer.denoise_var(tc[0], {k: v[:1] for k, v in ta.items()}, tv[0], SPP, n_passes=5, sigma_z=V.MAIN[0],
                                     sigma_l=V.MAIN[1], eps_l=V.MAIN[2], return_var=True)
    assert out.shape == tc[0].shape and vout.shape == tv[0].shape
    ref = _ref(dnv_lib, "corridor", shape, 1, 5, V.MAIN)
    assert np.array_equal(_bits(out), _bits(ref[0][0])) and np.array_equal(_bits(vout), _bits(ref[1][0]))


def test_non_uniform_counts_after_a_refine_round(gpu, dnv_lib):
    """One refine round on the corridor tile leaves pixels with 8 and with 32
    samples side by side; the call on var / count equals the reference on the
    same arrays."""
    import torch

    from mirror_maze import Renderer, make_ext

    w, h = VIEW["corridor"]
    s, u = V.corridor_view(w, h)
    e = make_ext(SPP, 8, 8, frame=3)
    with Renderer(0) as r:
        r.upload_scene(s)
        color, var, _ = r.trace_tile_var(u, e, 0, 0, w, h)
        aov = r.trace_aov(u, None, 8, x0=0, y0=0, w=w, h=h)
        count = torch.full((h, w), float(SPP), dtype=torch.float32, device=color.device)
        n_sel = r.refine(u, e, color, var, count, 0.05, 24, 2**20, ids=aov["id"][0])
        assert 0 < n_sel < w * h and sorted(np.unique(count.cpu().numpy())) == [8.0, 32.0]
        held = [t.clone() for t in (color, var, count)]
        out, vout = r.denoise_var(color, aov, var, count, n_passes=5, sigma_z=V.MAIN[0], sigma_l=V.MAIN[1],
                                  eps_l=V.MAIN[2], return_var=True)
        r.sync()
        assert all(torch.equal(a, b) for a, b in zip(held, (color, var, count)))
    g = {k: aov[k].cpu().numpy() for k in NAMES}
    g["id"] = g["id"].view(np.uint32)
    vmean = (var / count).cpu().numpy()
    ref = V.filter_ref(dnv_lib, color.cpu().numpy(), g, vmean, 5, *V.MAIN)
    assert _differ((out[None], vout[None]), ref[:2]) == (0, 0)


def test_scratch_regrows_and_is_reused_without_a_sync(gpu, dnv_lib):
    """A small call, a larger one (the colour and the variance scratch regrow),
    the small one again, back to back on a fresh context with no sync in
    between: the first and the third result are equal, all three equal the
    reference, and the inputs are as they were."""
    from mirror_maze import Renderer

    small, large = ("synthetic", (67, 5)), ("corridor", (130, 9))
    with Renderer(0) as r:
        one = _run(r, *small, 1, 5, V.MAIN, return_var=True)
        two = _run(r, *large, N_FRAMES, 5, V.MAIN, return_var=True)
        three = _run(r, *small, 1, 5, V.MAIN, return_var=True)
        r.sync()
        assert _differ(one, three) == (0, 0)
        assert _differ(one, _ref(dnv_lib, *small, 1, 5, V.MAIN)) == (0, 0)
        assert _differ(two, _ref(dnv_lib, *large, N_FRAMES, 5, V.MAIN)) == (0, 0)
    assert _unchanged(*small) and _unchanged(*large)


def test_calls_on_two_streams_and_both_filters_share_the_scratch_in_order(gpu, dnv_lib):
    """The renderer follows torch's current stream; calls alternating between
    two streams, and between denoise_var and denoise, still take turns on the
    context's scratch: every result equals its reference (denoise's is
    denoise_var's with the luminance term off, tests/test_denoise_var.py)."""
    import torch

    from mirror_maze import Renderer

    name, shape = "synthetic", (130, 9)
    c, a, _ = _first(name, shape, N_FRAMES)
    ref = _ref(dnv_lib, name, shape, N_FRAMES, 5, V.MAIN)
    plain_ref = _ref(dnv_lib, name, shape, N_FRAMES, 5, (0.02, 0.0, 0.0))[0]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    with Renderer(0) as r:
        outs, plains = [], []
        for i in range(6):  # var, plain on one stream, then on the other, ...
            with torch.cuda.stream(streams[i & 1]):
                outs.append(_run(r, name, shape, N_FRAMES, 5, V.MAIN, return_var=True))
                plains.append(r.denoise(c, a, n_passes=5, sigma_z=0.02, sigma_l=0.0))
        for i in range(4):  # the same interleaving on one stream
            outs.append(_run(r, name, shape, N_FRAMES, 5, V.MAIN, return_var=True))
            plains.append(r.denoise(c, a, n_passes=5, sigma_z=0.02, sigma_l=0.0))
        torch.cuda.synchronize()
        assert all(_differ(o, ref) == (0, 0) for o in outs)
        assert all(np.array_equal(_bits(p), _bits(plain_ref)) for p in plains)
    assert _unchanged(name, shape)


def test_errors_with_a_context(renderer):
    """The new rejections return MM_ERR_INVALID from a real context, under this
    call's name, and their neighbours that are in order return MM_OK;
    Renderer.denoise_var raises on mismatched shapes, dtypes and devices before
    calling the library."""
    import torch

    from mirror_maze import _lib

    L, inv, ctx = _lib.lib(), _lib.MM_ERR_INVALID, renderer._ctx
    name, shape = "synthetic", (67, 5)
    tc, ta, tv = _inputs(name, shape)[:3]
    n, h, w = tc.shape[:3]
    vm = (tv / SPP).contiguous()
    out, vout = torch.empty_like(tc), torch.empty_like(vm)
    a = _lib.mm_aov(*[ta[k].data_ptr() for k in NAMES])

    def params(n_passes=5, sigma_z=0.02, sigma_l=4.0, eps_l=1e-3, flags=0, reserved=0):
        return _lib.mm_denoise_var_params(n_passes, sigma_z, sigma_l, eps_l, flags, reserved)

    def call(color=tc.data_ptr(), aov=a, v=vm.data_ptr(), p=params(), n=n, w=w, h=h, o=out.data_ptr(),
             vo=vout.data_ptr()):
        return L.mm_denoise_frames_var(ctx, color, C.byref(aov) if aov is not None else None, v,
                                       C.byref(p) if p is not None else None, n, w, h, o, vo)

    assert call() == _lib.MM_OK and call(vo=None) == _lib.MM_OK
    # the variance input: null, misaligned
    assert call(v=None) == inv and call(v=vm.data_ptr() + 2, n=1) == inv
    assert call(v=vm.data_ptr() + 4, n=1) == _lib.MM_OK
    assert call(vo=vout.data_ptr() + 2, n=1) == inv
    # eps_l with the luminance term on and off; flags; reserved
    for eps in (0.0, -1e-3, float("inf"), float("nan")):
        assert call(p=params(eps_l=eps)) == inv
        assert call(p=params(sigma_l=0.0, eps_l=eps)) == _lib.MM_OK
    assert b"eps_l" in L.mm_last_error(ctx)
    assert call(p=params(flags=2)) == inv and call(p=params(flags=0x80000001)) == inv
    assert call(p=params(reserved=1)) == inv
    assert call(p=params(n_passes=0)) == inv and call(p=params(n_passes=9)) == inv
    # overlaps: an output on an input, on the variance input, the outputs on each other
    assert call(o=tc.data_ptr()) == inv and call(vo=vm.data_ptr()) == inv and call(o=vm.data_ptr(), n=1, w=4, h=1) == inv
    assert call(vo=tc.data_ptr()) == inv and call(vo=ta["id"].data_ptr()) == inv
    assert call(vo=out.data_ptr() + 16 * n * w * h - 4) == inv
    two = torch.empty((2, n, h, w), dtype=torch.float32, device=tc.device)  # two variance images side by side
    two[0] = vm
    assert call(v=two.data_ptr(), vo=two.data_ptr() + 4 * n * w * h - 4) == inv
    assert call(v=two.data_ptr(), vo=two.data_ptr() + 4 * n * w * h) == _lib.MM_OK  # beside it: no overlap
    assert torch.equal(two[0], vm)
    # what mm_denoise_frames rejects
    assert call(color=None) == inv and call(o=None) == inv and call(aov=None) == inv and call(p=None) == inv
    assert call(aov=_lib.mm_aov(ta["normal_depth"].data_ptr(), None, ta["id"].data_ptr())) == inv
    assert call(color=tc.data_ptr() + 4, n=1) == inv and call(o=out.data_ptr() + 8, n=1) == inv
    assert call(n=0) == inv and call(w=0) == inv and call(h=0) == inv
    assert b"mm_denoise_frames_var" in L.mm_last_error(ctx)
    renderer.sync()
    assert _unchanged(name, shape)
    # the Python wrapper
    kw = dict(n_passes=5)
    with pytest.raises(ValueError):
        renderer.denoise_var(tc, ta, tv[:1], SPP, **kw)                              # frame counts differ
    with pytest.raises(ValueError):
        renderer.denoise_var(tc, ta, tv.double(), SPP, **kw)                         # dtype of the variance
    with pytest.raises(ValueError):
        renderer.denoise_var(tc, ta, tv.cpu(), SPP, **kw)                            # device
    with pytest.raises(ValueError):
        renderer.denoise_var(tc, ta, tv, torch.full_like(tv[0], 8.0), **kw)          # count's shape
    with pytest.raises(ValueError):
        renderer.denoise_var(tc, ta, tv, 0, **kw)                                    # no samples
    with pytest.raises(ValueError):
        renderer.denoise_var(tc, {k: ta[k] for k in NAMES[:2]}, tv, SPP, **kw)       # a guide is missing
    with pytest.raises(ValueError):
        renderer.denoise_var(tc, ta, tv, SPP, var_out=torch.empty_like(tc), **kw)    # var_out's shape
    with pytest.raises(ValueError):
        renderer.denoise_var(tc, ta, tv, SPP, n_passes=9)
