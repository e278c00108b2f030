"""mm_upsample_frames and mm_fill_pixels on the GPU against tests/upsample_ref.c
on the same inputs: every comparison is on bits, zero differing elements,
nothing excluded -- both calls are specified operation by operation
(include/mm_api.h).  The input conditions (what the synthetic and the scene
inputs make every clause decide) are tests/test_upsample.py's."""
from __future__ import annotations

import numpy as np
import pytest

import upsample_support as U

pytestmark = pytest.mark.gpu

NAMES = U.NAMES


@pytest.fixture(scope="module")
def up_lib(tmp_path_factory):
    return U.build_ref(tmp_path_factory.mktemp("upsample_ref"))


@pytest.fixture(scope="module")
def renderer(gpu):
    from mirror_maze import Renderer

    r = Renderer(0)
    yield r
    r.close()


def _scene_renderer(name, view=None, defaults=False):
    """(Renderer with the scene uploaded, uniform).  MM_OPT_DEFER_MIN 0 unless `defaults`: a multi-frame variance
    launch then runs at the tests' small sizes, so trace_upsampled(var=True) traces its low view in ONE launch --
    the route a 1920x1080 batch takes.  With the default options it is refused at these sizes and trace_upsampled
    traces frame by frame: test_trace_upsampled_with_default_options covers that route and compares the two."""
    from mirror_maze import Renderer, _lib

    s, u = U.scene_view(name, view)
    r = Renderer(0)
    if not defaults:
        r.set_option(_lib.MM_OPT_DEFER_MIN, 0)
    r.upload_scene(s)
    return r, u


def _dev(a):
    import torch

    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else np.array(a)).to("cuda:0")


def _host(t):
    return None if t is None else t.cpu().numpy()


def _bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint32)


def _differ(got, ref):
    return int((_bits(got) != _bits(ref)).sum())


def _with_cam(u, cam10):
    from mirror_maze import _lib

    uf = _lib.mm_uniform.from_buffer_copy(bytes(u))
    uf.cam = _lib.mm_camera.from_buffer_copy(np.ascontiguousarray(cam10, dtype=np.float32).tobytes())
    return uf


def _cameras(u, n):
    """n cameras a few centimetres apart, from the view's."""
    cams = np.tile(np.frombuffer(bytes(u.cam), dtype=np.float32), (n, 1))
    cams[:, 0] += np.float32(0.004) * np.arange(n, dtype=np.float32)
    cams[:, 2] += np.float32(0.05) * np.arange(n, dtype=np.float32)
    return cams


@pytest.fixture(params=[1, 0], ids=["lds", "gather"])
def staging(request, renderer):
    """MM_OPT_UPSAMPLE_LDS 1 (the default) and 0 on the module's renderer: both kernels compute the same bits."""
    from mirror_maze import _lib

    renderer.set_option(_lib.MM_OPT_UPSAMPLE_LDS, request.param)
    yield request.param
    renderer.set_option(_lib.MM_OPT_UPSAMPLE_LDS, 1)


@pytest.mark.parametrize("shape", U.SHAPES)
@pytest.mark.parametrize("scale", U.SCALES)
def test_synthetic_inputs_equal_the_reference_on_all_bits(renderer, up_lib, staging, shape, scale):
    """Colour, weight and variance, zero differing bits: 1 and 3 frames (a tap
    never reads another frame), w_min 0.25 / 0.5 / 1, with and without
    low_vmean (whose values include subnormals), with and without the weight
    output, the taps gathered from memory and staged in LDS; the inputs are
    unchanged afterwards."""
    for n in U.N_FRAMES:
        low, g, vm = U.synthetic(shape, scale, n)
        tlow, tvm = _dev(low), _dev(vm)
        ta = {k: _dev(g[k]) for k in NAMES}
        for w_min in U.W_MINS:
            ref_c, ref_w, ref_v, _ = U.upsample_ref(up_lib, low, g, scale, w_min, vm)
            for use_var in (True, False):
                for want_weight in (True, False):
                    c, wt, vo = renderer.upsample(tlow, ta, scale, w_min, tvm if use_var else None, want_weight)
                    case = (shape, scale, n, w_min, use_var, want_weight)
                    assert _differ(c, ref_c) == 0, case
                    assert (wt is None) == (not want_weight) and (vo is None) == (not use_var), case
                    if want_weight:
                        assert _differ(wt, ref_w) == 0, case
                    if use_var:
                        assert _differ(vo, ref_v) == 0, case
        assert _differ(tlow, low) == 0 and _differ(tvm, vm) == 0
        assert all(_differ(ta[k], g[k]) == 0 for k in NAMES)


@pytest.mark.parametrize("name", list(U.VIEW))
@pytest.mark.parametrize("scale", U.SCENE_SCALES)
def test_scene_cases_equal_the_reference_on_all_bits(up_lib, gpu, name, scale):
    """The GPU's own low trace (8 spp, with its variance) and trace_aov of the
    whole view: the upsample equals the reference run over the downloaded
    inputs."""
    from mirror_maze import _lib, make_ext

    r, u = _scene_renderer(name)
    try:
        w, h = U.VIEW[name]
        lw, lh = U.lattice_shape(w, h, scale)
        low, lvar, _ = r.trace_tile_var(U.low_uniform(u, scale), make_ext(U.SPP, 8, U.MIRROR_LIMIT, frame=3), 0, 0, lw, lh)
        aov = r.trace_aov(u, None, U.MIRROR_LIMIT, x0=0, y0=0, w=w, h=h)
        r.sync()
        vm = np.ascontiguousarray(_host(lvar) / np.float32(U.SPP))
        g = {k: _host(aov[k]) for k in NAMES}
        g["id"] = g["id"].view(np.uint32)
        ref_c, ref_w, ref_v, cnt = U.upsample_ref(up_lib, _host(low), g, scale, 0.25, vm)
        assert np.isfinite(ref_c).all() and np.isfinite(ref_v).all()
        for lds in (1, 0):  # the lattice footprint staged in LDS (the default), and the taps gathered from memory
            r.set_option(_lib.MM_OPT_UPSAMPLE_LDS, lds)
            c, wt, vo = r.upsample(low, aov, scale, 0.25, _dev(vm))
            assert _differ(c, ref_c) == 0 and _differ(wt, ref_w) == 0 and _differ(vo, ref_v) == 0, (name, scale, lds)
        assert cnt["taken"] > 0 and cnt["from_2"] > 0
    finally:
        r.close()


@pytest.mark.parametrize("name", list(U.VIEW))
@pytest.mark.parametrize("scale", U.SCALES)
def test_low_view_is_the_full_views_lattice_on_the_gpu(gpu, name, scale):
    """The premise, for the GPU's primary_dir: trace_aov of the (view / s) view
    equals the full view's [::s, ::s] on all bits."""
    view = U.VIEW8[name] if scale == 8 else U.VIEW[name]
    r, u = _scene_renderer(name, view)
    try:
        w, h = view
        full = r.trace_aov(u, None, U.MIRROR_LIMIT, x0=0, y0=0, w=w, h=h)
        lo = r.trace_aov(U.low_uniform(u, scale), None, U.MIRROR_LIMIT, x0=0, y0=0, w=w // scale, h=h // scale)
        r.sync()
        for k in NAMES:
            assert _differ(lo[k], full[k][:, ::scale, ::scale].contiguous()) == 0, (name, scale, k)
    finally:
        r.close()


@pytest.mark.parametrize("var", [False, True])
def test_trace_upsampled_fills_its_holes_with_the_full_views_pixels(gpu, var):
    """Corridor 140 x 48, s = 2, two cameras, 8 spp from RNG frame 5: every hole
    pixel equals that pixel of trace_tile on the full view with the frame's
    camera and RNG frame, every lattice pixel the low trace, both with weight
    1; the weight is positive everywhere; with var the holes' variance is
    trace_pixels_var's / spp; the result runs through accumulate_var and
    denoise_var."""
    import torch

    from mirror_maze import make_ext

    name, scale = "corridor", 2
    r, u = _scene_renderer(name)
    try:
        w, h = U.VIEW[name]
        lw, lh = U.lattice_shape(w, h, scale)
        cams = _cameras(u, 2)
        ext = make_ext(U.SPP, 8, U.MIRROR_LIMIT, frame=5)
        _, _, w0, _, share0 = r.trace_upsampled(u, cams, ext, scale, 0, 0, w, h, var=var, fill=False)
        color, aov, weight, vout, share = r.trace_upsampled(u, cams, ext, scale, 0, 0, w, h, var=var)
        low, _ = r.trace_tile_cameras(U.low_uniform(u, scale), cams, ext, 0, 0, lw, lh)
        r.sync()
        assert share == share0 and (vout is not None) == var
        holes = _host(w0) == 0
        ids = _host(aov["id"]).view(np.uint32)
        assert not (ids == U.FAILED).any()
        assert _differ(color[:, ::scale, ::scale].contiguous(), low) == 0
        wt = _host(weight)
        assert (wt[:, ::scale, ::scale] == 1.0).all() and (wt[holes] == 1.0).all() and (wt > 0).all()
        assert np.array_equal(wt[~holes], _host(w0)[~holes])
        for f in range(2):
            assert holes[f].any() and abs(share[f] - holes[f].mean()) < 1e-9, share
            uf, ef = _with_cam(u, cams[f]), make_ext(U.SPP, 8, U.MIRROR_LIMIT, frame=5 + f)
            full, _ = r.trace_tile(uf, ef, 0, 0, w, h)
            r.sync()
            assert _differ(_host(color[f])[holes[f]], _host(full)[holes[f]]) == 0, f
            if var:
                _, pv, _ = r.trace_pixels_var(uf, ef, U.holes_of(_host(w0[f])))
                assert _differ(_host(vout[f])[holes[f]], _host(pv / float(U.SPP))) == 0, f
        if var:
            acc, avar = r.accumulate_var(u, cams, color, aov, vout, weight)
            dn = r.denoise_var(acc, aov, avar, 1.0)
            r.sync()
            assert torch.isfinite(acc).all() and torch.isfinite(avar).all() and torch.isfinite(dn).all()
            assert float(acc[1][..., 3].max()) > 1.0
    finally:
        r.close()


def test_fill_pixels_replaces_exactly_the_listed_pixels(renderer, up_lib):
    """Bit-exact replace of colour, variance and weight; entries outside the
    window touch nothing; the optional images may be left out; an empty list
    does nothing; the list's buffers are unchanged."""
    rng = np.random.default_rng(11)
    w, h, x0, y0 = 37, 9, 10, 20
    img = rng.uniform(0, 1, size=(h, w, 4)).astype(np.float32)
    var, wt = rng.uniform(0, 1, size=(2, h, w)).astype(np.float32)
    inside = rng.permutation(w * h)[:300]
    px = np.stack([x0 + inside % w, y0 + inside // w], axis=1).astype(np.uint32)
    px = np.concatenate([px, np.uint32([[x0 - 1, y0], [x0 + w, y0], [x0, y0 - 1], [x0, y0 + h], [0, 0], [0xFFFFFFFF, y0]])])
    px = np.ascontiguousarray(px[rng.permutation(len(px))])
    ex = rng.uniform(2, 3, size=(len(px), 4)).astype(np.float32)
    ex[::7] = np.float32([1e-40, -0.0, np.inf, 3e38])  # copied, not computed: every bit pattern survives
    ev = rng.uniform(2, 3, size=len(px)).astype(np.float32)
    ev[::5] = np.float32(1e-44)
    tpx, tex, tev = _dev(px), _dev(ex), _dev(ev)
    for use_var in (True, False):
        for use_weight in (True, False):
            ti, tv, tw = _dev(img), _dev(var), _dev(wt)
            ref_i, ref_v, ref_w, n_in = U.fill_ref(up_lib, img, var if use_var else None, wt if use_weight else None, x0,
                                                   y0, px, ex, ev if use_var else None, 0.75)
            assert n_in == 300
            got = renderer.fill_pixels(ti, tpx, tex, 0.75, tv if use_var else None, tev if use_var else None,
                                       tw if use_weight else None, x0, y0)
            assert got is ti and _differ(ti, ref_i) == 0
            assert _differ(tv, ref_v if use_var else var) == 0 and _differ(tw, ref_w if use_weight else wt) == 0
    assert _differ(tpx, px) == 0 and _differ(tex, ex) == 0 and _differ(tev, ev) == 0
    ti = _dev(img)
    renderer.fill_pixels(ti, np.zeros((0, 2), np.uint32), _dev(np.zeros((0, 4), np.float32)), 1.0, x0=x0, y0=y0)
    assert _differ(ti, img) == 0
    with pytest.raises(ValueError):
        renderer.fill_pixels(ti, tpx, tex, 1.0, var=_dev(var))


@pytest.mark.parametrize("var", [False, True])
@pytest.mark.parametrize("n", [1, 2])
def test_trace_upsampled_with_default_options(gpu, n, var):
    """A Renderer as a user gets it (no option set), the corridor's window (8, 4, 67, 37) at s = 2, one and two
    cameras: with `var` the low view is far below the paths a multi-frame variance launch needs, so it is traced
    frame by frame; the result equals the one-launch route's (MM_OPT_DEFER_MIN 0) on all bits, and every hole
    equals that pixel of trace_tile on the full view."""
    from mirror_maze import make_ext

    scale, (x0, y0, w, h) = 2, (8, 4, 67, 37)
    ext = make_ext(U.SPP, 8, U.MIRROR_LIMIT, frame=9)
    got = {}
    for defaults in (True, False):
        r, u = _scene_renderer("corridor", defaults=defaults)
        try:
            cams = _cameras(u, n)
            color, aov, weight, vout, share = r.trace_upsampled(u, cams, ext, scale, x0, y0, w, h, var=var)
            _, _, w0, _, _ = r.trace_upsampled(u, cams, ext, scale, x0, y0, w, h, var=var, fill=False)
            r.sync()
            got[defaults] = (color, weight, vout, share)
            if defaults:
                holes = _host(w0) == 0
                assert tuple(color.shape) == (n, h, w, 4) and (vout is not None) == var
                for f in range(n):
                    assert holes[f].any()
                    ef = make_ext(U.SPP, 8, U.MIRROR_LIMIT, frame=9 + f)
                    full, _ = r.trace_tile(_with_cam(u, cams[f]), ef, x0, y0, w, h)
                    r.sync()
                    assert _differ(_host(color[f])[holes[f]], _host(full)[holes[f]]) == 0, f
                    assert (_host(weight[f])[holes[f]] == 1.0).all() and (_host(weight[f]) > 0).all()
        finally:
            r.close()
    a, b = got[True], got[False]
    assert _differ(a[0], b[0]) == 0 and _differ(a[1], b[1]) == 0 and a[3] == b[3]
    if var:
        assert _differ(a[2], b[2]) == 0


def test_flythrough_upsample_renders_with_default_options(gpu, tmp_path, capsys):
    """scripts/flythrough.py --upsample 2 --accumulate-var --denoise-var --denoise, rendered: three 64x48 frames
    in batches of two, every file written."""
    import importlib.util
    import sys
    from pathlib import Path

    repo = Path(__file__).resolve().parent.parent
    path0 = list(sys.path)
    try:
        spec = importlib.util.spec_from_file_location("flythrough_up_gpu", repo / "scripts" / "flythrough.py")
        fly = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(fly)
        rc = fly.main(["--maze", "4", "--frames", "3", "--batch", "2", "--width", "64", "--height", "48", "--out",
                       str(tmp_path), "--upsample", "2", "--accumulate-var", "--denoise-var", "--denoise"])
    finally:
        sys.path[:] = path0
    assert rc == 0
    out = capsys.readouterr().out
    assert out.count("upsampled x2, holes") == 3
    for f in range(3):
        for tag in ("up", "accv", "dnv", "dn"):
            assert (tmp_path / f"frame_{f:04d}_{tag}.png").stat().st_size > 0
        assert not (tmp_path / f"frame_{f:04d}.png").exists()
