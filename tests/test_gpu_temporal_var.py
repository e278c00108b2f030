"""mm_accumulate_frames_var and mm_blend_pixels_var on the GPU against
tests/temporal_var_ref.c on the same inputs: every comparison is on bits, zero
differing elements, nothing excluded -- both calls are specified operation by
operation (include/mm_api.h).  The input conditions (what the sequences,
variances and weights make every clause decide, and that every compared output
is finite) are tests/test_temporal_var.py's."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import denoise_support as D
import denoise_var_support as DV
import temporal_support as T
import temporal_var_support as TV
import topup_support as TU

pytestmark = pytest.mark.gpu

NAMES = T.NAMES
SCENES = tuple(n for n in T.SEQUENCES if n != "synthetic")
_CACHE = {}


@pytest.fixture(scope="module")
def tv_lib(tmp_path_factory):
    return TV.build_ref(tmp_path_factory.mktemp("temporal_var_ref"))


@pytest.fixture(scope="module")
def dnv_lib(tmp_path_factory):
    return DV.build_ref(tmp_path_factory.mktemp("denoise_var_ref"))


@pytest.fixture(scope="module")
def renderer(gpu):
    from mirror_maze import Renderer

    r = Renderer(0)
    yield r
    r.close()


def _inputs(name, shape):
    """dict of one case: the view's uniform, (x0, y0), cams, and the frames,
    guides, variances of the mean and weights as CUDA tensors (tc, ta, tv, tw)
    and as numpy arrays (color, g, vm, wt).  The scene sequences are traced on
    the GPU with their variance (8 spp, one launch for the four cameras) and
    vmean = var / 8 is formed in numpy float32 and uploaded, so both sides
    see the same bits; built once, read-only."""
    import torch

    key = (name, shape)
    if key in _CACHE:
        return _CACHE[key]
    from mirror_maze import Renderer, _lib, make_ext

    w, h = shape
    dev = torch.device("cuda:0")
    if name == "synthetic":
        cams, color, g = T.synthetic(shape)
        view, (x0, y0) = T.synthetic_view(shape), T.SYN_ORIGIN
        u = _lib.mm_uniform()
        u.view_w, u.view_h = view
        tc = torch.from_numpy(color).to(dev)
        ta = {k: torch.from_numpy(g[k].view(np.int32) if k == "id" else g[k]).to(dev) for k in NAMES}
        vm = TV.synthetic_vmean(shape)
    else:
        s, u = T.scene_view(name)
        view = T.VIEW[name]
        cams = T.scene_cameras(name)
        x0, y0 = T.ORIGIN[name][shape]
        with Renderer(0) as r:
            r.set_option(_lib.MM_OPT_DEFER_MIN, 0)  # a multi-frame variance launch of any size
            r.upload_scene(s)
            tc, var, _ = r.trace_tile_var(u, make_ext(TV.SPP, 8, T.MIRROR_LIMIT, frame=3), x0, y0, w, h, 1, cameras=cams)
            ta = r.trace_aov(u, cams, T.MIRROR_LIMIT, x0=x0, y0=y0, w=w, h=h, y_stride=1)
            r.sync()
        color = tc.cpu().numpy()
        g = {k: ta[k].cpu().numpy() for k in NAMES}
        g["id"] = g["id"].view(np.uint32)
        vm = TV.vmean_of(var.cpu().numpy())
    wt = TV.weights(shape)
    assert np.isfinite(vm).all() and (vm >= 0).all()
    for a in (cams, color, vm, wt, *g.values()):
        a.setflags(write=False)
    _CACHE[key] = dict(u=u, view=(float(view[0]), float(view[1])), x0=x0, y0=y0, cams=cams, tc=tc, ta=ta,
                       tv=torch.from_numpy(np.array(vm)).to(dev), tw=torch.from_numpy(np.array(wt)).to(dev),
                       color=color, g=g, vm=vm, wt=wt)
    return _CACHE[key]


def _ref(tv_lib, name, shape, lo, hi, with_prev, n_max, weighted, tol_z=0.02, w_min=0.25):
    """(colour, variance) of the reference for frames lo..hi-1, computed once
    and shared (read-only).  with_prev: the history starts from frame 1 of the
    two-frame reference run without prev, its guides, camera and variance."""
    key = ("ref", name, shape, lo, hi, with_prev, n_max, weighted, tol_z, w_min)
    if key not in _CACHE:
        c = _inputs(name, shape)
        prev = _prev_np(tv_lib, name, shape, n_max, weighted, tol_z, w_min) if with_prev else None
        out, vout, _ = TV.accumulate_ref(tv_lib, c["view"], c["cams"][lo:hi], c["color"][lo:hi],
                                         {k: c["g"][k][lo:hi] for k in NAMES}, c["vm"][lo:hi],
                                         c["wt"][lo:hi] if weighted else None, prev=prev, n_max=n_max, tol_z=tol_z,
                                         w_min=w_min, x0=c["x0"], y0=c["y0"])
        assert np.isfinite(out).all() and np.isfinite(vout).all()
        out.setflags(write=False)
        vout.setflags(write=False)
        _CACHE[key] = (out, vout)
    return _CACHE[key]


def _prev_np(tv_lib, name, shape, n_max, weighted, tol_z=0.02, w_min=0.25):
    c = _inputs(name, shape)
    two, tvar = _ref(tv_lib, name, shape, 0, 2, False, n_max, weighted, tol_z, w_min)
    return two[1], {k: c["g"][k][1:2] for k in NAMES}, c["cams"][1], tvar[1]


def _prev_gpu(tv_lib, name, shape, n_max, weighted, tol_z=0.02, w_min=0.25):
    """The same prev as CUDA tensors (colour and variance uploaded from the reference)."""
    import torch

    c = _inputs(name, shape)
    pc, _, pcam, pvar = _prev_np(tv_lib, name, shape, n_max, weighted, tol_z, w_min)
    dev = c["tc"].device
    return (torch.from_numpy(np.array(pc)).to(dev), {k: c["ta"][k][1:2] for k in NAMES}, pcam,
            torch.from_numpy(np.array(pvar)).to(dev))


def _run(r, c, lo, hi, weighted=False, prev=None, **kw):
    return r.accumulate_var(c["u"], c["cams"][lo:hi], c["tc"][lo:hi], {k: c["ta"][k][lo:hi] for k in NAMES},
                            c["tv"][lo:hi], c["tw"][lo:hi] if weighted else None, prev=prev, x0=c["x0"], y0=c["y0"], **kw)


def _bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint32)


def _same(got, ref):
    """Zero differing bits in the colour and in the variance."""
    return int((_bits(got[0]) != _bits(ref[0])).sum()) + int((_bits(got[1]) != _bits(ref[1])).sum()) == 0


def _unchanged(name, shape):
    c = _inputs(name, shape)
    return (np.array_equal(_bits(c["tc"]), _bits(c["color"])) and np.array_equal(_bits(c["tv"]), _bits(c["vm"]))
            and np.array_equal(_bits(c["tw"]), _bits(c["wt"]))
            and all(np.array_equal(_bits(c["ta"][k]), _bits(c["g"][k])) for k in NAMES))


@pytest.mark.parametrize("shape", D.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", T.SEQUENCES)
def test_frames_prev_caps_and_weights_bit_exact(renderer, tv_lib, name, shape):
    """n_frames 1, 2 and 4, with and without prev, n_max 1, 4 and 65535,
    weights None and per pixel: zero differing bits against the reference in
    the colour and in the variance, every pixel of every frame; with weights
    None the colour is Renderer.accumulate's bit for bit; the inputs are as
    they were."""
    c = _inputs(name, shape)
    for weighted in (False, True):
        for n_max in T.N_MAX:
            for n in (1, 2, T.N_FRAMES):
                for with_prev in (False, True):
                    prev = _prev_gpu(tv_lib, name, shape, n_max, weighted) if with_prev else None
                    got = _run(renderer, c, 0, n, weighted, prev=prev, n_max=n_max)
                    ref = _ref(tv_lib, name, shape, 0, n, with_prev, n_max, weighted)
                    assert got[0].shape == c["tc"][:n].shape and got[1].shape == c["tv"][:n].shape
                    assert _same(got, ref), (name, shape, weighted, n_max, n, with_prev)
                    if not weighted:
                        plain = renderer.accumulate(c["u"], c["cams"][:n], c["tc"][:n], {k: c["ta"][k][:n] for k in NAMES},
                                                    prev=None if prev is None else prev[:3], n_max=n_max,
                                                    x0=c["x0"], y0=c["y0"])
                        assert np.array_equal(_bits(got[0]), _bits(plain)), (name, shape, n_max, n, with_prev)
    assert _unchanged(name, shape)


@pytest.mark.parametrize("tol_z,w_min", [(0.002, 0.25), (0.3, 1.0), (0.02, 0.9), (1e-6, 1e-6)])
@pytest.mark.parametrize("name", T.SEQUENCES)
def test_tolerances_bit_exact(renderer, tv_lib, name, tol_z, w_min):
    """test_gpu_temporal.py's tolerance pairs, on colour and variance, with
    per-pixel weights."""
    for shape in ((67, 5), (130, 9), (3, 40)):
        c = _inputs(name, shape)
        got = _run(renderer, c, 0, T.N_FRAMES, True, prev=_prev_gpu(tv_lib, name, shape, 32, True, tol_z, w_min),
                   n_max=32, tol_z=tol_z, w_min=w_min)
        assert _same(got, _ref(tv_lib, name, shape, 0, T.N_FRAMES, True, 32, True, tol_z, w_min)), (name, shape, tol_z, w_min)
    if name == "corridor":  # the parameters matter on these inputs
        a = _ref(tv_lib, name, (130, 9), 0, T.N_FRAMES, True, 32, True, 0.002, 0.25)
        b = _ref(tv_lib, name, (130, 9), 0, T.N_FRAMES, True, 32, True, 0.3, 1.0)
        assert not np.array_equal(a[0], b[0])


@pytest.mark.parametrize("name", T.SEQUENCES)
def test_chaining_on_the_gpu(renderer, tv_lib, name):
    """Frames 0..3 in one call equal frames 0..1, then frames 2..3 with prev
    taken from frame 1 of the first call's out and var_out, bit for bit; a
    single-frame tensor is one frame; `out` and `var_out` are written in
    place."""
    import torch

    for shape in ((130, 9), (67, 5)):
        c = _inputs(name, shape)
        for weighted in (False, True):
            whole = _run(renderer, c, 0, T.N_FRAMES, weighted, n_max=3)
            head = _run(renderer, c, 0, 2, weighted, n_max=3)
            into, vinto = torch.zeros_like(c["tc"][2:]), torch.zeros_like(c["tv"][2:])
            tail = _run(renderer, c, 2, T.N_FRAMES, weighted,
                        prev=(head[0][1], {k: c["ta"][k][1] for k in NAMES}, c["cams"][1], head[1][1]), n_max=3,
                        out=into, var_out=vinto)
            assert tail[0] is into and tail[1] is vinto
            assert np.array_equal(_bits(whole[0]), _bits(torch.cat([head[0], tail[0]])))
            assert np.array_equal(_bits(whole[1]), _bits(torch.cat([head[1], tail[1]])))
            assert _same(whole, _ref(tv_lib, name, shape, 0, T.N_FRAMES, False, 3, weighted))
        one = renderer.accumulate_var(c["u"], c["cams"][:1], c["tc"][0], {k: c["ta"][k][0] for k in NAMES}, c["tv"][0],
                                      c["tw"][0], x0=c["x0"], y0=c["y0"])
        assert one[0].shape == c["tc"][0].shape and one[1].shape == c["tv"][0].shape
        assert np.array_equal(_bits(one[0])[..., :3], _bits(c["color"][0])[..., :3])
        assert np.array_equal(_bits(one[0])[..., 3], _bits(c["wt"][0])) and np.array_equal(_bits(one[1]), _bits(c["vm"][0]))
    assert _unchanged(name, (130, 9)) and _unchanged(name, (67, 5))


def test_back_to_back_calls_of_different_sizes(gpu, tv_lib):
    """A small call, a larger one, the small one again, back to back on a fresh
    context with no sync in between: the first and the third result are equal,
    all three equal the reference, and the inputs are as they were."""
    from mirror_maze import Renderer

    small, large = ("synthetic", (67, 5)), ("corridor", (130, 9))
    cs, cl = _inputs(*small), _inputs(*large)
    with Renderer(0) as r:
        one = _run(r, cs, 0, 2, True, n_max=4)
        two = _run(r, cl, 0, T.N_FRAMES, False, n_max=4)
        three = _run(r, cs, 0, 2, True, n_max=4)
        r.sync()
        assert _same(one, three)
        assert _same(one, _ref(tv_lib, *small, 0, 2, False, 4, True))
        assert _same(two, _ref(tv_lib, *large, 0, T.N_FRAMES, False, 4, False))
    assert _unchanged(*small) and _unchanged(*large)


@pytest.mark.parametrize("m", TU.WEIGHTS)
def test_blend_pixels_var_bit_exact(renderer, tv_lib, m):
    """topup_support.blend_inputs and a variance image: colour and variance
    equal the reference on all bits, the colour equals blend_pixels', and the
    entries outside the window touch nothing (the reference skips them)."""
    import torch

    image, px, extra = TU.blend_inputs()
    x0, y0, w, h = TU.WINDOW
    rng = np.random.default_rng(3)
    var = rng.uniform(0, 1, size=(h, w)).astype(np.float32)
    var[0, :6] = (0.0, 1e-40, 1e30, 0.0, 1e-40, 1e30)
    ev = rng.uniform(0, 1, size=len(px)).astype(np.float32)
    ev[::7] = np.float32(1e-40)
    dev = torch.device("cuda:0")
    t_img, t_var = torch.from_numpy(image).to(dev), torch.from_numpy(var).to(dev)
    t_px = torch.from_numpy(px.view(np.int32)).to(dev)
    t_ex, t_ev = torch.from_numpy(extra).to(dev), torch.from_numpy(ev).to(dev)
    plain = renderer.blend_pixels(t_img.clone(), t_px, t_ex, m, x0, y0)
    got, gvar = renderer.blend_pixels_var(t_img, t_var, t_px, t_ex, t_ev, m, x0, y0)
    assert got is t_img and gvar is t_var
    ref, rvar, n = TV.blend_ref(tv_lib, image, var, x0, y0, px, extra, ev, m)
    assert n == 120 and np.isfinite(rvar).all()
    assert np.array_equal(_bits(got), _bits(ref)) and np.array_equal(_bits(gvar), _bits(rvar))
    assert np.array_equal(_bits(got), _bits(plain))
    assert int((_bits(rvar) != _bits(var)).sum()) <= 120 and int((_bits(gvar) != _bits(var)).sum()) > 60
    assert np.array_equal(_bits(t_px), _bits(px)) and np.array_equal(_bits(t_ex), _bits(extra))
    assert np.array_equal(_bits(t_ev), _bits(ev))
    # an empty list is MM_OK and touches nothing
    renderer.blend_pixels_var(t_img, t_var, np.zeros((0, 2), np.uint32), t_ex[:0], t_ev[:0], m, x0, y0)
    assert np.array_equal(_bits(t_img), _bits(ref)) and np.array_equal(_bits(t_var), _bits(rvar))


@pytest.mark.parametrize("name", SCENES)
def test_trace_accumulate_denoise_is_the_references_composed(renderer, tv_lib, dnv_lib, name):
    """trace_tile_var(cameras) -> accumulate_var -> denoise_var(acc, aov, Vout,
    1.0, return_var=True) equals temporal_var_ref.c followed by
    denoise_var_ref.c, on bits, colour and variance, at (130, 9)."""
    shape = (130, 9)
    c = _inputs(name, shape)  # trace_tile_var(cameras=...) made tc and tv's variance
    acc, vout = _run(renderer, c, 0, T.N_FRAMES)
    got, gvar = renderer.denoise_var(acc, c["ta"], vout, 1.0, return_var=True)
    ref_acc, ref_vout = _ref(tv_lib, name, shape, 0, T.N_FRAMES, False, 32, False)
    assert _same((acc, vout), (ref_acc, ref_vout))
    ref, rvar, _ = DV.filter_ref(dnv_lib, ref_acc, c["g"], ref_vout, n_passes=4, sigma_z=0.02, sigma_l=8.0, eps_l=1e-2)
    assert np.isfinite(ref).all() and np.isfinite(rvar).all()
    assert np.array_equal(_bits(got), _bits(ref)) and np.array_equal(_bits(gvar), _bits(rvar))
    assert _unchanged(name, shape)


@pytest.mark.parametrize("n_min,rel_tol", [(3.0, None), (None, 0.2), (3.0, 0.2)])
def test_top_up_var_is_select_trace_blend(gpu, tv_lib, n_min, rel_tol):
    """top_up_var on the jump sequence's last accumulated frame (history
    lengths 2 and 4 side by side: the jump cut part of the window's history;
    on the CPU reference N is 2 at 72 pixels, 4 at 792, and 619 pixels are
    above rel_tol 0.2):
    the selection is the union of
    select_short_history and select_noisy computed on CPU copies, row-major,
    each pixel once, and acc and var afterwards equal the reference blend of
    trace_pixels_var's result with extra_vmean = var / extra_spp, on bits."""
    import torch

    from mirror_maze import Renderer, make_ext, select_noisy, select_short_history

    name, shape, extra_spp, key = "maze4_jump", (130, 9), 6, (1 << 21) + 3
    c = _inputs(name, shape)
    s, u = T.scene_view(name)
    e = make_ext(TV.SPP, 8, T.MIRROR_LIMIT, frame=3)
    with Renderer(0) as r:
        r.upload_scene(s)
        acc, vout = _run(r, c, 0, T.N_FRAMES)
        a0, v0 = acc[-1].cpu(), vout[-1].cpu()
        ids = c["ta"]["id"][-1].cpu()
        want = set()
        if n_min is not None:
            want |= {tuple(p) for p in select_short_history(a0, ids, n_min, c["x0"], c["y0"]).tolist()}
        if rel_tol is not None:
            want |= {tuple(p) for p in select_noisy(a0, v0, 1.0, rel_tol, ids=ids, x0=c["x0"], y0=c["y0"]).tolist()}
        px = np.array(sorted(want, key=lambda p: (p[1], p[0])), dtype=np.uint32).reshape(-1, 2)
        assert 0 < len(px) < shape[0] * shape[1]
        a1, v1 = acc[-1].clone(), vout[-1].clone()
        got_a, got_v, n = r.top_up_var(c["u"], c["cams"][-1], e, a1, v1, {"id": c["ta"]["id"][-1]}, extra_spp, key,
                                       n_min=n_min, rel_tol=rel_tol, x0=c["x0"], y0=c["y0"])
        assert got_a is a1 and got_v is v1 and n == len(px)
        uk = type(c["u"]).from_buffer_copy(bytes(c["u"]))
        C.memmove(C.byref(uk), np.ascontiguousarray(c["cams"][-1], dtype=np.float32).ctypes.data, 40)
        extra, var_b, _ = r.trace_pixels_var(uk, make_ext(extra_spp, 8, T.MIRROR_LIMIT, frame=key), px)
        ev = (var_b / float(extra_spp)).cpu().numpy()
        ref_a, ref_v, inside = TV.blend_ref(tv_lib, a0.numpy(), v0.numpy(), c["x0"], c["y0"], px, extra.cpu().numpy(), ev,
                                            extra_spp / TV.SPP)
        assert inside == len(px)
        assert np.array_equal(_bits(got_a), _bits(ref_a)) and np.array_equal(_bits(got_v), _bits(ref_v))
        changed = (_bits(got_a) != _bits(a0.numpy())).any(axis=-1)
        assert int(changed.sum()) == len(px)  # alpha grew at every selected pixel, and at no other
    assert _unchanged(name, shape)


def test_errors_with_a_context(renderer, tv_lib):
    """Overlapping outputs and misaligned pointers return MM_ERR_INVALID from a
    real context, which accepts the call that is in order, and name the call;
    Renderer.accumulate_var raises on mismatched shapes before calling the
    library."""
    import torch

    from mirror_maze import _lib

    L, inv, ctx = _lib.lib(), _lib.MM_ERR_INVALID, renderer._ctx
    c = _inputs("synthetic", (67, 5))
    tc, ta, tv, tw = c["tc"], c["ta"], c["tv"], c["tw"]
    n, h, w = tc.shape[:3]
    out, vout = torch.empty_like(tc), torch.empty_like(tv)
    cams = np.ascontiguousarray(c["cams"])
    a = _lib.mm_aov(*[ta[k].data_ptr() for k in NAMES])
    ok = _lib.mm_temporal_params(32, 0.02, 0.25, 0)

    def call(color=tc.data_ptr(), aov=a, vm=tv.data_ptr(), wt=None, prev=None, p=ok, n=n, o=out.data_ptr(),
             vo=vout.data_ptr()):
        return L.mm_accumulate_frames_var(ctx, C.byref(c["u"]), cams.ctypes.data, color, C.byref(aov), vm, wt,
                                          None if prev is None else C.byref(prev), C.byref(p), n, c["x0"], c["y0"], w, h,
                                          o, vo)

    assert call() == _lib.MM_OK and call(wt=tw.data_ptr()) == _lib.MM_OK
    # overlaps: var_out on vmean, var_out on the weights, var_out on out, out on an input
    assert call(vo=tv.data_ptr()) == inv and call(wt=tw.data_ptr(), vo=tw.data_ptr()) == inv
    assert call(vo=out.data_ptr()) == inv and call(vo=out.data_ptr() + 16 * n * w * h - 4) == inv
    assert call(o=tc.data_ptr()) == inv and call(o=ta["albedo"].data_ptr()) == inv
    assert b"mm_accumulate_frames_var" in L.mm_last_error(ctx)
    # misaligned pointers
    assert call(n=1, vm=tv.data_ptr() + 2) == inv and call(n=1, vo=vout.data_ptr() + 1) == inv
    assert call(n=1, wt=tw.data_ptr() + 3) == inv and call(n=1, o=out.data_ptr() + 8) == inv
    # prev: an earlier call's outputs are fine, this call's are not, a null variance is not
    first = renderer.accumulate_var(c["u"], cams[:1], tc[:1], {k: ta[k][:1] for k in NAMES}, tv[:1], x0=c["x0"], y0=c["y0"])
    pa = _lib.mm_aov(*[ta[k].data_ptr() for k in NAMES])
    cam0 = _lib.mm_camera.from_buffer_copy(cams[0].tobytes())
    rest = dict(n=1, color=tc[1:].data_ptr(), aov=_lib.mm_aov(*[ta[k][1:].data_ptr() for k in NAMES]), vm=tv[1:].data_ptr())
    assert call(prev=_lib.mm_temporal_prev_var(first[0].data_ptr(), pa, cam0, first[1].data_ptr()), **rest) == _lib.MM_OK
    assert call(prev=_lib.mm_temporal_prev_var(first[0].data_ptr(), pa, cam0, vout.data_ptr()), **rest) == inv
    assert call(prev=_lib.mm_temporal_prev_var(first[0].data_ptr(), pa, cam0, out.data_ptr()), **rest) == inv
    assert call(prev=_lib.mm_temporal_prev_var(first[0].data_ptr(), pa, cam0, None), **rest) == inv
    assert call(prev=_lib.mm_temporal_prev_var(first[0].data_ptr(), pa, cam0, first[1].data_ptr() + 2), **rest) == inv
    assert b"mm_accumulate_frames_var" in L.mm_last_error(ctx)
    # mm_blend_pixels_var with the context
    px = torch.tensor([[0, 0], [1, 0], [2, 0], [3, 0]], dtype=torch.int32, device=tc.device)  # each pixel once
    ex, ev = torch.zeros((4, 4), device=tc.device), torch.zeros((4,), device=tc.device)
    img, var = out[0], vout[0]

    def blend(i=img.data_ptr(), v=var.data_ptr(), e=ex.data_ptr(), s=ev.data_ptr(), m=1.0):
        return L.mm_blend_pixels_var(ctx, i, v, 0, 0, w, h, px.data_ptr(), e, s, 4, m)

    assert blend() == _lib.MM_OK
    assert blend(v=img.data_ptr()) == inv and blend(s=var.data_ptr()) == inv and blend(s=img.data_ptr()) == inv
    assert blend(v=var.data_ptr() + 2) == inv and blend(s=ev.data_ptr() + 1) == inv and blend(m=0.0) == inv
    assert b"mm_blend_pixels_var" in L.mm_last_error(ctx)
    renderer.sync()
    assert _unchanged("synthetic", (67, 5))
    with pytest.raises(ValueError):
        renderer.accumulate_var(c["u"], cams[:2], tc, ta, tv)                                  # camera count
    with pytest.raises(ValueError):
        renderer.accumulate_var(c["u"], cams, tc, ta, tv[:1])                                  # vmean's frames
    with pytest.raises(ValueError):
        renderer.accumulate_var(c["u"], cams, tc, ta, tv, tw[:, :, :-1].contiguous())          # weight's shape
    with pytest.raises(ValueError):
        renderer.accumulate_var(c["u"], cams, tc, ta, tv.double())                             # dtype
    with pytest.raises(ValueError):
        renderer.accumulate_var(c["u"], cams, tc, ta, tv, prev=(tc[0], ta, cams[0], tv[0, :-1].contiguous()))
    with pytest.raises(ValueError):
        renderer.accumulate_var(c["u"], cams, tc, ta, tv, var_out=torch.empty((n, h, w, 1), device=tc.device))
    with pytest.raises(ValueError):
        renderer.blend_pixels_var(img, var[:-1].contiguous(), px, ex, ev, 1.0)
    with pytest.raises(ValueError):
        renderer.top_up_var(c["u"], cams[0], None, img, var, ta["id"][0], 8, 1 << 21)           # neither n_min nor rel_tol
