"""The Python binding on the GPU: every tensor check's ValueError text and which of two wrong arguments is
reported, the calls following torch's current stream or the pinned one, and what empty inputs give.  Numeric
results are pinned elsewhere (test_gpu_frames, test_gpu_trace_pixels, test_gpu_variance, ...); nothing here
compares pixels.  The texts are the binding's as it stood before its repeated steps were folded, and the whole
file was run against that binding first: nothing differed."""
from __future__ import annotations

import ctypes as C
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

VIEW = (64, 32)
W, H = 16, 8  # the window
N = 5  # entries of a pixel list
PIXELS_TEXT = "pixels must be a contiguous int32 / uint32 (n, 2) CUDA tensor or an (n, 2) array"
COLOR_TEXT = "color must be a contiguous float32 CUDA tensor (h, w, 4) or (n, h, w, 4)"
IMAGE_TEXT = "image must be a contiguous float32 (h, w, 4) CUDA tensor"
CAMERA_TEXT = "cameras must be mm_camera / mm_uniform values or an (n, 10) float32 array"
FILTER_OUT_TEXT = "out must be a contiguous float32 (uint8 for RGBA8) CUDA tensor of color's shape"
ACC_OUT_TEXT = "out must be a contiguous float32 CUDA tensor of color's shape"
AOV_SHAPES = {"normal_depth": ((1, H, W, 4), "torch.float32"), "albedo": ((1, H, W, 4), "torch.float32"),
              "id": ((1, H, W), "torch.int32")}


def _out_text(n):
    return f"out must be a contiguous float32 or uint8 CUDA tensor of {n} elements"


class _State:
    pass


@pytest.fixture(scope="module")
def S(gpu):
    """A renderer over the N = 4 maze and one valid set of every method's arguments for a 16 x 8 window."""
    import torch

    from mirror_maze import Renderer, Scene, default_uniform, make_ext

    s = _State()
    s.dev = gpu
    s.r = Renderer(0)
    s.r.upload_scene(Scene.build(4, 0))
    s.u = default_uniform(*VIEW, 0)
    s.e = make_ext(2, 2, 2, frame=0)
    s.color, s.var, _ = s.r.trace_tile_var(s.u, s.e, 0, 0, W, H)
    s.aov = s.r.trace_aov(s.u, x0=0, y0=0, w=W, h=H)
    s.vmean = (s.var / 2.0).contiguous()
    s.acc, s.acc_var = s.r.accumulate_var(s.u, [s.u], s.color, s.aov, s.vmean)
    s.px = torch.tensor([[0, 0], [3, 1], [15, 7], [7, 2], [8, 5]], dtype=torch.int32, device=gpu)
    s.extra, s.extra_var, _ = s.r.trace_pixels_var(s.u, s.e, s.px)
    s.rays = torch.zeros((N, 2, 4), dtype=torch.float32, device=gpu)
    s.rays[:, 1, 0] = 1.0
    s.r.sync()
    torch.cuda.synchronize()
    yield s
    s.r.close()


def _wrong(t, kinds):
    """Wrong versions of the valid tensor `t`: another dtype, a doubled last axis, a strided view of t's shape, a
    CPU copy, and uint8 where float32 is due."""
    import torch

    wide = torch.cat([t, t], dim=-1)
    other = {torch.float32: torch.float64, torch.int32: torch.int64, torch.uint8: torch.float32}[t.dtype]
    every = {"dtype": t.to(other), "shape": wide, "strided": wide[..., ::2], "cpu": t.cpu(), "uint8": t.to(torch.uint8)}
    assert every["strided"].shape == t.shape and not every["strided"].is_contiguous()
    return {k: every[k] for k in kinds}


ALL = ("dtype", "shape", "strided", "cpu")


def _cases(s):
    """(label, call taking the argument under test, its valid value, text or {kind: text}, kinds of wrong)."""
    import torch

    r, u, e, dev = s.r, s.u, s.e, s.dev
    f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)  # noqa: E731
    rgba8 = torch.zeros((H, W, 4), dtype=torch.uint8, device=dev)
    hits = torch.zeros((N, 2), dtype=torch.int32, device=dev)
    plane = lambda what, shape: f"{what} must be a contiguous float32 tensor of shape {shape} on {dev}"  # noqa: E731
    entries = lambda what, shape: f"{what} must be a contiguous float32 {shape} tensor on {dev}"  # noqa: E731
    cases = [
        ("quantize rgba", lambda x: r.quantize(x), s.color, "rgba must be a contiguous float32 CUDA tensor [..., 4]", ALL),
        ("quantize out", lambda x: r.quantize(s.color, out=x), rgba8,
         "out must be a contiguous uint8 CUDA tensor of rgba's shape", ALL),
        ("trace_tile out", lambda x: r.trace_tile(u, e, 0, 0, W, H, out=x), f32(H, W, 4), _out_text(H * W * 4), ALL),
        ("trace_tile_frames out", lambda x: r.trace_tile_frames(u, e, 2, 0, 0, W, H, out=x), f32(2, H, W, 4),
         _out_text(2 * H * W * 4), ALL),
        ("trace_tile_cameras out", lambda x: r.trace_tile_cameras(u, [u, u], e, 0, 0, W, H, out=x), f32(2, H, W, 4),
         _out_text(2 * H * W * 4), ALL),
        ("query_rays rays", lambda x: r.query_rays(x), s.rays,
         "rays must be a contiguous float32 (n, 2, 4) CUDA tensor or array", ALL),
        ("query_rays out", lambda x: r.query_rays(s.rays, out=x), hits,
         "out must be a contiguous int32 (n, 2) CUDA tensor", ALL),
        ("denoise color", lambda x: r.denoise(x, s.aov), s.color, COLOR_TEXT, ALL),
        ("denoise out", lambda x: r.denoise(s.color, s.aov, out=x), f32(H, W, 4), FILTER_OUT_TEXT, ALL),
        ("denoise float out for rgba8", lambda x: r.denoise(s.color, s.aov, rgba8=True, out=x), rgba8,
         FILTER_OUT_TEXT, ("dtype",)),
        ("denoise_var color", lambda x: r.denoise_var(x, s.aov, s.var, 2), s.color, COLOR_TEXT, ALL),
        ("denoise_var var", lambda x: r.denoise_var(s.color, s.aov, x, 2), s.var,
         f"var must be a float32 tensor of shape {(H, W)} on {dev}", ("dtype", "shape", "cpu")),
        ("denoise_var count", lambda x: r.denoise_var(s.color, s.aov, s.var, x), f32(H, W) + 2,
         "count must be a number or a tensor of var's shape on its device", ("shape", "cpu")),
        ("denoise_var out", lambda x: r.denoise_var(s.color, s.aov, s.var, 2, out=x), f32(H, W, 4), FILTER_OUT_TEXT, ALL),
        ("denoise_var var_out", lambda x: r.denoise_var(s.color, s.aov, s.var, 2, var_out=x), f32(H, W),
         "var_out must be a contiguous float32 CUDA tensor of var's shape", ALL + ("uint8",)),
        ("accumulate color", lambda x: r.accumulate(u, [u], x, s.aov), s.color, COLOR_TEXT, ALL),
        ("accumulate out", lambda x: r.accumulate(u, [u], s.color, s.aov, out=x), f32(H, W, 4), ACC_OUT_TEXT,
         ALL + ("uint8",)),
        ("accumulate prev colour", lambda x: r.accumulate(u, [u], s.color, s.aov, prev=(x, s.aov, u)), s.acc,
         f"prev's colour must be a contiguous float32 tensor of shape {(H, W, 4)} on {dev}", ALL),
        ("accumulate_var color", lambda x: r.accumulate_var(u, [u], x, s.aov, s.vmean), s.color, COLOR_TEXT, ALL),
        ("accumulate_var vmean", lambda x: r.accumulate_var(u, [u], s.color, s.aov, x), s.vmean,
         plane("vmean", (H, W)), ALL),
        ("accumulate_var weight", lambda x: r.accumulate_var(u, [u], s.color, s.aov, s.vmean, weight=x), f32(H, W) + 1,
         plane("weight", (H, W)), ALL),
        ("accumulate_var out", lambda x: r.accumulate_var(u, [u], s.color, s.aov, s.vmean, out=x), f32(H, W, 4),
         ACC_OUT_TEXT, ALL + ("uint8",)),
        ("accumulate_var var_out", lambda x: r.accumulate_var(u, [u], s.color, s.aov, s.vmean, var_out=x), f32(H, W),
         plane("var_out", (H, W)), ALL + ("uint8",)),
        ("accumulate_var prev colour",
         lambda x: r.accumulate_var(u, [u], s.color, s.aov, s.vmean, prev=(x, s.aov, u, s.acc_var)), s.acc,
         f"prev's colour must be a contiguous float32 tensor of shape {(H, W, 4)} on {dev}", ALL),
        ("accumulate_var prev variance",
         lambda x: r.accumulate_var(u, [u], s.color, s.aov, s.vmean, prev=(s.acc, s.aov, u, x)), s.acc_var,
         {"shape": f"prev's variance must be a float32 tensor of shape {(H, W)} on {dev}",
          "dtype": plane("prev's variance", (H, W)), "strided": plane("prev's variance", (H, W)),
          "cpu": plane("prev's variance", (H, W))}, ALL),
        ("trace_pixels pixels", lambda x: r.trace_pixels(u, e, x), s.px, PIXELS_TEXT, ALL),
        ("trace_pixels out", lambda x: r.trace_pixels(u, e, s.px, out=x), f32(N, 4), _out_text(N * 4), ALL),
        ("blend_pixels image", lambda x: r.blend_pixels(x, s.px, s.extra, 1.0), s.acc, IMAGE_TEXT, ALL),
        ("blend_pixels pixels", lambda x: r.blend_pixels(s.acc, x, s.extra, 1.0), s.px, PIXELS_TEXT, ALL),
        ("blend_pixels extra", lambda x: r.blend_pixels(s.acc, s.px, x, 1.0), s.extra, entries("extra", (N, 4)), ALL),
        ("blend_pixels_var image", lambda x: r.blend_pixels_var(x, s.acc_var, s.px, s.extra, s.extra_var, 1.0), s.acc,
         IMAGE_TEXT, ALL),
        ("blend_pixels_var var", lambda x: r.blend_pixels_var(s.acc, x, s.px, s.extra, s.extra_var, 1.0), s.acc_var,
         entries("var", (H, W)), ALL),
        ("blend_pixels_var pixels", lambda x: r.blend_pixels_var(s.acc, s.acc_var, x, s.extra, s.extra_var, 1.0), s.px,
         PIXELS_TEXT, ALL),
        ("blend_pixels_var extra", lambda x: r.blend_pixels_var(s.acc, s.acc_var, s.px, x, s.extra_var, 1.0), s.extra,
         entries("extra", (N, 4)), ALL),
        ("blend_pixels_var extra_vmean", lambda x: r.blend_pixels_var(s.acc, s.acc_var, s.px, s.extra, x, 1.0),
         s.extra_var, entries("extra_vmean", (N,)), ALL),
        ("trace_tile_var out", lambda x: r.trace_tile_var(u, e, 0, 0, W, H, out=x), f32(H, W, 4), _out_text(H * W * 4),
         ALL),
        ("trace_tile_var var", lambda x: r.trace_tile_var(u, e, 0, 0, W, H, var=x), f32(H, W),
         f"var must be a contiguous float32 CUDA tensor of shape {(H, W)}", ALL),
        ("trace_tile_var var of frames", lambda x: r.trace_tile_var(u, e, 0, 0, W, H, n_frames=2, var=x), f32(2, H, W),
         f"var must be a contiguous float32 CUDA tensor of shape {(2, H, W)}", ALL),
        ("trace_pixels_var pixels", lambda x: r.trace_pixels_var(u, e, x), s.px, PIXELS_TEXT, ALL),
        ("trace_pixels_var out", lambda x: r.trace_pixels_var(u, e, s.px, out=x), f32(N, 4), _out_text(N * 4), ALL),
        ("trace_pixels_var var", lambda x: r.trace_pixels_var(u, e, s.px, var=x), f32(N),
         f"var must be a contiguous float32 CUDA tensor of {N} elements", ALL),
        ("trace_pixel_lists pixels", lambda x: r.trace_pixel_lists(u, None, e, x, [0, 2, N]), s.px, PIXELS_TEXT, ALL),
        ("trace_pixel_lists out", lambda x: r.trace_pixel_lists(u, None, e, s.px, [0, 2, N], out=x), f32(N, 4),
         _out_text(N * 4), ALL),
        ("trace_pixel_lists var", lambda x: r.trace_pixel_lists(u, None, e, s.px, [0, 2, N], var=x), f32(N),
         f"var must be None, True or a contiguous float32 CUDA tensor of {N} elements", ALL),
        ("top_up_var acc", lambda x: r.top_up_var(u, u, e, x, s.acc_var, s.aov, 2, 2**20, n_min=2.0), s.acc,
         "acc must be one (h, w, 4) frame and var its (h, w) variance", ("shape",)),
        ("top_up_var var", lambda x: r.top_up_var(u, u, e, s.acc, x, s.aov, 2, 2**20, n_min=2.0), s.acc_var,
         "acc must be one (h, w, 4) frame and var its (h, w) variance", ("shape",)),
    ]
    for k, (shape, dt) in AOV_SHAPES.items():
        swap = lambda x, k=k: dict(s.aov, **{k: x})  # noqa: E731
        text = f"must be a contiguous {dt} tensor of shape {shape} on {dev}"
        cases += [
            (f"trace_aov out {k}", lambda x, k=k: r.trace_aov(u, x0=0, y0=0, w=W, h=H, out={k: x}), s.aov[k],
             f"out[{k!r}] must be a contiguous {dt} CUDA tensor of shape {shape}", ALL),
            (f"denoise aov {k}", lambda x, swap=swap: r.denoise(s.color, swap(x)), s.aov[k], f"aov[{k!r}] " + text, ALL),
            (f"denoise_var aov {k}", lambda x, swap=swap: r.denoise_var(s.color, swap(x), s.var, 2), s.aov[k],
             f"aov[{k!r}] " + text, ALL),
            (f"accumulate aov {k}", lambda x, swap=swap: r.accumulate(u, [u], s.color, swap(x)), s.aov[k],
             f"aov[{k!r}] " + text, ALL),
            (f"accumulate prev aov {k}",
             lambda x, swap=swap: r.accumulate(u, [u], s.color, s.aov, prev=(s.acc, swap(x), u)), s.aov[k],
             f"prev's aov[{k!r}] " + text, ALL),
            (f"accumulate_var prev aov {k}",
             lambda x, swap=swap: r.accumulate_var(u, [u], s.color, s.aov, s.vmean, prev=(s.acc, swap(x), u, s.acc_var)),
             s.aov[k], f"prev's aov[{k!r}] " + text, ALL),
        ]
    return cases


def test_texts_of_one_wrong_argument(S):
    """One wrong tensor at a time -- another dtype, another shape, strided, on the CPU, uint8 where float32 is
    due -- for every method that checks its tensors: the whole ValueError text; nothing is launched."""
    s = S
    before = s.r.last_call()
    cases = _cases(s)
    n = 0
    for label, call, good, text, kinds in cases:
        for kind, x in _wrong(good, kinds).items():
            want = text[kind] if isinstance(text, dict) else text
            with pytest.raises(ValueError, match="^" + re.escape(want) + "$"):
                call(x)
                pytest.fail(f"{label}: {kind} was accepted")
            n += 1
    assert n == 248, n  # every case above was reached
    # arguments that are not tensors
    for call, want in (
            (lambda: s.r.trace_aov(s.u, x0=0, y0=0, w=W, h=H, want=("depth",)),
             "want must name some of ('normal_depth', 'albedo', 'id')"),
            (lambda: s.r.denoise(s.color, {"id": s.aov["id"]}),
             "aov must hold the buffers ('normal_depth', 'albedo', 'id') of trace_aov"),
            (lambda: s.r.denoise(s.color, s.aov, n_passes=9), "n_passes must be 1..8"),
            (lambda: s.r.denoise_var(s.color, s.aov, s.var, 0), "count must be positive"),
            (lambda: s.r.accumulate(s.u, [s.u, s.u], s.color, s.aov), "1 frames need 1 cameras, not 2"),
            (lambda: s.r.accumulate_var(s.u, [], s.color, s.aov, s.vmean), "1 frames need 1 cameras, not 0"),
            (lambda: s.r.accumulate(s.u, [s.u], s.color, s.aov, n_max=0), "n_max must be 1..65535"),
            (lambda: s.r.trace_tile_cameras(s.u, np.zeros((2, 9), dtype=np.float32), s.e, 0, 0, W, H), CAMERA_TEXT),
            (lambda: s.r.trace_pixels(s.u, s.e, np.zeros((N, 2), dtype=np.float32)), "pixels must hold integers"),
            (lambda: s.r.top_up_var(s.u, s.u, s.e, s.acc, s.acc_var, s.aov, 2, 2**20),
             "top_up_var needs n_min, rel_tol or both")):
        with pytest.raises(ValueError, match="^" + re.escape(want) + "$"):
            call()
    assert s.r.last_call() == before


def test_which_of_two_wrong_arguments_is_reported(S):
    """Two wrong arguments in one call: the text is that of the check that stands first in the method."""
    import torch

    s = S
    r, u, e = s.r, s.u, s.e
    before = r.last_call()
    cpu = lambda t: t.cpu()  # noqa: E731
    bad_aov = dict(s.aov, albedo=cpu(s.aov["albedo"]))
    aov_text = f"aov['albedo'] must be a contiguous torch.float32 tensor of shape {(1, H, W, 4)} on {s.dev}"
    plane = lambda what, shape: f"{what} must be a contiguous float32 tensor of shape {shape} on {s.dev}"  # noqa: E731
    entries = lambda what, shape: f"{what} must be a contiguous float32 {shape} tensor on {s.dev}"  # noqa: E731
    u8 = torch.zeros((H, W, 4), dtype=torch.uint8)
    pairs = [
        (lambda: r.quantize(cpu(s.color), out=u8), "rgba must be a contiguous float32 CUDA tensor [..., 4]"),
        (lambda: r.trace_tile_cameras(u, np.zeros((2, 9)), e, 0, 0, W, H, out=cpu(s.color)), CAMERA_TEXT),
        (lambda: r.query_rays(cpu(s.rays), out=torch.zeros((N, 2))),
         "rays must be a contiguous float32 (n, 2, 4) CUDA tensor or array"),
        (lambda: r.trace_aov(u, x0=0, y0=0, w=W, h=H, want=(), out={"id": cpu(s.aov["id"])}),
         "want must name some of ('normal_depth', 'albedo', 'id')"),
        (lambda: r.trace_aov(u, x0=0, y0=0, w=W, h=H, out={k: cpu(v) for k, v in s.aov.items()}),
         f"out['normal_depth'] must be a contiguous torch.float32 CUDA tensor of shape {(1, H, W, 4)}"),
        (lambda: r.denoise(cpu(s.color), bad_aov), COLOR_TEXT),
        (lambda: r.denoise(s.color, bad_aov, n_passes=0), aov_text),
        (lambda: r.denoise(s.color, s.aov, n_passes=0, out=cpu(s.color)), "n_passes must be 1..8"),
        (lambda: r.denoise_var(s.color, bad_aov, cpu(s.var), 2), aov_text),
        (lambda: r.denoise_var(s.color, s.aov, cpu(s.var), 0), f"var must be a float32 tensor of shape {(H, W)} on {s.dev}"),
        (lambda: r.denoise_var(s.color, s.aov, s.var, 0, n_passes=0), "count must be positive"),
        (lambda: r.denoise_var(s.color, s.aov, s.var, 2, out=cpu(s.color), var_out=cpu(s.var)), FILTER_OUT_TEXT),
        (lambda: r.accumulate(u, [u, u], s.color, bad_aov), "1 frames need 1 cameras, not 2"),
        (lambda: r.accumulate(u, [u], s.color, bad_aov, n_max=0), aov_text),
        (lambda: r.accumulate(u, [u], s.color, s.aov, out=cpu(s.color), prev=(cpu(s.acc), s.aov, u)), ACC_OUT_TEXT),
        (lambda: r.accumulate(u, [u], s.color, s.aov, prev=(cpu(s.acc), bad_aov, np.zeros(9))),
         f"prev's colour must be a contiguous float32 tensor of shape {(H, W, 4)} on {s.dev}"),
        (lambda: r.accumulate(u, [u], s.color, s.aov, prev=(s.acc, bad_aov, np.zeros(9))), CAMERA_TEXT),
        (lambda: r.accumulate_var(u, [u], s.color, s.aov, cpu(s.vmean), weight=cpu(s.vmean), n_max=0),
         "n_max must be 1..65535"),
        (lambda: r.accumulate_var(u, [u], s.color, s.aov, cpu(s.vmean), weight=cpu(s.vmean)), plane("vmean", (H, W))),
        (lambda: r.accumulate_var(u, [u], s.color, s.aov, s.vmean, weight=cpu(s.vmean), out=cpu(s.color)),
         plane("weight", (H, W))),
        (lambda: r.accumulate_var(u, [u], s.color, s.aov, s.vmean, out=cpu(s.color), var_out=cpu(s.var)), ACC_OUT_TEXT),
        (lambda: r.accumulate_var(u, [u], s.color, s.aov, s.vmean, var_out=cpu(s.var),
                                  prev=(cpu(s.acc), s.aov, u, s.acc_var)), plane("var_out", (H, W))),
        (lambda: r.accumulate_var(u, [u], s.color, s.aov, s.vmean, prev=(cpu(s.acc), s.aov, u, cpu(s.acc_var))),
         f"prev's colour must be a contiguous float32 tensor of shape {(H, W, 4)} on {s.dev}"),
        (lambda: r.accumulate_var(u, [u], s.color, s.aov, s.vmean, prev=(s.acc, bad_aov, u, cpu(s.acc_var))),
         plane("prev's variance", (H, W))),
        (lambda: r.trace_pixels(u, e, cpu(s.px), out=cpu(s.extra)), PIXELS_TEXT),
        (lambda: r.blend_pixels(cpu(s.acc), cpu(s.px), s.extra, 1.0), IMAGE_TEXT),
        (lambda: r.blend_pixels(s.acc, cpu(s.px), cpu(s.extra), 1.0), PIXELS_TEXT),
        (lambda: r.blend_pixels_var(cpu(s.acc), cpu(s.acc_var), s.px, s.extra, s.extra_var, 1.0), IMAGE_TEXT),
        (lambda: r.blend_pixels_var(s.acc, cpu(s.acc_var), cpu(s.px), s.extra, s.extra_var, 1.0), entries("var", (H, W))),
        (lambda: r.blend_pixels_var(s.acc, s.acc_var, cpu(s.px), cpu(s.extra), s.extra_var, 1.0), PIXELS_TEXT),
        (lambda: r.blend_pixels_var(s.acc, s.acc_var, s.px, cpu(s.extra), cpu(s.extra_var), 1.0),
         entries("extra", (N, 4))),
        (lambda: r.trace_tile_var(u, e, 0, 0, W, H, cameras=np.zeros((1, 9)), out=cpu(s.color)), CAMERA_TEXT),
        (lambda: r.trace_tile_var(u, e, 0, 0, W, H, out=cpu(s.color), var=cpu(s.var)), _out_text(H * W * 4)),
        (lambda: r.trace_pixels_var(u, e, cpu(s.px), var=cpu(s.extra_var)), PIXELS_TEXT),
        (lambda: r.trace_pixels_var(u, e, s.px, out=cpu(s.extra), var=cpu(s.extra_var)), _out_text(N * 4)),
        (lambda: r.trace_pixel_lists(u, None, e, cpu(s.px), [0, 2]), PIXELS_TEXT),
        (lambda: r.trace_pixel_lists(u, None, e, s.px, [0, 2], out=cpu(s.extra)),
         f"offsets end at 2, the pixel array holds {N} entries"),
        (lambda: r.trace_pixel_lists(u, [u], e, s.px, [0, 2, N], frame_keys=[1]), "2 lists need 2 cameras, not 1"),
        (lambda: r.trace_pixel_lists(u, None, e, s.px, [0, 2, N], frame_keys=[1], out=cpu(s.extra)),
         "2 lists need 2 frame keys, not 1"),
        (lambda: r.trace_pixel_lists(u, None, e, s.px, [0, 2, N], out=cpu(s.extra), var=cpu(s.extra_var)),
         _out_text(N * 4)),
        (lambda: r.top_up_var(u, u, e, cpu(s.acc)[None], s.acc_var, s.aov, 2, 2**20),
         "top_up_var needs n_min, rel_tol or both"),
    ]
    for i, (call, want) in enumerate(pairs):
        with pytest.raises(ValueError, match="^" + re.escape(want) + "$"):
            call()
            pytest.fail(f"pair {i} was accepted")
    assert r.last_call() == before


def _stream_of(r):
    from mirror_maze import lib

    h = C.c_void_p()
    r._check(lib().mm_get_stream(r._ctx, C.byref(h)))
    return h.value or 0


def _sixteen(s):
    """The 16 methods that enqueue on the stream, each with valid tiny arguments."""
    r, u, e = s.r, s.u, s.e
    return [
        ("quantize", lambda: r.quantize(s.color)),
        ("trace_tile", lambda: r.trace_tile(u, e, 0, 0, W, H)),
        ("trace_tile_frames", lambda: r.trace_tile_frames(u, e, 2, 0, 0, W, H)),
        ("trace_tile_cameras", lambda: r.trace_tile_cameras(u, [u, u], e, 0, 0, W, H)),
        ("query_rays", lambda: r.query_rays(s.rays)),
        ("trace_aov", lambda: r.trace_aov(u, x0=0, y0=0, w=W, h=H)),
        ("denoise", lambda: r.denoise(s.color, s.aov, n_passes=1)),
        ("denoise_var", lambda: r.denoise_var(s.color, s.aov, s.var, 2, n_passes=1)),
        ("accumulate", lambda: r.accumulate(u, [u], s.color, s.aov)),
        ("accumulate_var", lambda: r.accumulate_var(u, [u], s.color, s.aov, s.vmean)),
        ("trace_pixels", lambda: r.trace_pixels(u, e, s.px)),
        ("blend_pixels", lambda: r.blend_pixels(s.acc.clone(), s.px, s.extra, 1.0)),
        ("blend_pixels_var", lambda: r.blend_pixels_var(s.acc.clone(), s.acc_var.clone(), s.px, s.extra, s.extra_var,
                                                        1.0)),
        ("trace_tile_var", lambda: r.trace_tile_var(u, e, 0, 0, W, H)),
        ("trace_pixels_var", lambda: r.trace_pixels_var(u, e, s.px)),
        ("trace_pixel_lists", lambda: r.trace_pixel_lists(u, None, e, s.px, [0, 2, N])),
    ]


def test_calls_follow_the_current_stream_unless_one_is_pinned(S):
    """Without a pinned stream each of the 16 methods leaves the context on torch's current stream; with one
    pinned they leave it there; set_stream(None) makes the next call follow again."""
    import torch

    from mirror_maze import lib

    s = S
    r = s.r
    calls = _sixteen(s)
    assert len(calls) == 16 and not r._pinned_stream
    a, b = torch.cuda.Stream(device=s.dev), torch.cuda.Stream(device=s.dev)
    assert len({0, a.cuda_stream, b.cuda_stream}) == 3
    keep = []  # every result lives until the final synchronize
    with torch.cuda.stream(a):
        for name, call in calls:
            r._check(lib().mm_set_stream(r._ctx, b.cuda_stream))  # (the C call: it leaves the binding unpinned)
            keep.append(call())
            assert _stream_of(r) == a.cuda_stream, name
    torch.cuda.synchronize()
    r.set_stream(b)
    try:
        with torch.cuda.stream(a):
            for name, call in calls:
                keep.append(call())
                assert _stream_of(r) == b.cuda_stream, name
        torch.cuda.synchronize()
    finally:
        r.set_stream(None)
    assert _stream_of(r) not in (a.cuda_stream, b.cuda_stream)
    with torch.cuda.stream(a):
        keep.append(calls[1][1]())
        assert _stream_of(r) == a.cuda_stream
    torch.cuda.synchronize()
    r.sync()


# What empty inputs give, as the binding gave them before the fold (recorded from a run of this file on it).
EMPTY_LIST_CALLS = 0  # call numbers the four empty list calls take
NO_CAMERAS = {"trace_tile_cameras": (-1, "mm_trace_tile_cameras: no cameras"),
              "trace_tile_var": (-1, "mm_trace_tile: null argument")}


def test_empty_inputs(S):
    """Zero cameras are refused by the library, by a text that depends on the pointer the binding passes (null
    from trace_tile_cameras, the empty array's from trace_tile_var); empty lists and zero rays launch nothing
    and give empty results."""
    import torch

    from mirror_maze import MMError, lib

    s = S
    r, u, e = s.r, s.u, s.e
    seen = {}
    for name, call in (("trace_tile_cameras", lambda: r.trace_tile_cameras(u, [], e, 0, 0, W, H)),
                       ("trace_tile_var", lambda: r.trace_tile_var(u, e, 0, 0, W, H, cameras=[]))):
        with pytest.raises(MMError) as ei:
            call()
        seen[name] = (ei.value.code, lib().mm_last_error(r._ctx).decode())
        assert str(ei.value) == f"[{seen[name][0]}] {seen[name][1]}"
    print("zero cameras:", seen)
    before = r.last_call()
    none = torch.zeros((0, 2), dtype=torch.int32, device=s.dev)
    out, st = r.trace_pixels(u, e, none, stats=True)
    assert tuple(out.shape) == (0, 4) and out.dtype == torch.float32 and (st.rays, st.paths) == (0, 0)
    out, var, st = r.trace_pixels_var(u, e, none, stats=True)
    assert tuple(out.shape) == (0, 4) and tuple(var.shape) == (0,) and (st.rays, st.paths) == (0, 0)
    out, var, st = r.trace_pixel_lists(u, None, e, none, [0, 0, 0], var=True, stats=True)
    assert tuple(out.shape) == (0, 4) and tuple(var.shape) == (0,) and (st.rays, st.paths) == (0, 0)
    out, var, st = r.trace_pixel_lists(u, None, e, np.zeros((0, 2), dtype=np.uint32), [0, 0])
    assert tuple(out.shape) == (0, 4) and var is None and st is None
    print("last_call before / after the empty lists:", before, r.last_call())
    acc, acc_var = s.acc.clone(), s.acc_var.clone()
    assert r.blend_pixels(acc, none, torch.zeros((0, 4), device=s.dev), 1.0) is acc
    got = r.blend_pixels_var(acc, acc_var, none, torch.zeros((0, 4), device=s.dev), torch.zeros((0,), device=s.dev), 1.0)
    assert got[0] is acc and got[1] is acc_var
    t, k = r.query_rays(torch.zeros((0, 2, 4), device=s.dev))
    assert tuple(t.shape) == tuple(k.shape) == (0,) and t.dtype == torch.float32 and k.dtype == torch.int32
    t, k = r.query_rays(np.zeros((0, 2, 4)))
    assert tuple(t.shape) == tuple(k.shape) == (0,)
    r.sync()
    assert torch.equal(acc, s.acc) and torch.equal(acc_var, s.acc_var)
    assert seen == NO_CAMERAS
    assert r.last_call() == before + EMPTY_LIST_CALLS
