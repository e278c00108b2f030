"""The Python binding's argument handling, on the CPU: the ext a trace call and an extra-sample round pass down,
camera and pixel-list conversion, the offsets / frame keys of trace_pixel_lists, the null pointers of empty
lists, and the refusal of CPU tensors.  Nothing here needs the library: the methods run on a Renderer without a
context, over a stand-in for lib() that records every call and returns MM_OK, on CPU tensors that claim to be
CUDA tensors.  The expectations were first run against the binding as it stood before its repeated steps were
folded (every step inline in every method); nothing differed."""
from __future__ import annotations

import ctypes as C
import itertools
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from mirror_maze import _lib, make_ext, mm_camera, mm_uniform  # noqa: E402
from mirror_maze import renderer as R  # noqa: E402
from mirror_maze.renderer import Renderer  # noqa: E402

STRIPPED = _lib.MM_EXT_ACCUMULATE | _lib.MM_EXT_RGBA8 | _lib.MM_EXT_COUNT_STATS
CAMERA_TEXT = "cameras must be mm_camera / mm_uniform values or an (n, 10) float32 array"
PIXELS_TEXT = "pixels must be a contiguous int32 / uint32 (n, 2) CUDA tensor or an (n, 2) array"


class _OnGpu(torch.Tensor):
    """A CPU tensor that answers is_cuda with True: it passes the binding's checks, and nothing reads it."""
    is_cuda = property(lambda self: True)


def _gpu(t):
    return t.as_subclass(_OnGpu)


class _Lib:
    """Stands in for lib(): every entry point records (name, args, peek(name, args)) and returns MM_OK."""

    def __init__(self, peek=None):
        self.calls, self.peek = [], peek

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args, self.peek(name, args) if self.peek else None))
            return _lib.MM_OK
        return call


@pytest.fixture
def rec(monkeypatch):
    """(renderer without a context and with a pinned stream, the recording library)."""
    L = _Lib()
    monkeypatch.setattr(R, "lib", lambda: L)
    monkeypatch.setattr(torch.Tensor, "to", lambda self, *a, **k: _gpu(self))  # an "upload" stays on the CPU
    for make in ("zeros", "empty"):  # and so does a tensor made on a device

        def on_cpu(*a, _make=getattr(torch, make), **k):
            return _gpu(_make(*a, **{**k, "device": "cpu"})) if "device" in k else _make(*a, **k)
        monkeypatch.setattr(torch, make, on_cpu)
    r = Renderer.__new__(Renderer)
    r._ctx, r.device, r._view, r._pinned_stream = C.c_void_p(), 0, None, True
    return r, L


def _uniform():
    u = mm_uniform()
    u.view_w, u.view_h, u.chunk_w = 64.0, 32.0, 4
    u.cam.focal = 1.5
    return u


def _ext_of(args):
    """The mm_ext among a recorded call's arguments (passed by reference)."""
    exts = [a._obj for a in args if isinstance(getattr(a, "_obj", None), _lib.mm_ext)]
    assert len(exts) == 1
    return exts[0]


def _fields(e):
    return e.spp, e.bounce_limit, e.mirror_limit, e.frame, e.flags, e.reserved


PIXELS = np.array([[1, 2], [3, 4], [5, 6], [7, 8], [9, 10]], dtype=np.int32)

# the seven trace methods, each with small valid arguments (its C entry point is "mm_" + the method's name)
TRACE_CALLS = {
    "trace_tile": lambda r, u, e, **kw: r.trace_tile(u, e, 0, 0, 4, 2, **kw),
    "trace_tile_frames": lambda r, u, e, **kw: r.trace_tile_frames(u, e, 3, 0, 0, 4, 2, **kw),
    "trace_tile_cameras": lambda r, u, e, **kw: r.trace_tile_cameras(u, [u, u], e, 0, 0, 4, 2, **kw),
    "trace_pixels": lambda r, u, e, **kw: r.trace_pixels(u, e, PIXELS, **kw),
    "trace_tile_var": lambda r, u, e, **kw: r.trace_tile_var(u, e, 0, 0, 4, 2, **kw),
    "trace_pixels_var": lambda r, u, e, **kw: r.trace_pixels_var(u, e, PIXELS, **kw),
    "trace_pixel_lists": lambda r, u, e, **kw: r.trace_pixel_lists(u, None, e, PIXELS, [0, 2, 5], **kw),
}
OUT_SHAPE = {"trace_tile": (2, 4, 4), "trace_tile_frames": (3, 2, 4, 4), "trace_tile_cameras": (2, 2, 4, 4),
             "trace_pixels": (5, 4), "trace_tile_var": (2, 4, 4), "trace_pixels_var": (5, 4),
             "trace_pixel_lists": (5, 4)}


@pytest.mark.parametrize("name", list(TRACE_CALLS))
def test_trace_call_ext_is_the_callers_with_the_calls_flags(rec, name):
    """Every combination of stats, rgba8 and a uint8 `out`, over an ext with and without flags of its own: the C
    call named after the method gets the caller's ext with COUNT_STATS / RGBA8 or-ed in and reserved 0, and the
    method returns the stats object only when asked."""
    r, L = rec
    u = _uniform()
    for flags, stats, rgba8, out8 in itertools.product((0, _lib.MM_EXT_ACCUMULATE, 0x4 | 0x100), (False, True),
                                                       (False, True), (False, True)):
        e = make_ext(5, 6, 7, frame=11, flags=flags)
        e.reserved = 9
        out = _gpu(torch.zeros(OUT_SHAPE[name], dtype=torch.uint8)) if out8 else None
        del L.calls[:]
        ret = TRACE_CALLS[name](r, u, e, stats=stats, rgba8=rgba8, out=out)
        assert [c[0] for c in L.calls] == ["mm_" + name]
        want = flags | (_lib.MM_EXT_COUNT_STATS if stats else 0) | (_lib.MM_EXT_RGBA8 if rgba8 or out8 else 0)
        assert _fields(_ext_of(L.calls[0][1])) == (5, 6, 7, 11, want, 0)
        assert _fields(e) == (5, 6, 7, 11, flags, 9)  # the caller's ext is not written
        assert ret[0].dtype == (torch.uint8 if rgba8 or out8 else torch.float32)
        assert tuple(ret[0].shape) == OUT_SHAPE[name] and (out is None or ret[0] is out)
        assert isinstance(ret[-1], _lib.mm_stats) if stats else ret[-1] is None
        assert len(ret) == (2 if name in ("trace_tile", "trace_tile_frames", "trace_tile_cameras", "trace_pixels")
                            else 3)
        if name == "trace_pixel_lists":
            assert ret[1] is None
        elif len(ret) == 3:
            assert ret[1].dtype == torch.float32 and tuple(ret[1].shape) == OUT_SHAPE[name][:-1]


class _Rounds(Renderer):
    """A Renderer whose trace and blend calls only record their arguments."""

    def __init__(self):
        self._ctx, self.device, self._view, self._pinned_stream = C.c_void_p(), 0, None, True
        self.seen = []

    def trace_pixels(self, u, e, pixels, **kw):
        self.seen.append(("trace_pixels", u, e))
        return torch.ones((pixels.shape[0], 4)), None

    def trace_pixels_var(self, u, e, pixels, **kw):
        self.seen.append(("trace_pixels_var", u, e))
        return torch.ones((pixels.shape[0], 4)), torch.ones(pixels.shape[0]), None

    def trace_pixel_lists(self, u, cameras, e, pixels, offsets, frame_keys=None, **kw):
        self.seen.append(("trace_pixel_lists", u, e))
        return torch.ones((pixels.shape[0], 4)), torch.ones(pixels.shape[0]), None

    def blend_pixels(self, *a, **kw):
        pass

    def blend_pixels_var(self, *a, **kw):
        pass


def _camera(k=0.0):
    c = mm_camera()
    c.center[:] = [1.0 + k, 2.0, 3.0]
    c.focal = 1.25
    c.quat[:] = [0.5, -0.5, 0.25, 0.75]
    c.viewport[:] = [2.0, 1.5]
    return c


def _round(r, which, e, cam, spp=3, key=2**20 + 5):
    """One extra-sample round of method `which` over a 2 x 3 window in which every pixel is selected."""
    u = _uniform()
    acc, var, cnt = torch.ones((2, 3, 4)), torch.full((2, 3), 4.0), torch.full((2, 3), 2.0)
    ids = torch.zeros((2, 3), dtype=torch.int32)
    if which == "top_up":
        assert r.top_up(u, cam, e, acc, {"id": ids}, 2.0, spp, key)[1] == 6
    elif which == "top_up_var":
        assert r.top_up_var(u, cam, e, acc, var, ids, spp, key, n_min=2.0, rel_tol=0.1)[2] == 6
    elif which == "refine":
        assert r.refine(u, e, acc, var, cnt, 0.1, spp, key) == 6
    else:
        assert r.refine_frames(u, [cam, cam], e, acc[None].repeat(2, 1, 1, 1), var[None].repeat(2, 1, 1),
                               cnt[None].repeat(2, 1, 1), 0.1, spp, [key, key + 1]) == [6, 6]
    return r.seen[-1]


@pytest.mark.parametrize("which", ["top_up", "top_up_var", "refine", "refine_frames"])
def test_extra_sample_ext_strips_the_output_flags(which):
    """The ext of an extra-sample round: the given spp, the caller's limits, ACCUMULATE / RGBA8 / COUNT_STATS
    stripped and every other flag kept, reserved 0; the RNG frame is the key, but refine_frames keeps ext.frame
    (its keys travel as frame_keys)."""
    r = _Rounds()
    for flags in (0, 0x1, 0x2, 0x4, STRIPPED, STRIPPED | 0x100, 0x100):
        e = make_ext(8, 6, 7, frame=11, flags=flags)
        e.reserved = 9
        _, _, got = _round(r, which, e, _camera())
        frame = 11 if which == "refine_frames" else 2**20 + 5
        assert _fields(got) == (3, 6, 7, frame, flags & ~STRIPPED, 0)
        assert _fields(e) == (8, 6, 7, 11, flags, 9)


def test_camera_conversion():
    """One camera as mm_camera, mm_uniform or 10 floats (float32, float64, (10,) or (1, 10)) reaches the trace call
    as uniform.cam, the other fields of the caller's uniform kept and the caller's uniform not written; sequences
    through Renderer._cameras; the refusal text."""
    cam = _camera(0.5)
    row = np.frombuffer(bytes(cam), dtype=np.float32)
    holder = mm_uniform()
    holder.cam = cam
    for which in ("top_up", "top_up_var"):
        for given in (cam, holder, row.copy(), row.astype(np.float64), row.reshape(1, 10).copy()):
            r = _Rounds()
            _, u, _ = _round(r, which, make_ext(8, 6, 7), given)
            assert bytes(u.cam) == bytes(cam)
            assert (u.view_w, u.view_h, u.chunk_w) == (64.0, 32.0, 4)
        for bad in (np.zeros(9, dtype=np.float32), np.zeros((2, 10), dtype=np.float32)):
            with pytest.raises(ValueError, match=re.escape(CAMERA_TEXT)):
                _round(_Rounds(), which, make_ext(8, 6, 7), bad)
    rows = np.stack([np.frombuffer(bytes(_camera(k)), dtype=np.float32) for k in range(3)])
    for given in ([_camera(k) for k in range(3)], rows, rows.astype(np.float64)):
        got = Renderer._cameras(given)
        assert got.dtype == np.float32 and got.flags.c_contiguous and np.array_equal(got, rows)
    assert Renderer._cameras([]).shape == (0, 10)
    for bad in (np.zeros((3, 9), dtype=np.float32), np.zeros(10, dtype=np.float32), np.zeros((1, 1, 10))):
        with pytest.raises(ValueError, match=re.escape(CAMERA_TEXT)):
            Renderer._cameras(bad)


def _peek_lists(name, args):
    """What mm_trace_pixel_lists was given, read while its arrays live: (n_lists, offsets, keys, cameras, null
    pixels, null out, null var)."""
    if name != "mm_trace_pixel_lists":
        return None
    _, _, cams, _, keys, n_lists, pixels, offs, out, var, _ = args
    read = lambda p, t, n: None if p is None else np.ctypeslib.as_array((t * n).from_address(p)).copy()  # noqa: E731
    return (n_lists, read(offs, C.c_uint64, n_lists + 1), read(keys, C.c_uint32, n_lists),
            read(cams, C.c_float, 10 * n_lists), pixels is None, out is None, var is None)


def test_offsets_and_frame_keys(rec):
    """offsets and frame_keys as list, numpy array (any integer dtype) and CPU tensor reach the call as uint64 /
    uint32 arrays; the refusals, each with its text, in the order offsets, cameras, keys."""
    r, L = rec
    L.peek = _peek_lists
    u, e = _uniform(), make_ext(2, 2, 2)
    keys = [2**31 + 11, 5, 9000]
    for offs, ks in (([0, 2, 2, 5], keys), (np.array([0, 2, 2, 5], dtype=np.int32), np.array(keys, dtype=np.int64)),
                     (np.array([0, 2, 2, 5], dtype=np.uint64), np.array(keys, dtype=np.uint32)),
                     (torch.tensor([0, 2, 2, 5]), keys), (torch.tensor([0, 2, 2, 5], dtype=torch.int32), None)):
        r.trace_pixel_lists(u, None, e, PIXELS, offs, frame_keys=ks)
        n_lists, got_offs, got_keys, cams, *null = L.calls[-1][2]
        assert n_lists == 3 and got_offs.tolist() == [0, 2, 2, 5] and cams is None and null == [False, False, True]
        assert got_keys is None if ks is None else got_keys.tolist() == keys
    rows = np.stack([np.frombuffer(bytes(_camera(k)), dtype=np.float32) for k in range(3)])
    _, v, _ = r.trace_pixel_lists(u, rows, e, PIXELS, [0, 2, 2, 5], var=True)
    assert L.calls[-1][2][3].tolist() == rows.reshape(-1).tolist() and L.calls[-1][2][4:] == (False, False, False)
    assert v.dtype == torch.float32 and tuple(v.shape) == (5,)
    n = len(L.calls)
    for offs, cams, ks, text in (
            ([5], None, None, "offsets must hold n_lists + 1 values, n_lists >= 1"),
            ([], None, None, "offsets must hold n_lists + 1 values, n_lists >= 1"),
            ([0, 2, 4], None, None, "offsets end at 4, the pixel array holds 5 entries"),
            ([0, 2, 6], rows, keys, "offsets end at 6, the pixel array holds 5 entries"),
            ([0, 2, 5], rows, keys, "2 lists need 2 cameras, not 3"),
            ([0, 2, 5], rows[:2], keys, "2 lists need 2 frame keys, not 3"),
            ([0, 2, 2, 5], None, [1, 2], "3 lists need 3 frame keys, not 2"),
            ([0, 2, 2, 5], rows[:, :9], keys, CAMERA_TEXT)):
        with pytest.raises(ValueError, match=re.escape(text)):
            r.trace_pixel_lists(u, cams, e, PIXELS, offs, frame_keys=ks)
    assert len(L.calls) == n  # a refused call reaches no entry point


def _peek_pixels(name, args):
    """The (n, 2) int32 entries mm_trace_pixels was given."""
    if name != "mm_trace_pixels":
        return None
    _, _, _, pixels, n, out, _ = args
    return None if pixels is None else np.ctypeslib.as_array((C.c_int32 * (2 * n)).from_address(pixels)).copy()


def test_pixel_arrays(rec):
    """An array of pixels is uploaded as int32 with the bits of uint32: any integer dtype, (n, 2) or flat;
    non-integers are refused; a uint32 / int32 tensor is taken as it is."""
    r, L = rec
    L.peek = _peek_pixels
    u, e = _uniform(), make_ext(2, 2, 2)
    big = np.array([[2**32 - 1, 2**31], [7, 0]], dtype=np.uint32)
    for given in (big, big.astype(np.uint64), big.astype(np.int64), big.reshape(-1), big.view(np.int32), big.tolist()):
        out, _ = r.trace_pixels(u, e, given)
        assert tuple(out.shape) == (2, 4)
        assert L.calls[-1][2].view(np.uint32).tolist() == big.reshape(-1).tolist()
    for bad in (big.astype(np.float32), big.astype(np.float64), np.zeros((2, 2), dtype=bool), [[0.5, 1.0]]):
        for call in (r.trace_pixels, r.trace_pixels_var):
            with pytest.raises(ValueError, match=re.escape("pixels must hold integers")):
                call(u, e, bad)
    t = _gpu(torch.from_numpy(big.view(np.int32).copy()))
    r.trace_pixels(u, e, t)
    assert L.calls[-1][1][3] == t.data_ptr()
    if hasattr(torch, "uint32"):
        t = _gpu(torch.from_numpy(big.view(np.int32).copy()).view(torch.uint32))
        r.trace_pixels(u, e, t)
        assert L.calls[-1][1][3] == t.data_ptr()
    for bad in (_gpu(torch.zeros((2, 2), dtype=torch.int64)), _gpu(torch.zeros((2, 3), dtype=torch.int32)),
                _gpu(torch.zeros((4, 2), dtype=torch.int32))[::2], _gpu(torch.zeros(4, dtype=torch.int32))):
        with pytest.raises(ValueError, match=re.escape(PIXELS_TEXT)):
            r.trace_pixels(u, e, bad)


def test_empty_lists_pass_null_pointers(rec):
    """n = 0: the list calls pass null pixel / out / var pointers; zero cameras are a null pointer in
    trace_tile_cameras and trace_aov and the (empty) array's pointer in trace_tile_var."""
    r, L = rec
    u, e = _uniform(), make_ext(2, 2, 2)
    none = np.zeros((0, 2), dtype=np.int32)
    r.trace_pixels(u, e, none)
    assert L.calls[-1][1][3:6] == (None, 0, None)
    r.trace_pixels_var(u, e, none)
    assert L.calls[-1][1][3:7] == (None, 0, None, None)
    r.trace_pixel_lists(u, None, e, none, [0, 0], var=True)
    assert (L.calls[-1][1][6], L.calls[-1][1][8], L.calls[-1][1][9]) == (None, None, None)
    r.blend_pixels(_gpu(torch.zeros((2, 3, 4))), none, _gpu(torch.zeros((0, 4))), 1.0)
    assert L.calls[-1][0] == "mm_blend_pixels" and L.calls[-1][1][6:9] == (None, None, 0)
    r.blend_pixels_var(_gpu(torch.zeros((2, 3, 4))), _gpu(torch.zeros((2, 3))), none, _gpu(torch.zeros((0, 4))),
                       _gpu(torch.zeros((0,))), 1.0)
    assert L.calls[-1][0] == "mm_blend_pixels_var" and L.calls[-1][1][7:11] == (None, None, None, 0)
    t, k = r.query_rays(np.zeros((0, 2, 4), dtype=np.float32))
    assert L.calls[-1][0] == "mm_query_rays" and L.calls[-1][1][1:] == (None, 0, None)
    assert t.dtype == torch.float32 and k.dtype == torch.int32 and tuple(t.shape) == tuple(k.shape) == (0,)
    r.trace_tile_cameras(u, [], e, 0, 0, 4, 2)
    assert L.calls[-1][1][2] is None and L.calls[-1][1][4] == 0
    r.trace_aov(u, [], x0=0, y0=0, w=4, h=2, want=("id",))
    assert L.calls[-1][0] == "mm_trace_aov" and L.calls[-1][1][2:4] == (None, 0)
    r.trace_tile_var(u, e, 0, 0, 4, 2, cameras=[])
    assert L.calls[-1][0] == "mm_trace_tile_var" and L.calls[-1][1][2] is not None and L.calls[-1][1][4] == 0


def test_cpu_tensors_are_refused(rec):
    """A CPU tensor where a CUDA tensor is due: every method's own text, and no entry point is reached."""
    r, L = rec
    u, e = _uniform(), make_ext(2, 2, 2)
    f = lambda *s: torch.zeros(s)  # noqa: E731
    aov = {"normal_depth": _gpu(f(2, 3, 4)), "albedo": _gpu(f(2, 3, 4)), "id": _gpu(torch.zeros((2, 3), dtype=torch.int32))}
    img, px = _gpu(f(2, 3, 4)), _gpu(torch.zeros((5, 2), dtype=torch.int32))
    dev = img.device
    out_text = lambda n: f"out must be a contiguous float32 or uint8 CUDA tensor of {n} elements"  # noqa: E731
    cases = [
        (lambda: r.quantize(f(2, 3, 4)), "rgba must be a contiguous float32 CUDA tensor [..., 4]"),
        (lambda: r.quantize(img, out=torch.zeros((2, 3, 4), dtype=torch.uint8)),
         "out must be a contiguous uint8 CUDA tensor of rgba's shape"),
        (lambda: r.trace_tile(u, e, 0, 0, 3, 2, out=f(2, 3, 4)), out_text(24)),
        (lambda: r.trace_tile_frames(u, e, 2, 0, 0, 3, 2, out=f(2, 2, 3, 4)), out_text(48)),
        (lambda: r.trace_tile_cameras(u, [u], e, 0, 0, 3, 2, out=f(1, 2, 3, 4)), out_text(24)),
        (lambda: r.trace_pixels(u, e, px, out=f(5, 4)), out_text(20)),
        (lambda: r.trace_pixels(u, e, torch.zeros((5, 2), dtype=torch.int32)), PIXELS_TEXT),
        (lambda: r.trace_tile_var(u, e, 0, 0, 3, 2, out=f(2, 3, 4)), out_text(24)),
        (lambda: r.trace_tile_var(u, e, 0, 0, 3, 2, var=f(2, 3)),
         "var must be a contiguous float32 CUDA tensor of shape (2, 3)"),
        (lambda: r.trace_pixels_var(u, e, px, var=f(5)), "var must be a contiguous float32 CUDA tensor of 5 elements"),
        (lambda: r.trace_pixel_lists(u, None, e, px, [0, 5], var=f(5)),
         "var must be None, True or a contiguous float32 CUDA tensor of 5 elements"),
        (lambda: r.query_rays(f(3, 2, 4)), "rays must be a contiguous float32 (n, 2, 4) CUDA tensor or array"),
        (lambda: r.query_rays(_gpu(f(3, 2, 4)), out=torch.zeros((3, 2), dtype=torch.int32)),
         "out must be a contiguous int32 (n, 2) CUDA tensor"),
        (lambda: r.trace_aov(u, x0=0, y0=0, w=3, h=2, want=("id",), out={"id": torch.zeros((1, 2, 3), dtype=torch.int32)}),
         "out['id'] must be a contiguous torch.int32 CUDA tensor of shape (1, 2, 3)"),
        (lambda: r.denoise(f(2, 3, 4), aov), "color must be a contiguous float32 CUDA tensor (h, w, 4) or (n, h, w, 4)"),
        (lambda: r.denoise(img, dict(aov, albedo=f(2, 3, 4))),
         f"aov['albedo'] must be a contiguous torch.float32 tensor of shape (1, 2, 3, 4) on {dev}"),
        (lambda: r.denoise(img, aov, out=f(2, 3, 4)),
         "out must be a contiguous float32 (uint8 for RGBA8) CUDA tensor of color's shape"),
        (lambda: r.denoise_var(img, aov, f(2, 3), 8), f"var must be a float32 tensor of shape (2, 3) on {dev}"),
        (lambda: r.accumulate(u, [u], f(2, 3, 4), aov),
         "color must be a contiguous float32 CUDA tensor (h, w, 4) or (n, h, w, 4)"),
        (lambda: r.accumulate(u, [u], img, aov, out=f(2, 3, 4)),
         "out must be a contiguous float32 CUDA tensor of color's shape"),
        (lambda: r.accumulate(u, [u], img, aov, prev=(f(2, 3, 4), aov, u)),
         f"prev's colour must be a contiguous float32 tensor of shape (2, 3, 4) on {dev}"),
        (lambda: r.accumulate_var(u, [u], img, aov, f(2, 3)),
         f"vmean must be a contiguous float32 tensor of shape (2, 3) on {dev}"),
        (lambda: r.accumulate_var(u, [u], img, aov, _gpu(f(2, 3)), prev=(img, aov, u, f(2, 3))),
         f"prev's variance must be a contiguous float32 tensor of shape (2, 3) on {dev}"),
        (lambda: r.blend_pixels(f(2, 3, 4), px, _gpu(f(5, 4)), 1.0),
         "image must be a contiguous float32 (h, w, 4) CUDA tensor"),
        (lambda: r.blend_pixels(img, px, f(5, 4), 1.0), f"extra must be a contiguous float32 (5, 4) tensor on {dev}"),
        (lambda: r.blend_pixels_var(img, f(2, 3), px, _gpu(f(5, 4)), _gpu(f(5)), 1.0),
         f"var must be a contiguous float32 (2, 3) tensor on {dev}"),
        (lambda: r.blend_pixels_var(img, _gpu(f(2, 3)), px, _gpu(f(5, 4)), f(5), 1.0),
         f"extra_vmean must be a contiguous float32 (5,) tensor on {dev}"),
    ]
    for call, text in cases:
        with pytest.raises(ValueError, match=re.escape(text)):
            call()
    assert L.calls == []
