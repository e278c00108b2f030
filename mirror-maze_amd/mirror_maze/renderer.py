"""Renderer: the reference's compute dispatch as a Python object over the C ABI.

Method names follow the reference's operator interface:
  * ``upload_scene``   — make_buf for buffers 1, 2, 3, 5, 6 (src/main.rs:725-730)
  * ``compute_shader`` — copy_to_buf(chunks) + dispatch_thread_groups
                         (src/main.rs:778-885, kernel src/shaders.metal:245-368)
  * ``read_texture``   — the screen texture the dispatch writes
  * ``trace_tile``     — the offline renderer's throughput entry point

Device buffers for ``trace_tile`` are torch tensors on the GPU (torch is the
device-memory/stream plumbing); the library enqueues on torch's current
stream so ordering with torch ops (e.g. an RCCL gather) is preserved.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _args, _lib
from ._args import tensor_ok
from ._lib import check, lib
from .sampling import (_select_noisy_frames, merge_at, merge_samples, select_holes, select_holes_frames,  # noqa: F401
                       select_noisy, select_noisy_frames, select_short_history)
from .scene import Scene


def _ptr(t, n=1):
    """A tensor's address for a C call: None for no tensor, and for the tensors of an empty list (n = 0)."""
    return t.data_ptr() if t is not None and n else None


class Renderer:
    def __init__(self, device: int = 0):
        self._ctx = C.c_void_p()
        check(lib().mm_create(device, C.byref(self._ctx)))
        self.device = device
        self._view = None
        self._pinned_stream = False

    # -- lifecycle --------------------------------------------------------
    def close(self) -> None:
        if self._ctx:
            lib().mm_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int) -> None:
        check(rc, self._ctx)

    def set_stream(self, stream=None) -> None:
        """Pin a torch.cuda.Stream (or raw hipStream_t int).  None = follow
        torch's current stream at every trace_tile call (the default)."""
        self._pinned_stream = stream is not None
        handle = _lib.MM_OWN_STREAM if stream is None else int(getattr(stream, "cuda_stream", stream))
        self._check(lib().mm_set_stream(self._ctx, handle))

    def _follow(self, device) -> None:
        """Before a call that enqueues: unless a stream is pinned, take torch's current stream of `device`, so the
        call is ordered with the torch ops that made or will read its tensors."""
        if not self._pinned_stream:
            import torch

            self._check(lib().mm_set_stream(self._ctx, torch.cuda.current_stream(device).cuda_stream))

    def own_stream(self):
        """Pin the context's own (library-created, non-blocking) stream and
        return it as a torch.cuda.ExternalStream, so torch ops can be ordered
        with this context's work.  Two contexts on their own streams run
        independent frames concurrently (the next frame's blocks fill the
        CUs the previous frame's tail leaves idle)."""
        import torch

        self.set_stream(_lib.MM_OWN_STREAM)
        h = C.c_void_p()
        self._check(lib().mm_get_stream(self._ctx, C.byref(h)))
        return torch.cuda.ExternalStream(h.value, device=torch.device(f"cuda:{self.device}"))

    def set_wave_timeline(self, buf=None) -> None:
        """Diagnostics: per-wave (entry, staged, exit, chunks) u64 records of
        the wave-persistent kernel into an int64 CUDA tensor of shape
        (n_waves, 4); None turns recording off."""
        if buf is None:
            self._check(lib().mm_set_wave_timeline(self._ctx, None, 0))
        else:
            self._check(lib().mm_set_wave_timeline(self._ctx, buf.data_ptr(), buf.shape[0]))

    def set_pipeline(self, pipe: int) -> None:
        self._check(lib().mm_set_pipeline(self._ctx, pipe))

    def set_option(self, key: int, value: int) -> None:
        self._check(lib().mm_set_option(self._ctx, key, value))

    def scene_info(self, key: int) -> float:
        """mm_scene_info: facts about the uploaded scene's search structures
        (MM_INFO_*: grid availability and size, BVH depth)."""
        v = C.c_double()
        self._check(lib().mm_scene_info(self._ctx, key, C.byref(v)))
        return v.value

    # -- scene ------------------------------------------------------------
    def upload_scene(self, s: Scene) -> None:
        rects = np.ascontiguousarray(s.rects, dtype=np.float32)
        nodes = np.ascontiguousarray(s.nodes)
        idx = np.ascontiguousarray(s.idx, dtype=np.uint32)
        mats = np.ascontiguousarray(s.is_mirror, dtype=np.uint8)
        emis = np.ascontiguousarray(s.emission, dtype=np.float32)
        self._check(lib().mm_upload_scene(self._ctx, rects.ctypes.data, rects.shape[0], nodes.ctypes.data,
                                          nodes.shape[0], idx.ctypes.data, mats.ctypes.data, emis.ctypes.data))

    # -- parity mode --------------------------------------------------------
    def compute_shader(self, uniform: _lib.mm_uniform, pixel_update_buffer: np.ndarray) -> None:
        """One reference dispatch: (W/32)x(H/32) groups, 64 samples per pixel."""
        chunks = np.ascontiguousarray(pixel_update_buffer, dtype=np.uint32).reshape(-1, 2)
        self._check(lib().mm_trace_chunks(self._ctx, C.byref(uniform), chunks.ctypes.data, chunks.shape[0]))
        self._view = (int(uniform.view_w), int(uniform.view_h))

    def read_texture(self):
        """(rgba_f32 [H,W,4], rgba8 [H,W,4]) of the screen texture."""
        if self._view is None:
            raise RuntimeError("nothing rendered yet")
        W, H = self._view
        f = np.zeros((H, W, 4), dtype=np.float32)
        b = np.zeros((H, W, 4), dtype=np.uint8)
        self._check(lib().mm_read_framebuffer(self._ctx, f.ctypes.data, b.ctypes.data))
        return f, b

    def present(self) -> None:
        """One presentation step: the fragment_shader blur of the RGBA8 texture
        as a Jacobi step (src/shaders.metal:214-225; mm_present)."""
        self._check(lib().mm_present(self._ctx))

    def read_packets(self, n_chunks: int) -> np.ndarray:
        """(n_chunks, 16, 4) float32 packets of the last compute_shader: rgb and
        bitcast(x << 16 | y) (the shaders.air revision's pixel_data output)."""
        out = np.zeros((n_chunks, 16, 4), dtype=np.float32)
        self._check(lib().mm_read_packets(self._ctx, out.ctypes.data, n_chunks))
        return out

    def quantize(self, rgba, out=None):
        """RGBA8 (uint8 CUDA tensor, same shape; into `out` if given) of a float32
        RGBA CUDA tensor, with the texture-write conversion (mm_quantize_rgba8)."""
        import torch

        if not tensor_ok(rgba, torch.float32, ((..., 4),)):
            raise ValueError("rgba must be a contiguous float32 CUDA tensor [..., 4]")
        if out is None:
            out = torch.empty(rgba.shape, dtype=torch.uint8, device=rgba.device)
        elif not tensor_ok(out, torch.uint8, (rgba.shape,)):
            raise ValueError("out must be a contiguous uint8 CUDA tensor of rgba's shape")
        self._follow(rgba.device)
        self._check(lib().mm_quantize_rgba8(self._ctx, rgba.data_ptr(), out.data_ptr(), rgba.numel() // 4))
        return out

    # -- throughput mode ------------------------------------------------------
    @staticmethod
    def _out(out, shape, rgba8, device):
        """The output tensor: float32 (..., 4), or uint8 (..., 4) for RGBA8
        frames (MM_EXT_RGBA8, set when `out` is uint8 or rgba8=True)."""
        import torch

        if out is None:
            out = torch.zeros(shape, dtype=torch.uint8 if rgba8 else torch.float32, device=device)
        n = 1
        for d in shape:
            n *= d
        if not tensor_ok(out, (torch.float32, torch.uint8), numel=n):
            raise ValueError(f"out must be a contiguous float32 or uint8 CUDA tensor of {n} elements")
        return out, out.dtype == torch.uint8

    def _trace(self, call, ext, stats, r8, *outs):
        """The shared end of the trace calls: `call`, the method's own C entry point, is given the references of
        the call's ext (the caller's with the flags `stats` and `r8` ask for) and of a mm_stats.  Returns (*outs,
        mm_stats or None)."""
        st = _lib.mm_stats()
        self._check(call(C.byref(_args.call_ext(ext, stats, r8)), C.byref(st)))
        return (*outs, st if stats else None)

    def trace_tile(self, uniform: _lib.mm_uniform, ext: _lib.mm_ext, x0: int, y0: int, w: int, h: int,
                   y_stride: int = 1, out=None, stats: bool = False, rgba8: bool = False):
        """Render a tile into a (h, w, 4) float32 CUDA tensor (allocated if None),
        or with rgba8 / a uint8 `out` its RGBA8 texture-write conversion
        (MM_EXT_RGBA8: equal to quantize() of the float tile).  Returns (out,
        mm_stats or None)."""
        out, r8 = self._out(out, (h, w, 4), rgba8, f"cuda:{self.device}")
        self._follow(out.device)
        return self._trace(lambda e, st: lib().mm_trace_tile(self._ctx, C.byref(uniform), e, x0, y0, w, h, y_stride,
                                                             out.data_ptr(), st), ext, stats, r8, out)

    def trace_tile_frames(self, uniform: _lib.mm_uniform, ext: _lib.mm_ext, n_frames: int, x0: int, y0: int,
                          w: int, h: int, y_stride: int = 1, out=None, stats: bool = False, rgba8: bool = False):
        """Render frames ext.frame .. ext.frame + n_frames - 1 of a tile in ONE
        launch (mm_trace_tile_frames) into a (n_frames, h, w, 4) float32 CUDA
        tensor (allocated if None; uint8 RGBA8 with rgba8 / a uint8 `out`, as
        trace_tile); frame f equals trace_tile with frame ext.frame + f.
        Returns (out, mm_stats summed over the frames or None)."""
        out, r8 = self._out(out, (n_frames, h, w, 4), rgba8, f"cuda:{self.device}")
        self._follow(out.device)
        return self._trace(lambda e, st: lib().mm_trace_tile_frames(self._ctx, C.byref(uniform), e, n_frames, x0, y0,
                                                                    w, h, y_stride, out.data_ptr(), st),
                           ext, stats, r8, out)

    _cameras = staticmethod(_args.cameras)

    def trace_tile_cameras(self, uniform: _lib.mm_uniform, cameras, ext: _lib.mm_ext, x0: int, y0: int,
                           w: int, h: int, y_stride: int = 1, out=None, stats: bool = False, rgba8: bool = False):
        """Render a moving-camera sequence of a tile in ONE launch
        (mm_trace_tile_cameras): frame f with cameras[f] and RNG frame ext.frame
        + f, into a (n_frames, h, w, 4) float32 CUDA tensor (allocated if None;
        uint8 RGBA8 with rgba8 / a uint8 `out`, as trace_tile).  `cameras`: a
        sequence of mm_camera or mm_uniform (its .cam), or an (n, 10) float32
        array such as scene.walk_cameras returns; view size and chunk_w come
        from `uniform`, its .cam is ignored.  Frame f equals trace_tile with
        uniform.cam = cameras[f] and frame ext.frame + f.  Returns (out,
        mm_stats summed over the frames or None)."""
        cams = self._cameras(cameras)
        n = cams.shape[0]
        out, r8 = self._out(out, (n, h, w, 4), rgba8, f"cuda:{self.device}")
        self._follow(out.device)
        return self._trace(lambda e, st: lib().mm_trace_tile_cameras(self._ctx, C.byref(uniform),
                                                                     cams.ctypes.data if n else None, e, n, x0, y0,
                                                                     w, h, y_stride, out.data_ptr(), st),
                           ext, stats, r8, out)

    # -- closest-hit answers -------------------------------------------------
    def query_rays(self, rays, out=None):
        """Closest hit of each of n caller-supplied rays (mm_query_rays).
        `rays`: (n, 2, 4) float32 CUDA tensor or array, ray i = (origin xyz, -),
        (direction xyz, -).  Returns (t, k): float32 and int32 views of an
        (n, 2) int32 CUDA tensor (`out` if given) -- the reference walk's
        answer, k's bits those of the uint32 rect index, MM_AOV_ID_MISS
        (t = 1e30) where nothing is hit."""
        import torch

        dev = torch.device(f"cuda:{self.device}")
        if not torch.is_tensor(rays):
            rays = torch.from_numpy(np.ascontiguousarray(rays, dtype=np.float32)).to(dev)
        if not tensor_ok(rays, torch.float32, ((None, 2, 4),)):
            raise ValueError("rays must be a contiguous float32 (n, 2, 4) CUDA tensor or array")
        n = rays.shape[0]
        if out is None:
            out = torch.empty((n, 2), dtype=torch.int32, device=rays.device)
        elif not tensor_ok(out, torch.int32, ((n, 2),)):
            raise ValueError("out must be a contiguous int32 (n, 2) CUDA tensor")
        self._follow(rays.device)
        self._check(lib().mm_query_rays(self._ctx, _ptr(rays, n), n, _ptr(out, n)))
        return out[:, 0].view(torch.float32), out[:, 1]

    AOV_NAMES = ("normal_depth", "albedo", "id")

    def trace_aov(self, uniform: _lib.mm_uniform, cameras=None, mirror_limit: int = 15, *, x0: int, y0: int,
                  w: int, h: int, y_stride: int = 1, want=AOV_NAMES, out=None):
        """Per-pixel feature buffers of a tile (mm_trace_aov): the pixel-centre
        ray followed through the mirror chain to the first surface that shades
        diffusely.  `cameras`: None (uniform.cam, one frame) or what
        trace_tile_cameras takes (one frame per camera, one launch).  Returns a
        dict of the buffers named in `want`, CUDA tensors (taken from the dict
        `out` where it has them):
          normal_depth  (n_frames, h, w, 4) float32: outward normal, distance
          albedo        (n_frames, h, w, 4) float32: rect colour, mirror hits
          id            (n_frames, h, w)    int32:   rect | MM_AOV_ID_* bits"""
        import torch

        want = tuple(want)
        if not want or any(k not in self.AOV_NAMES for k in want):
            raise ValueError(f"want must name some of {self.AOV_NAMES}")
        cams = None if cameras is None else self._cameras(cameras)
        n = 1 if cams is None else cams.shape[0]
        dev = torch.device(f"cuda:{self.device}")
        bufs = {}
        for k in want:
            shape, dt = ((n, h, w), torch.int32) if k == "id" else ((n, h, w, 4), torch.float32)
            t = (out or {}).get(k)
            if t is None:
                t = torch.empty(shape, dtype=dt, device=dev)
            elif not tensor_ok(t, dt, (shape,)):
                raise ValueError(f"out[{k!r}] must be a contiguous {dt} CUDA tensor of shape {shape}")
            bufs[k] = t
        self._follow(dev)
        a = _lib.mm_aov(*[bufs[k].data_ptr() if k in bufs else None for k in self.AOV_NAMES])
        self._check(lib().mm_trace_aov(self._ctx, C.byref(uniform), None if cams is None else
                                       (cams.ctypes.data if n else None), n, mirror_limit, x0, y0, w, h, y_stride,
                                       C.byref(a)))
        return bufs

    def denoise(self, color, aov, n_passes: int = 4, sigma_z: float = 0.02, sigma_l: float = 0.5,
                rgba8: bool = False, out=None):
        """Edge-aware a-trous denoise of traced frames (mm_denoise_frames).
        `color`: an (h, w, 4) or (n, h, w, 4) float32 CUDA tensor, what
        trace_tile / trace_tile_frames / trace_tile_cameras return; `aov`: the
        dict trace_aov returns for the same tile and cameras (all three
        buffers).  Pass i spaces its 5x5 taps 2^i apart; a tap counts only
        where it shows the centre's surface, weighed by a depth term (sigma_z)
        and a luminance term (sigma_l, halved every pass); a sigma <= 0 turns
        its term off.  Returns a float32 tensor of color's shape (`out` if
        given), or with rgba8 / a uint8 `out` its RGBA8 conversion (equal to
        quantize() of the float result).  The inputs are not written."""
        import torch

        n, h, w = self._frames(color)
        a = self._aov_frames(aov, n, h, w, color.device, "aov")
        if not 1 <= int(n_passes) <= _lib.MM_DENOISE_MAX_PASSES:
            raise ValueError(f"n_passes must be 1..{_lib.MM_DENOISE_MAX_PASSES}")
        out = self._filter_out(out, color.shape, color.device, rgba8,
                               "out must be a contiguous float32 (uint8 for RGBA8) CUDA tensor of color's shape")
        r8 = out.dtype == torch.uint8
        self._follow(color.device)
        p = _lib.mm_denoise_params(int(n_passes), float(sigma_z), float(sigma_l), _lib.MM_DN_RGBA8 if r8 else 0)
        self._check(lib().mm_denoise_frames(self._ctx, color.data_ptr(), C.byref(a), C.byref(p), n, w, h,
                                            out.data_ptr()))
        return out

    def denoise_var(self, color, aov, var, count, n_passes: int = 4, sigma_z: float = 0.02, sigma_l: float = 8.0,
                    eps_l: float = 1e-2, rgba8: bool = False, out=None, var_out=None, return_var: bool = False):
        """Variance-guided a-trous denoise (mm_denoise_frames_var): denoise()
        with the luminance stop of every pixel at sigma_l standard deviations
        of the pixel mean (from a 3x3 of the variance around it) plus eps_l,
        not halved per pass.  `color`, `aov`, `rgba8`, `out`: as in denoise().
        `var`: an (h, w) or (n, h, w) float32 CUDA tensor, the variance of ONE
        sample's luminance, what trace_tile_var returns or refine() keeps;
        `count`: the samples each pixel holds, a number or a tensor of var's
        shape.  The filter takes var / count, formed here.  Returns `out`, or
        with return_var or a `var_out` tensor (float32, var's shape) the pair
        (out, var_out): the variance of the filtered mean's luminance, the taps
        taken as independent.  The defaults are from the sweep in
        profiles/denoise_var/quality.txt.  The inputs are not written.  (var / count is a
        torch operation on torch's current stream: with a pinned stream, call
        this under that stream, as refine().)"""
        import torch

        n, h, w = self._frames(color)
        lead = tuple(color.shape[:-1])
        a = self._aov_frames(aov, n, h, w, color.device, "aov")
        if not tensor_ok(var, torch.float32, (lead, (n, h, w), (h, w)) if n == 1 else (lead,), device=color.device,
                         contiguous=False):
            raise ValueError(f"var must be a float32 tensor of shape {lead} on {color.device}")
        if torch.is_tensor(count):
            if not (count.device == color.device and tuple(count.shape) == tuple(var.shape)):
                raise ValueError("count must be a number or a tensor of var's shape on its device")
        elif not float(count) > 0:
            raise ValueError("count must be positive")
        if not 1 <= int(n_passes) <= _lib.MM_DENOISE_MAX_PASSES:
            raise ValueError(f"n_passes must be 1..{_lib.MM_DENOISE_MAX_PASSES}")
        out = self._filter_out(out, color.shape, color.device, rgba8,
                               "out must be a contiguous float32 (uint8 for RGBA8) CUDA tensor of color's shape")
        if var_out is not None or return_var:
            var_out = self._filter_out(var_out, var.shape, color.device, None,
                                       "var_out must be a contiguous float32 CUDA tensor of var's shape")
        r8 = out.dtype == torch.uint8
        self._follow(color.device)
        vmean = (var / count).to(torch.float32).contiguous()  # bookkeeping, as merge_samples is
        p = _lib.mm_denoise_var_params(int(n_passes), float(sigma_z), float(sigma_l), float(eps_l),
                                       _lib.MM_DNV_RGBA8 if r8 else 0, 0)
        self._check(lib().mm_denoise_frames_var(self._ctx, color.data_ptr(), C.byref(a), vmean.data_ptr(),
                                                C.byref(p), n, w, h, out.data_ptr(), _ptr(var_out)))
        return out if var_out is None else (out, var_out)

    @staticmethod
    def _frames(color):
        """(n, h, w) of a colour tensor, (h, w, 4) or (n, h, w, 4)."""
        import torch

        if not tensor_ok(color, torch.float32, ((None, None, 4), (None, None, None, 4))):
            raise ValueError("color must be a contiguous float32 CUDA tensor (h, w, 4) or (n, h, w, 4)")
        return (1 if color.dim() == 3 else color.shape[0]), *color.shape[-3:-1]

    _PLANE = "{what} must be a contiguous float32 tensor of shape {shape} on {device}"
    _ENTRIES = "{what} must be a contiguous float32 {shape} tensor on {device}"  # (the pixel-list methods' wording)

    @staticmethod
    def _plane(t, what, shape, device, wording=_PLANE):
        """`t`, a contiguous float32 tensor of `shape` on `device`."""
        import torch

        if not tensor_ok(t, torch.float32, (shape,), device=device):
            raise ValueError(wording.format(what=what, shape=shape, device=device))
        return t

    @staticmethod
    def _filter_out(out, shape, device, rgba8, msg):
        """A filter's output of `shape`: `out` if it fits (else ValueError(msg)), or a new tensor.  rgba8 None: float32;
        else uint8 is allowed too, and it is what rgba8 asks for."""
        import torch

        if out is None:
            return torch.empty(shape, dtype=torch.uint8 if rgba8 else torch.float32, device=device)
        dtypes = torch.float32 if rgba8 is None else torch.uint8 if rgba8 else (torch.float32, torch.uint8)
        if not tensor_ok(out, dtypes, (shape,), device=device):
            raise ValueError(msg)
        return out

    def _prev(self, prev, h, w, device, var):
        """The mm_temporal_prev of accumulate()'s `prev` triple -- var: the mm_temporal_prev_var of accumulate_var()'s
        quadruple -- for an h x w window on `device`."""
        import torch

        if var:
            pc, pa, pcam, pvar = prev
        else:
            pc, pa, pcam = prev
        if not tensor_ok(pc, torch.float32, ((h, w, 4), (1, h, w, 4)), device=device):
            raise ValueError(f"prev's colour must be a contiguous float32 tensor of shape {(h, w, 4)} on {device}")
        if var and not tensor_ok(pvar, torch.float32, ((h, w), (1, h, w)), device=device):
            if torch.is_tensor(pvar) and tuple(pvar.shape) in ((h, w), (1, h, w)):  # (its shape is not what is wrong)
                self._plane(pvar, "prev's variance", tuple(pvar.shape), device)
            raise ValueError(f"prev's variance must be a float32 tensor of shape {(h, w)} on {device}")
        pcam = _args.camera(pcam)
        fields = (pc.data_ptr(), self._aov_frames(pa, 1, h, w, device, "prev's aov"), pcam)
        return _lib.mm_temporal_prev_var(*fields, pvar.data_ptr()) if var else _lib.mm_temporal_prev(*fields)

    @staticmethod
    def _window(image):
        """(h, w) of an accumulated frame, (h, w, 4)."""
        import torch

        if not tensor_ok(image, torch.float32, ((None, None, 4),)):
            raise ValueError("image must be a contiguous float32 (h, w, 4) CUDA tensor")
        return tuple(image.shape[:2])

    def _aov_frames(self, aov, n, h, w, device, what):
        """The mm_aov of an aov dict whose buffers hold n frames of h x w on `device`."""
        import torch

        if not (isinstance(aov, dict) and all(k in aov for k in self.AOV_NAMES)):
            raise ValueError(f"{what} must hold the buffers {self.AOV_NAMES} of trace_aov")
        for k in self.AOV_NAMES:
            shape, dt = ((n, h, w), torch.int32) if k == "id" else ((n, h, w, 4), torch.float32)
            t = aov[k]
            if not tensor_ok(t, dt, (shape, shape[1:]) if n == 1 else (shape,), device=device):
                raise ValueError(f"{what}[{k!r}] must be a contiguous {dt} tensor of shape {shape} on {device}")
        return _lib.mm_aov(*[aov[k].data_ptr() for k in self.AOV_NAMES])

    def accumulate(self, uniform: _lib.mm_uniform, cameras, color, aov, prev=None, n_max: int = 32,
                   tol_z: float = 0.02, w_min: float = 0.25, x0: int = 0, y0: int = 0, out=None):
        """Temporal accumulation of a camera sequence (mm_accumulate_frames).
        `color`: the (h, w, 4) or (n, h, w, 4) float32 CUDA tensor
        trace_tile_cameras returned for `cameras` over the window (x0, y0, w,
        h) of uniform's view with y_stride 1; `aov`: what trace_aov returned
        for the same window and cameras (all three buffers).  Every pixel's
        surface point -- its virtual image, when it is seen through mirrors --
        is projected into the frame before; where the pixels there show the
        same point through the same mirrors (id, mirror hits, normal, distance
        within tol_z; valid bilinear weight at least w_min) the output is the
        running mean of up to n_max frames, elsewhere the frame itself.  The
        frame before frame 0 is `prev`, a (color, aov, camera) triple: an
        earlier call's last output frame, that frame's guides and its camera;
        None starts a new history.  Returns a float32 tensor of color's shape
        (`out` if given) whose alpha is the history length; it feeds denoise()
        unchanged.  The inputs are not written."""
        n, h, w = self._frames(color)
        cams = self._cameras(cameras)
        if cams.shape[0] != n:
            raise ValueError(f"{n} frames need {n} cameras, not {cams.shape[0]}")
        a = self._aov_frames(aov, n, h, w, color.device, "aov")
        if not 1 <= int(n_max) <= 65535:
            raise ValueError("n_max must be 1..65535")
        out = self._filter_out(out, color.shape, color.device, None,
                               "out must be a contiguous float32 CUDA tensor of color's shape")
        pv = None if prev is None else self._prev(prev, h, w, color.device, False)
        self._follow(color.device)
        p = _lib.mm_temporal_params(int(n_max), float(tol_z), float(w_min), 0)
        self._check(lib().mm_accumulate_frames(self._ctx, C.byref(uniform), cams.ctypes.data, color.data_ptr(),
                                               C.byref(a), None if pv is None else C.byref(pv), C.byref(p), n, x0, y0,
                                               w, h, out.data_ptr()))
        return out

    def accumulate_var(self, uniform: _lib.mm_uniform, cameras, color, aov, vmean, weight=None, prev=None,
                       n_max: int = 32, tol_z: float = 0.02, w_min: float = 0.25, x0: int = 0, y0: int = 0, out=None,
                       var_out=None):
        """accumulate() with the variance of the pixel mean carried through the
        history (mm_accumulate_frames_var).  `color`, `cameras`, `aov`, the
        parameters and the window: as in accumulate().  `vmean`: a float32 CUDA
        tensor of color's shape without the last axis, the variance of each
        frame's pixel-MEAN luminance (trace_tile_var's var / the samples the
        pixel holds).  `weight`: None, or a tensor of vmean's shape, the frame's
        weight per pixel in frames (samples held / frame spp, e.g. count /
        ext.spp after refine()); None is 1 everywhere, and the colours are then
        accumulate()'s bit for bit.  `prev` is a (color, aov, camera, var)
        quadruple: an earlier call's last output frame, that frame's guides, its
        camera and its var_out.  Returns (out, var_out): the accumulated frames
        (alpha = history length in frames) and the variance of their luminance,
        the taps taken as independent; var_out feeds denoise_var() with count 1
        and select_noisy() with count 1.  The inputs are not written."""
        import torch

        n, h, w = self._frames(color)
        lead = tuple(color.shape[:-1])
        cams = self._cameras(cameras)
        if cams.shape[0] != n:
            raise ValueError(f"{n} frames need {n} cameras, not {cams.shape[0]}")
        a = self._aov_frames(aov, n, h, w, color.device, "aov")
        if not 1 <= int(n_max) <= 65535:
            raise ValueError("n_max must be 1..65535")
        self._plane(vmean, "vmean", lead, color.device)
        if weight is not None:
            self._plane(weight, "weight", lead, color.device)
        out = self._filter_out(out, color.shape, color.device, None,
                               "out must be a contiguous float32 CUDA tensor of color's shape")
        if var_out is None:
            var_out = torch.empty(lead, dtype=torch.float32, device=color.device)
        else:
            self._plane(var_out, "var_out", lead, color.device)
        pv = None if prev is None else self._prev(prev, h, w, color.device, True)
        self._follow(color.device)
        p = _lib.mm_temporal_params(int(n_max), float(tol_z), float(w_min), 0)
        self._check(lib().mm_accumulate_frames_var(self._ctx, C.byref(uniform), cams.ctypes.data, color.data_ptr(),
                                                   C.byref(a), vmean.data_ptr(), _ptr(weight),
                                                   None if pv is None else C.byref(pv), C.byref(p), n, x0, y0, w, h,
                                                   out.data_ptr(), var_out.data_ptr()))
        return out, var_out

    # -- pixel lists -----------------------------------------------------------
    def _pixel_list(self, pixels):
        """The (n, 2) int32 CUDA tensor of a pixel list: `pixels` itself, or an
        upload of an (n, 2) array of (x, y) pairs to this renderer's device."""
        return _args.pixel_list(pixels, f"cuda:{self.device}")

    def trace_pixels(self, uniform: _lib.mm_uniform, ext: _lib.mm_ext, pixels, out=None, stats: bool = False,
                     rgba8: bool = False):
        """Trace a list of pixels (mm_trace_pixels).  `pixels`: an (n, 2) int32 /
        uint32 CUDA tensor of (x, y) view coordinates, or an array that is
        uploaded.  Entry e of the (n, 4) float32 result (`out` if given; uint8
        RGBA8 with rgba8 / a uint8 `out`, as trace_tile) equals pixel (x, y) of
        trace_tile with the same uniform and ext, bit for bit; an entry outside
        the view gets zeros.  Returns (out, mm_stats or None)."""
        pixels = self._pixel_list(pixels)
        n = pixels.shape[0]
        out, r8 = self._out(out, (n, 4), rgba8, pixels.device)
        self._follow(out.device)
        return self._trace(lambda e, st: lib().mm_trace_pixels(self._ctx, C.byref(uniform), e, _ptr(pixels, n), n,
                                                               _ptr(out, n), st), ext, stats, r8, out)

    def trace_rays(self, ext: _lib.mm_ext, rays, jitter: bool = False, out=None, var=None, stats: bool = False,
                   rgba8: bool = False):
        """Shaded radiance along n caller-supplied rays (mm_trace_rays).  `rays`:
        an (n, 8) float32 CUDA tensor, ray i = (origin xyz, RNG key bits,
        direction xyz, -), as rays.pack_rays builds it.  Entry e of the (n, 4)
        float32 result (`out` if given; uint8 RGBA8 with rgba8 / a uint8 `out`,
        as trace_tile) is the mean of ext.spp paths from the ray; jitter: the
        primary ray's jitter on the direction (MM_RAYS_JITTER).  `var`: True,
        or an (n,) float32 CUDA tensor, for each entry's sample variance as
        trace_pixels_var defines it.  Returns (out, mm_stats or None), or
        (out, var, mm_stats or None) with `var`."""
        import torch

        rays = _args.ray_list(rays)
        n = rays.shape[0]
        out, r8 = self._out(out, (n, 4), rgba8, rays.device)
        if var is True:
            var = torch.zeros((n,), dtype=torch.float32, device=rays.device)
        elif var is False:
            var = None
        if var is not None and not tensor_ok(var, torch.float32, ((n,),)):
            raise ValueError(f"var must be a contiguous float32 CUDA tensor of {n} elements")
        self._follow(out.device)
        flags = _lib.MM_RAYS_JITTER if jitter else 0
        outs = (out,) if var is None else (out, var)
        return self._trace(lambda e, st: lib().mm_trace_rays(self._ctx, e, flags, _ptr(rays, n), n, _ptr(out, n),
                                                             None if var is None else _ptr(var, n), st),
                           ext, stats, r8, *outs)

    def blend_pixels(self, image, pixels, extra, m: float, x0: int = 0, y0: int = 0):
        """Blend extra samples into an accumulated frame, in place
        (mm_blend_pixels).  `image`: the (h, w, 4) float32 CUDA tensor of the
        window (x0, y0, w, h) whose alpha is the history length, as accumulate
        returns it; `pixels`, `extra`: a pixel list and what trace_pixels
        returned for it; `m`: the weight of the extra samples in frames (extra
        spp / frame spp).  Entries outside the window are skipped; the list
        must not name a window pixel twice.  Returns `image`."""
        h, w = self._window(image)
        pixels = self._pixel_list(pixels)
        n = pixels.shape[0]
        self._plane(extra, "extra", (n, 4), image.device, self._ENTRIES)
        self._follow(image.device)
        self._check(lib().mm_blend_pixels(self._ctx, image.data_ptr(), x0, y0, w, h, _ptr(pixels, n), _ptr(extra, n),
                                          n, float(m)))
        return image

    def top_up(self, uniform: _lib.mm_uniform, camera, ext: _lib.mm_ext, acc, aov, n_min: float, extra_spp: int,
               frame_key: int, x0: int = 0, y0: int = 0):
        """Spend extra samples where an accumulated frame's history is short.
        `acc`: ONE (h, w, 4) frame accumulate returned for the window (x0, y0,
        w, h), traced with `camera` and `ext`; `aov`: that frame's guides (its
        "id" buffer, (h, w) or (1, h, w)).  The pixels with history length
        acc[..., 3] < n_min whose id is neither MM_AOV_ID_MISS nor
        MM_AOV_ID_FAILED (those never get a history) are traced with extra_spp
        samples each and blended into `acc` with weight extra_spp / ext.spp, in
        place, in row-major order.  The extra samples are drawn with RNG frame
        `frame_key`: pick a key outside the sequence's frame numbers, e.g.
        2**20 + f for frame f, so that they are independent of every frame's
        own samples.  Returns (acc, n_selected); nothing is launched when no
        pixel is selected."""
        ids = aov["id"] if isinstance(aov, dict) else aov
        pixels = select_short_history(acc, ids, n_min, x0, y0)
        n = int(pixels.shape[0])
        if n == 0:
            return acc, 0
        u = _lib.mm_uniform.from_buffer_copy(bytes(uniform))
        u.cam = _args.camera(camera)
        e = _args.extra_ext(ext, extra_spp, frame_key)
        extra, _ = self.trace_pixels(u, e, pixels)
        self.blend_pixels(acc, pixels, extra, extra_spp / ext.spp, x0, y0)
        return acc, n

    def blend_pixels_var(self, image, var, pixels, extra, extra_vmean, m: float, x0: int = 0, y0: int = 0):
        """blend_pixels() with the variance image beside the colour, both in
        place (mm_blend_pixels_var).  `image`, `pixels`, `extra`, `m`, the
        window: as in blend_pixels(); `var`: the (h, w) float32 CUDA tensor
        accumulate_var returned beside `image`; `extra_vmean`: (n,) float32, the
        variance of each entry's extra MEAN (trace_pixels_var's var / extra
        spp).  The colours are blend_pixels()' bit for bit.  Returns (image,
        var)."""
        h, w = self._window(image)
        self._plane(var, "var", (h, w), image.device, self._ENTRIES)
        pixels = self._pixel_list(pixels)
        n = pixels.shape[0]
        self._plane(extra, "extra", (n, 4), image.device, self._ENTRIES)
        self._plane(extra_vmean, "extra_vmean", (n,), image.device, self._ENTRIES)
        self._follow(image.device)
        self._check(lib().mm_blend_pixels_var(self._ctx, image.data_ptr(), var.data_ptr(), x0, y0, w, h,
                                              _ptr(pixels, n), _ptr(extra, n), _ptr(extra_vmean, n), n, float(m)))
        return image, var

    def top_up_var(self, uniform: _lib.mm_uniform, camera, ext: _lib.mm_ext, acc, var, aov, extra_spp: int,
                   frame_key: int, n_min=None, rel_tol=None, x0: int = 0, y0: int = 0):
        """top_up() for a frame of accumulate_var: spend extra samples where the
        history is short, where the accumulated pixel is noisy, or both.
        `acc`, `var`: ONE (h, w, 4) frame and its (h, w) variance as
        accumulate_var returned them for the window (x0, y0, w, h), traced with
        `camera` and `ext`; `aov`: that frame's guides (its "id" buffer).  The
        selection is the union of select_short_history(acc, ids, n_min) and
        select_noisy(acc, var, 1.0, rel_tol, ids=ids) -- `var` is already the
        variance of the mean -- in row-major order; at least one of n_min and
        rel_tol must be given.  The selected pixels are traced with extra_spp
        (>= 2) samples each by trace_pixels_var (RNG frame `frame_key`, as in
        top_up()) and blended by blend_pixels_var with extra_vmean = the extra
        samples' variance / extra_spp and weight extra_spp / ext.spp, in place.
        Returns (acc, var, n_selected); nothing is launched for 0."""
        import torch

        if n_min is None and rel_tol is None:
            raise ValueError("top_up_var needs n_min, rel_tol or both")
        if acc.dim() != 3 or acc.shape[-1] != 4 or tuple(var.shape) != tuple(acc.shape[:2]):
            raise ValueError("acc must be one (h, w, 4) frame and var its (h, w) variance")
        ids = aov["id"] if isinstance(aov, dict) else aov
        lists = []
        if n_min is not None:
            lists.append(select_short_history(acc, ids, n_min, x0, y0))
        if rel_tol is not None:
            lists.append(select_noisy(acc, var, 1.0, rel_tol, ids=ids, x0=x0, y0=y0))
        pixels = lists[0]
        if len(lists) == 2:  # the union, row-major, each pixel once (x, y < 2^24)
            both = torch.cat(lists).long()
            key = torch.unique((both[:, 1] << 32) | both[:, 0])  # sorted
            pixels = torch.stack((key & 0xFFFFFFFF, key >> 32), dim=1).to(torch.int32).contiguous()
        n = int(pixels.shape[0])
        if n == 0:
            return acc, var, 0
        u = _lib.mm_uniform.from_buffer_copy(bytes(uniform))
        u.cam = _args.camera(camera)
        e = _args.extra_ext(ext, extra_spp, frame_key)
        extra, var_b, _ = self.trace_pixels_var(u, e, pixels)
        self.blend_pixels_var(acc, var, pixels, extra, (var_b / float(extra_spp)).contiguous(), extra_spp / ext.spp,
                              x0, y0)
        return acc, var, n

    # -- per-pixel sample variance ------------------------------------------------
    def trace_tile_var(self, uniform: _lib.mm_uniform, ext: _lib.mm_ext, x0: int, y0: int, w: int, h: int,
                       y_stride: int = 1, cameras=None, n_frames: int = 1, out=None, var=None, stats: bool = False,
                       rgba8: bool = False):
        """A tile and the sample variance of each pixel's luminance
        (mm_trace_tile_var).  `out` is what trace_tile (cameras None, n_frames
        1), trace_tile_frames (cameras None) or trace_tile_cameras would return,
        bit for bit: (h, w, 4), or (n_frames, h, w, 4) for a multi-frame call;
        `var` is a float32 CUDA tensor of that shape without the last axis, the
        unbiased variance of ONE sample's luminance (var / spp estimates the
        pixel mean's).  ext.spp must be at least 2; the samples are staged
        whatever MM_OPT_FUSE_RESOLVE says.  Returns (out, var, mm_stats or
        None)."""
        import torch

        cams = None if cameras is None else self._cameras(cameras)
        n = n_frames if cams is None else cams.shape[0]
        lead = (h, w) if cams is None and n_frames == 1 else (n, h, w)
        dev = f"cuda:{self.device}"
        out, r8 = self._out(out, (*lead, 4), rgba8, dev)
        if var is None:
            var = torch.zeros(lead, dtype=torch.float32, device=dev)
        if not tensor_ok(var, torch.float32, (lead,)):
            raise ValueError(f"var must be a contiguous float32 CUDA tensor of shape {lead}")
        self._follow(out.device)
        return self._trace(lambda e, st: lib().mm_trace_tile_var(self._ctx, C.byref(uniform),
                                                                 None if cams is None else cams.ctypes.data, e, n,
                                                                 x0, y0, w, h, y_stride, out.data_ptr(),
                                                                 var.data_ptr(), st), ext, stats, r8, out, var)

    def trace_pixels_var(self, uniform: _lib.mm_uniform, ext: _lib.mm_ext, pixels, out=None, var=None,
                         stats: bool = False, rgba8: bool = False):
        """A pixel list and each entry's sample variance (mm_trace_pixels_var):
        `out` as trace_pixels returns it, `var` an (n,) float32 CUDA tensor,
        entry e the variance trace_tile_var gives that pixel, bit for bit; an
        entry outside the view gets 0.  Returns (out, var, mm_stats or None)."""
        import torch

        pixels = self._pixel_list(pixels)
        n = pixels.shape[0]
        out, r8 = self._out(out, (n, 4), rgba8, pixels.device)
        if var is None:
            var = torch.zeros((n,), dtype=torch.float32, device=pixels.device)
        if not tensor_ok(var, torch.float32, ((n,),)):
            raise ValueError(f"var must be a contiguous float32 CUDA tensor of {n} elements")
        self._follow(out.device)
        return self._trace(lambda e, st: lib().mm_trace_pixels_var(self._ctx, C.byref(uniform), e, _ptr(pixels, n), n,
                                                                   _ptr(out, n), _ptr(var, n), st),
                           ext, stats, r8, out, var)

    def refine(self, uniform: _lib.mm_uniform, ext: _lib.mm_ext, color, var, count, rel_tol: float, extra_spp: int,
               frame_key: int, ids=None, x0: int = 0, y0: int = 0):
        """One round of noise-driven sampling, in place.  `color` (h, w, 4),
        `var` (h, w) and `count` (h, w) float32 CUDA tensors: the window (x0,
        y0, w, h) as trace_tile_var returned it for `uniform` (its camera is
        used) and the samples each pixel holds so far (ext.spp after the first
        frame).  The pixels select_noisy names -- standard error of the mean
        above rel_tol times the luminance; `ids`, a guides' id buffer, keeps
        MISS / FAILED pixels out -- are traced with extra_spp (>= 2) samples
        each by trace_pixels_var, and merge_samples pools both groups into
        color[..., :3], var and count of those pixels; every other pixel keeps
        its bits.  The extra samples are drawn with RNG frame `frame_key`: pick
        a key outside the sequence's frame numbers, e.g. 2**20 + 64 * f + round
        for round `round` of frame f, so that they are independent of every
        frame's own samples and of the other rounds'.  The caller loops with a
        new key per round until the return value, the number of pixels
        selected, is small enough; nothing is launched for 0."""
        pixels = select_noisy(color, var, count, rel_tol, ids=ids, x0=x0, y0=y0)
        n = int(pixels.shape[0])
        if n == 0:
            return 0
        mean_b, var_b, _ = self.trace_pixels_var(uniform, _args.extra_ext(ext, extra_spp, frame_key), pixels)
        merge_at(((pixels[:, 1] - y0).long(), (pixels[:, 0] - x0).long()), color, var, count, mean_b, var_b, extra_spp)
        return n

    # -- pixel lists of many frames in one launch -----------------------------------
    def trace_pixel_lists(self, uniform: _lib.mm_uniform, cameras, ext: _lib.mm_ext, pixels, offsets,
                          frame_keys=None, out=None, var=None, stats: bool = False, rgba8: bool = False):
        """The pixel lists of several frames in ONE launch
        (mm_trace_pixel_lists).  `pixels`: the lists back to back, as
        trace_pixels takes one; `offsets`: n_lists + 1 integers on the host,
        offsets[0] = 0 and non-decreasing -- list f is pixels[offsets[f] :
        offsets[f + 1]] and may be empty.  `cameras`: what trace_tile_cameras
        takes, one per list, or None for uniform.cam on every list;
        `frame_keys`: the lists' RNG frames, or None for ext.frame + f.  Entry
        e of the (n, 4) result equals trace_pixels' for it with its list's
        camera and frame, bit for bit.  `var`: None for the plain call, True
        or an (n,) float32 CUDA tensor for the variance call, whose (out, var)
        are trace_pixels_var's.  Returns (out, var or None, mm_stats or
        None)."""
        import torch

        pixels = self._pixel_list(pixels)
        n = pixels.shape[0]
        offs = _args.list_offsets(offsets, n)
        n_lists = offs.shape[0] - 1
        cams = None if cameras is None else self._cameras(cameras)
        if cams is not None and cams.shape[0] != n_lists:
            raise ValueError(f"{n_lists} lists need {n_lists} cameras, not {cams.shape[0]}")
        keys = _args.list_keys(frame_keys, n_lists)
        out, r8 = self._out(out, (n, 4), rgba8, pixels.device)
        if var is True:
            var = torch.zeros((n,), dtype=torch.float32, device=pixels.device)
        if var is not None and not tensor_ok(var, torch.float32, ((n,),)):
            raise ValueError(f"var must be None, True or a contiguous float32 CUDA tensor of {n} elements")
        self._follow(out.device)
        return self._trace(lambda e, st: lib().mm_trace_pixel_lists(
            self._ctx, C.byref(uniform), None if cams is None else cams.ctypes.data, e,
            None if keys is None else keys.ctypes.data, n_lists, _ptr(pixels, n), offs.ctypes.data, _ptr(out, n),
            _ptr(var, n), st), ext, stats, r8, out, var)

    def refine_frames(self, uniform: _lib.mm_uniform, cameras, ext: _lib.mm_ext, color, var, count, rel_tol: float,
                      extra_spp: int, frame_keys, ids=None, x0: int = 0, y0: int = 0):
        """One round of refine() for a whole batch of frames, in place, with one
        selection, one trace launch and one merge for all of them.  `color` (n,
        h, w, 4), `var` and `count` (n, h, w) float32 CUDA tensors: the window
        (x0, y0, w, h) of n frames as trace_tile_var(cameras=...) returned
        them, frame f traced with cameras[f]; `frame_keys`: n RNG frames, one
        per frame, new for every round (refine()'s rule); `ids`: the guides' id
        buffers, (n, h, w).  The result equals refine() called per frame with
        uniform.cam = cameras[f] and frame_keys[f], on all bits of colour,
        variance and count.  Returns the selected pixels per frame, a list of n
        ints; nothing is launched when no frame selects any."""
        pixels, offsets, fji = _select_noisy_frames(color, var, count, rel_tol, 1e-3, ids, x0, y0)
        counts = [int(b - a) for a, b in zip(offsets[:-1], offsets[1:])]
        if int(offsets[-1]) == 0:
            return counts
        e = _args.extra_ext(ext, extra_spp, ext.frame)  # (the lists' RNG frames are frame_keys)
        mean_b, var_b, _ = self.trace_pixel_lists(uniform, cameras, e, pixels, offsets, frame_keys, var=True)
        merge_at(fji.unbind(1), color, var, count, mean_b, var_b, extra_spp)
        return counts

    # -- tracing a lattice and rebuilding from the AOVs ---------------------------------
    def upsample(self, low, aov, scale: int, w_min: float = 0.25, low_vmean=None, want_weight: bool = True,
                 out=None):
        """Rebuild full-resolution frames from frames traced on the lattice of
        every scale-th pixel (mm_upsample_frames).  `low`: an (lh, lw, 4) or (n,
        lh, lw, 4) float32 CUDA tensor, lw = ceil(w / scale) and lh = ceil(h /
        scale): element (Y, X) is the traced value of window pixel (scale * X,
        scale * Y), what trace_tile* returns for the view (view_w / scale,
        view_h / scale) and the tile (x0 / scale, y0 / scale, lw, lh).  `aov`:
        the dict trace_aov returns for the full-resolution window (w, h) and the
        same cameras, all three buffers.  A pixel is interpolated from those of
        the four lattice pixels around it that show its surface through the same
        mirrors from the same side; where their bilinear weights sum to less
        than `w_min` (or the guides failed) it is a hole: zeros, weight 0.
        `low_vmean`: None, or the variance of the lattice pixels' MEAN luminance
        (trace_tile_var's var / spp), low's shape without the last axis.
        Returns (color, weight, var): color of the aov's frames' shape + (4,)
        (`out` if given), alpha 1; weight (None unless want_weight) the pixel's
        effective sample weight in frames, 1 at lattice pixels, up to 4 between
        them, 0 at holes -- accumulate_var's `weight` once the holes are filled;
        var (None without low_vmean) the variance of color's luminance, exact
        for the noise part.  `out`: None, or the float32 tensor the colour is
        written to (as denoise()'s).  The inputs are not written."""
        import torch

        n, lh, lw = self._frames(low)
        if int(scale) not in (2, 4, 8):
            raise ValueError("scale must be 2, 4 or 8")
        s = int(scale)
        ids = aov.get("id") if isinstance(aov, dict) else None
        if not torch.is_tensor(ids) or ids.dim() < 2:
            raise ValueError(f"aov must hold the buffers {self.AOV_NAMES} of trace_aov")
        h, w = ids.shape[-2:]
        if (-(-w // s), -(-h // s)) != (lw, lh):
            raise ValueError(f"a {w} x {h} window at scale {s} needs a {-(-w // s)} x {-(-h // s)} lattice, not {lw} x {lh}")
        a = self._aov_frames(aov, n, h, w, low.device, "aov")
        lead = tuple(low.shape[:-3]) + (h, w)
        if low_vmean is not None:
            self._plane(low_vmean, "low_vmean", tuple(low.shape[:-1]), low.device)
        out = self._filter_out(out, (*lead, 4), low.device, None,
                               "out must be a contiguous float32 CUDA tensor of the full-resolution frames' shape")
        weight = torch.empty(lead, dtype=torch.float32, device=low.device) if want_weight else None
        var = None if low_vmean is None else torch.empty(lead, dtype=torch.float32, device=low.device)
        self._follow(low.device)
        p = _lib.mm_upsample_params(s, float(w_min), 0, 0)
        self._check(lib().mm_upsample_frames(self._ctx, low.data_ptr(), C.byref(a), _ptr(low_vmean), C.byref(p), n, w, h,
                                             out.data_ptr(), _ptr(weight), _ptr(var)))
        return out, weight, var

    def fill_pixels(self, image, pixels, extra, m: float = 1.0, var=None, extra_vmean=None, weight=None,
                    x0: int = 0, y0: int = 0):
        """Replace the pixels of a list in a window's images, in place
        (mm_fill_pixels): image[p] = extra[e], and where given var[p] =
        extra_vmean[e] and weight[p] = m, copies exact on all bits.  `image`:
        the (h, w, 4) float32 CUDA tensor of the window (x0, y0, w, h);
        `pixels`, `extra`: a pixel list and what trace_pixels returned for it;
        `var`, `weight`: (h, w) float32 or None; `extra_vmean`: (n,) float32,
        given exactly when `var` is.  Entries outside the window are skipped;
        the list must not name a window pixel twice.  Returns `image`."""
        h, w = self._window(image)
        if (var is None) != (extra_vmean is None):
            raise ValueError("var and extra_vmean go together")
        pixels = self._pixel_list(pixels)
        n = pixels.shape[0]
        self._plane(extra, "extra", (n, 4), image.device, self._ENTRIES)
        if var is not None:
            self._plane(var, "var", (h, w), image.device, self._ENTRIES)
            self._plane(extra_vmean, "extra_vmean", (n,), image.device, self._ENTRIES)
        if weight is not None:
            self._plane(weight, "weight", (h, w), image.device, self._ENTRIES)
        self._follow(image.device)
        self._check(lib().mm_fill_pixels(self._ctx, image.data_ptr(), _ptr(var), _ptr(weight), x0, y0, w, h,
                                         _ptr(pixels, n), _ptr(extra, n), _ptr(extra_vmean, n), n, float(m)))
        return image

    def _low_var(self, ulow, cams, ext, x0, y0, w, h):
        """trace_upsampled's low view with its variance, (n, h, w, 4) and (n, h, w): one trace_tile_var launch for
        all cameras where the library takes it (a camera sequence is a multi-frame launch even with one camera, and
        a multi-frame variance launch needs the tail rings: MM_ERR_UNSUPPORTED below MM_OPT_DEFER_MIN paths,
        refused before anything is enqueued), else one single-frame call per camera -- the camera in the uniform,
        RNG frame ext.frame + f -- whose frame is the launch's bit for bit."""
        import torch

        n = cams.shape[0]
        if n > 1:
            try:
                low, lvar, _ = self.trace_tile_var(ulow, ext, x0, y0, w, h, cameras=cams)
                return low, lvar
            except _lib.MMError as err:
                if err.code != _lib.MM_ERR_UNSUPPORTED:
                    raise
        dev = f"cuda:{self.device}"
        low = torch.empty((n, h, w, 4), dtype=torch.float32, device=dev)
        lvar = torch.empty((n, h, w), dtype=torch.float32, device=dev)
        for f in range(n):
            uf = _lib.mm_uniform.from_buffer_copy(bytes(ulow))
            uf.cam = _args.camera(cams[f])
            ef = _lib.mm_ext(ext.spp, ext.bounce_limit, ext.mirror_limit, ext.frame + f, ext.flags, 0)
            self.trace_tile_var(uf, ef, x0, y0, w, h, out=low[f], var=lvar[f])
        return low, lvar

    def trace_upsampled(self, uniform: _lib.mm_uniform, cameras, ext: _lib.mm_ext, scale: int, x0: int, y0: int,
                        w: int, h: int, mirror_limit=None, w_min: float = 0.25, var: bool = False, fill: bool = True):
        """A camera sequence traced on the lattice of every scale-th pixel and
        rebuilt from the AOVs: the window (x0, y0, w, h) of uniform's view, one
        frame per camera (what trace_tile_cameras takes).  x0, y0 and the view
        size must be multiples of `scale`.  The steps:
          * the low view (view_w / scale, view_h / scale), tile (x0 / scale, y0
            / scale, ceil(w / scale), ceil(h / scale)), by trace_tile_cameras --
            with `var` by trace_tile_var, whose variance / ext.spp travels on:
            in one launch where a multi-frame variance launch runs (at least
            MM_OPT_DEFER_MIN paths, the tail rings), else one single-frame
            call per camera, which runs at any size and gives the same bits;
          * trace_aov of the full-resolution window (`mirror_limit`: None takes
            ext.mirror_limit);
          * upsample();
          * with `fill`, ONE trace_pixel_lists call over the holes of all
            frames -- the full view, list f's camera cameras[f] and RNG frame
            ext.frame + f, so a filled pixel equals that pixel of trace_tile on
            the full view bit for bit -- and one fill_pixels call per frame
            with m = 1.
        Returns (color (n, h, w, 4), aov, weight (n, h, w), var (n, h, w) or
        None, hole share per frame: a list of n floats, holes / (w * h) before
        the fill).  color, weight and var feed accumulate_var and denoise_var
        (count 1) unchanged once the holes are filled.
        RNG streams: a low-view pixel's stream is keyed by its index in the low
        view, so it coincides with the stream of an unrelated full-view pixel
        whose index is equal (a filled hole may share its stream with a lattice
        pixel elsewhere in the frame).  It correlates no neighbours."""
        s = int(scale)
        if s not in (2, 4, 8):
            raise ValueError("scale must be 2, 4 or 8")
        vw, vh = int(uniform.view_w), int(uniform.view_h)
        if vw != uniform.view_w or vh != uniform.view_h or any(v % s for v in (vw, vh, x0, y0)):
            raise ValueError(f"x0, y0 and the view size must be multiples of scale {s}")
        if ext.flags & (_lib.MM_EXT_ACCUMULATE | _lib.MM_EXT_RGBA8):
            raise ValueError("trace_upsampled takes a plain float frame: no MM_EXT_ACCUMULATE, no MM_EXT_RGBA8")
        cams = self._cameras(cameras)
        n = cams.shape[0]
        ulow = _lib.mm_uniform.from_buffer_copy(bytes(uniform))
        ulow.view_w, ulow.view_h = float(vw // s), float(vh // s)
        lw, lh = -(-w // s), -(-h // s)
        low_vmean = None
        if var:
            low, lvar = self._low_var(ulow, cams, ext, x0 // s, y0 // s, lw, lh)
            low_vmean = (lvar / float(ext.spp)).contiguous()
        else:
            low, _ = self.trace_tile_cameras(ulow, cams, ext, x0 // s, y0 // s, lw, lh)
        aov = self.trace_aov(uniform, cams, ext.mirror_limit if mirror_limit is None else mirror_limit,
                             x0=x0, y0=y0, w=w, h=h)
        color, weight, vout = self.upsample(low, aov, s, w_min, low_vmean)
        pixels, offsets = select_holes_frames(weight, x0, y0)
        share = [float(b - a) / float(w * h) for a, b in zip(offsets[:-1], offsets[1:])]
        if fill and int(offsets[-1]) > 0:
            e = _args.extra_ext(ext, ext.spp, ext.frame)
            extra, evar, _ = self.trace_pixel_lists(uniform, cams, e, pixels, offsets, var=True if var else None)
            evm = None if evar is None else (evar / float(ext.spp)).contiguous()
            for f in range(n):
                a, b = int(offsets[f]), int(offsets[f + 1])
                if a == b:
                    continue
                self.fill_pixels(color[f], pixels[a:b], extra[a:b], 1.0, None if vout is None else vout[f],
                                 None if evm is None else evm[a:b], weight[f], x0, y0)
        return color, aov, weight, vout, share

    def sync(self) -> None:
        """Wait for this context's work; raises MMError for the oldest
        trace_tile* call that failed on the GPU and was not reported yet (the
        message names that call)."""
        self._check(lib().mm_sync(self._ctx))

    def last_call(self) -> int:
        """Number of the last trace_tile / trace_tile_frames call (1, 2, ...)."""
        n = C.c_uint64()
        self._check(lib().mm_last_call(self._ctx, C.byref(n)))
        return n.value

    def call_status(self, call_id: int) -> bool:
        """Without waiting: True if call `call_id` finished clean, False while
        it runs; raises MMError (naming the call) if it failed on the GPU."""
        rc = lib().mm_call_status(self._ctx, call_id)
        if rc == _lib.MM_PENDING:
            return False
        self._check(rc)
        return True

    def set_profiling(self, enable: bool = True) -> None:
        self._check(lib().mm_set_profiling(self._ctx, 1 if enable else 0))

    def kernel_timing(self, reset: bool = True):
        """(summed ms, launches) of the ray-trace kernel since the last reset."""
        ms, n = C.c_float(), C.c_uint32()
        self._check(lib().mm_kernel_timing(self._ctx, C.byref(ms), C.byref(n), 1 if reset else 0))
        return ms.value, n.value

    def last_timing(self):
        ms, n = C.c_float(), C.c_uint32()
        self._check(lib().mm_last_timing(self._ctx, C.byref(ms), C.byref(n)))
        return ms.value, n.value


def make_ext(spp: int = 8, bounce_limit: int = 8, mirror_limit: int = 8, frame: int = 0,
             flags: int = 0) -> _lib.mm_ext:
    return _lib.mm_ext(spp, bounce_limit, mirror_limit, frame, flags, 0)
