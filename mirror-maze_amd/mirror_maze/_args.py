"""What Renderer's methods do to their arguments before a C call, where it needs no context: the one tensor
check, camera, pixel-list and ray-list conversion, the offsets and frame keys of trace_pixel_lists, and the two ext
builders.  Each caller keeps its own refusal text."""
from __future__ import annotations

import numpy as np

from . import _lib


def tensor_ok(t, dtypes, shapes=None, numel=None, device=None, contiguous=True) -> bool:
    """True if `t` is a CUDA tensor of one of `dtypes` (a dtype or a tuple of them) whose shape is one of `shapes`
    (None in a shape: any extent; a leading Ellipsis: any leading axes) or that holds `numel` elements, on `device`
    (None: any CUDA device), contiguous unless that is not asked for."""
    import torch

    if not (torch.is_tensor(t) and t.is_cuda and (device is None or t.device == device)
            and (t.dtype in dtypes if isinstance(dtypes, tuple) else t.dtype == dtypes)
            and (not contiguous or t.is_contiguous()) and (numel is None or t.numel() == numel)):
        return False
    if shapes is None:
        return True
    have = tuple(t.shape)
    for want in shapes:
        if want and want[0] is Ellipsis:
            want = want[1:]
            got = have[max(0, len(have) - len(want)):]
        else:
            got = have
        if len(got) == len(want) and all(w is None or w == g for w, g in zip(want, got)):
            return True
    return False


def call_ext(ext, stats, r8):
    """The mm_ext of a trace call: the caller's, with the flags the call's own arguments ask for."""
    return _lib.mm_ext(ext.spp, ext.bounce_limit, ext.mirror_limit, ext.frame,
                       ext.flags | (_lib.MM_EXT_COUNT_STATS if stats else 0) | (_lib.MM_EXT_RGBA8 if r8 else 0), 0)


def extra_ext(ext, spp, frame):
    """The mm_ext of an extra-sample round: `spp` samples with RNG frame `frame` into a float list of their own."""
    return _lib.mm_ext(int(spp), ext.bounce_limit, ext.mirror_limit, int(frame),
                       ext.flags & ~(_lib.MM_EXT_ACCUMULATE | _lib.MM_EXT_RGBA8 | _lib.MM_EXT_COUNT_STATS), 0)


def cameras(cameras) -> np.ndarray:
    """(n, 10) float32 camera records (sizeof(mm_camera) = 40 B per row) from
    an (n, 10) array or a sequence of mm_camera / mm_uniform (its .cam)."""
    if isinstance(cameras, np.ndarray):
        cams = np.ascontiguousarray(cameras, dtype=np.float32)
    else:
        rows = [np.frombuffer(bytes(getattr(c, "cam", c)), dtype=np.float32) for c in cameras]
        cams = np.stack(rows) if rows else np.zeros((0, 10), dtype=np.float32)
    if cams.ndim != 2 or cams.shape[1] != 10:
        raise ValueError("cameras must be mm_camera / mm_uniform values or an (n, 10) float32 array")
    return cams


def camera(c) -> _lib.mm_camera:
    """The mm_camera of one camera: a mm_camera, a mm_uniform (its .cam) or an array of 10 floats."""
    return _lib.mm_camera.from_buffer_copy(cameras(c.reshape(1, -1) if isinstance(c, np.ndarray) else [c]).tobytes())


def pixel_array(pixels) -> np.ndarray:
    """The (n, 2) int32 array of an array of (x, y) pairs (int32 holds the bits of the library's uint32)."""
    pixels = np.ascontiguousarray(pixels)
    if pixels.dtype.kind not in "iu":
        raise ValueError("pixels must hold integers")
    return pixels.astype(np.uint32).view(np.int32).reshape(-1, 2)


def pixel_list(pixels, device):
    """The (n, 2) int32 CUDA tensor of a pixel list: `pixels` itself, or an
    upload of an (n, 2) array of (x, y) pairs to `device`."""
    import torch

    if not torch.is_tensor(pixels):
        pixels = torch.from_numpy(pixel_array(pixels)).to(device)
    if pixels.dtype == getattr(torch, "uint32", None):
        pixels = pixels.view(torch.int32)
    if not tensor_ok(pixels, torch.int32, ((None, 2),)):
        raise ValueError("pixels must be a contiguous int32 / uint32 (n, 2) CUDA tensor or an (n, 2) array")
    return pixels


def ray_list(rays):
    """trace_rays' records: `rays` itself, a contiguous (n, 8) float32 CUDA tensor."""
    import torch

    if not tensor_ok(rays, torch.float32, ((None, 8),)):
        raise ValueError("rays must be a contiguous float32 (n, 8) CUDA tensor")
    return rays


def list_offsets(offsets, n) -> np.ndarray:
    """trace_pixel_lists' offsets as a uint64 array: n_lists + 1 >= 2 values on the host that end at `n`."""
    import torch

    offs = np.ascontiguousarray(np.asarray(offsets.cpu() if torch.is_tensor(offsets) else offsets),
                                dtype=np.uint64).reshape(-1)
    if offs.shape[0] < 2:
        raise ValueError("offsets must hold n_lists + 1 values, n_lists >= 1")
    if int(offs[-1]) != n:
        raise ValueError(f"offsets end at {int(offs[-1])}, the pixel array holds {n} entries")
    return offs


def list_keys(frame_keys, n_lists):
    """trace_pixel_lists' frame keys as a uint32 array of n_lists values, or None."""
    if frame_keys is None:
        return None
    keys = np.ascontiguousarray(np.asarray(frame_keys), dtype=np.uint32).reshape(-1)
    if keys.shape[0] != n_lists:
        raise ValueError(f"{n_lists} lists need {n_lists} frame keys, not {keys.shape[0]}")
    return keys
