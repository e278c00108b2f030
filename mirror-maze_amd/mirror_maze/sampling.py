"""The torch bookkeeping around the extra-sample rounds of Renderer.top_up / refine and the hole filling of
Renderer.trace_upsampled: which pixels a round traces (select_*) and how its samples are pooled with the ones a
pixel holds (merge_samples).  Plain torch operations on the tensors' device, CPU tensors included; no Renderer and
no library."""
from __future__ import annotations

import numpy as np

from . import _lib


def _lum(c):
    """The denoiser's luminance of (..., >= 3) colours."""
    return (0.25 * c[..., 0] + 0.5 * c[..., 1]) + 0.25 * c[..., 2]


def _has_history(ids, lead):
    """The mask of the pixels whose id is neither MM_AOV_ID_MISS nor MM_AOV_ID_FAILED (those never get a history)."""
    ids = ids.reshape(lead)
    miss, failed = _lib.MM_AOV_ID_MISS - (1 << 32), _lib.MM_AOV_ID_FAILED - (1 << 32)  # the int32 with those bits
    return (ids != miss) & (ids != failed)


def _noisy(color, var, count, rel_tol, floor, ids):
    """select_noisy's mask over the leading axes of `color`, (h, w) or (n, h, w)."""
    import torch

    lead = color.shape[:-1]
    var = var.reshape(lead)
    if torch.is_tensor(count):
        count = count.reshape(lead)
    sel = torch.sqrt(var / count) > rel_tol * (_lum(color) + floor)
    return sel if ids is None else sel & _has_history(ids, lead)


def _listed(sel, x0, y0):
    """(rows, pixels) of a mask (h, w) or (n, h, w): torch.nonzero's rows ([f,] j, i), frame-major and row-major
    (deterministic, no duplicates), and their (x0 + i, y0 + j) pairs as an (n, 2) int32 tensor."""
    import torch

    rows = torch.nonzero(sel)
    return rows, torch.stack((rows[:, -1] + x0, rows[:, -2] + y0), dim=1).to(torch.int32).contiguous()


def select_short_history(acc, ids, n_min: float, x0: int = 0, y0: int = 0):
    """The pixel list Renderer.top_up traces: the pixels of the accumulated
    window `acc` ((h, w, 4), alpha = history length) with alpha < n_min whose
    `ids` entry ((h, w) or (1, h, w) int32, the guides' id buffer) is neither
    MM_AOV_ID_MISS nor MM_AOV_ID_FAILED, as an (n, 2) int32 tensor of (x0 + i,
    y0 + j) pairs in row-major order (torch.nonzero's: deterministic, no
    duplicates) on acc's device.  Works on CPU tensors too."""
    if acc.dim() != 3 or acc.shape[-1] != 4:
        raise ValueError("acc must be one (h, w, 4) frame")
    return _listed((acc[..., 3] < n_min) & _has_history(ids, acc.shape[:2]), x0, y0)[1]


def select_noisy(color, var, count, rel_tol: float, floor: float = 1e-3, ids=None, x0: int = 0, y0: int = 0):
    """The pixel list Renderer.refine traces: the pixels of the window `color`
    ((h, w, 4) or (h, w, 3)) whose mean's standard error, sqrt(var / count), is
    above rel_tol * (lum(color) + floor) -- `var` (h, w) as trace_tile_var
    returns it, `count` the samples per pixel, a scalar or an (h, w) tensor;
    `floor` keeps black pixels from being selected for ever.  With `ids` ((h, w)
    or (1, h, w) int32, a guides' id buffer) a pixel whose id is MM_AOV_ID_MISS
    or MM_AOV_ID_FAILED is never selected.  Returns an (n, 2) int32 tensor of
    (x0 + i, y0 + j) pairs in row-major order (torch.nonzero's: deterministic,
    no duplicates) on color's device.  Works on CPU tensors too."""
    if color.dim() != 3 or color.shape[-1] < 3:
        raise ValueError("color must be one (h, w, 4) frame")
    return _listed(_noisy(color, var, count, rel_tol, floor, ids), x0, y0)[1]


def _select_noisy_frames(color, var, count, rel_tol, floor, ids, x0, y0):
    """select_noisy_frames' (pixels, offsets) and the (N, 3) rows (f, j, i) of
    the selected pixels, frame-major and row-major."""
    import torch

    if color.dim() != 4 or color.shape[-1] < 3:
        raise ValueError("color must be (n, h, w, 4) frames")
    fji, pixels = _listed(_noisy(color, var, count, rel_tol, floor, ids), x0, y0)
    per_frame = torch.bincount(fji[:, 0], minlength=color.shape[0])
    offsets = np.zeros(color.shape[0] + 1, dtype=np.uint64)
    offsets[1:] = torch.cumsum(per_frame, 0).cpu().numpy()
    return pixels, offsets, fji


def select_noisy_frames(color, var, count, rel_tol: float, floor: float = 1e-3, ids=None, x0: int = 0, y0: int = 0):
    """select_noisy() for a batch of frames at once, the lists
    Renderer.refine_frames traces: `color` (n, h, w, 4), `var` (n, h, w),
    `count` a scalar or (n, h, w), `ids` None or the frames' id buffers.
    Returns (pixels, offsets): the frames' select_noisy lists back to back,
    an (N, 2) int32 tensor on color's device, and the n + 1 offsets of the
    lists in it as a uint64 numpy array (one read-back for the whole batch),
    as Renderer.trace_pixel_lists takes them.  Works on CPU tensors too."""
    pixels, offsets, _ = _select_noisy_frames(color, var, count, rel_tol, floor, ids, x0, y0)
    return pixels, offsets


def select_holes(weight, x0: int = 0, y0: int = 0):
    """The holes of ONE upsampled frame: the pixels of `weight` ((h, w), what
    Renderer.upsample returns beside the colour) that are 0, as an (n, 2) int32
    tensor of (x0 + i, y0 + j) pairs in row-major order (torch.nonzero's:
    deterministic, no duplicates) on weight's device.  Works on CPU tensors
    too."""
    if weight.dim() != 2:
        raise ValueError("weight must be one (h, w) frame")
    return _listed(weight == 0, x0, y0)[1]


def select_holes_frames(weight, x0: int = 0, y0: int = 0):
    """select_holes() for a batch of frames at once: `weight` (n, h, w).
    Returns (pixels, offsets) in select_noisy_frames' form -- the frames' lists
    back to back as an (N, 2) int32 tensor and their n + 1 offsets as a uint64
    numpy array (one read-back for the whole batch) -- as
    Renderer.trace_pixel_lists takes them.  Works on CPU tensors too."""
    import torch

    if weight.dim() != 3:
        raise ValueError("weight must be (n, h, w) frames")
    fji, pixels = _listed(weight == 0, x0, y0)
    offsets = np.zeros(weight.shape[0] + 1, dtype=np.uint64)
    offsets[1:] = torch.cumsum(torch.bincount(fji[:, 0], minlength=weight.shape[0]), 0).cpu().numpy()
    return pixels, offsets


def merge_samples(mean_a, var_a, n_a, mean_b, var_b, n_b):
    """Pool two independent groups of samples of the same pixels: `mean_*`
    (..., 3) colours, `var_*` (...) variances of one sample's luminance as
    trace_tile_var / trace_pixels_var return them, `n_*` the samples in each
    group (scalars or (...) tensors).  Returns (mean, var, n) of the n_a + n_b
    samples together:
      mean = mean_a + (mean_b - mean_a) * n_b / (n_a + n_b)          per channel
      var  = ((n_a-1) var_a + (n_b-1) var_b
              + n_a n_b / (n_a+n_b) * (lum(mean_a) - lum(mean_b))**2) / (n_a + n_b - 1)
    Plain float32 torch operations, on the tensors' device: this is bookkeeping
    over the pixels a round selected, not on the hot path, and stays in torch."""
    import torch

    n_a = torch.as_tensor(n_a, dtype=torch.float32, device=mean_a.device)
    n_b = torch.as_tensor(n_b, dtype=torch.float32, device=mean_a.device)
    n = n_a + n_b
    mean = mean_a + (mean_b - mean_a) * n_b.unsqueeze(-1) / n.unsqueeze(-1)
    d = _lum(mean_a) - _lum(mean_b)
    var = ((n_a - 1.0) * var_a + (n_b - 1.0) * var_b + n_a * n_b / n * d ** 2) / (n - 1.0)
    return mean, var, n


def merge_at(at, color, var, count, mean_b, var_b, n_b):
    """A round's n_b extra samples per pixel (`mean_b` (N, >= 3), `var_b` (N,)) pooled by merge_samples into
    color[..., :3], var and count at the N pixels the index tensors `at` name, in place."""
    rgb = (*at, slice(0, 3))
    color[rgb], var[at], count[at] = merge_samples(color[rgb], var[at], count[at], mean_b[:, :3], var_b, float(n_b))
