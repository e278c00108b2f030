"""Shared by tests/test_temporal_var.py and tests/test_gpu_temporal_var.py: the
CPU reference of mm_accumulate_frames_var and mm_blend_pixels_var
(tests/temporal_var_ref.c, a plain C statement of the arithmetic in
include/mm_api.h), and the variances and weights both files feed it beside
temporal_support's sequences."""
from __future__ import annotations

import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np

import temporal_support as T

HERE = Path(__file__).resolve().parent
REPO = HERE.parent
NAMES = T.NAMES
COUNTS = (*T.COUNTS, "m_above_cap", "tiny_product")
SPP = 8  # the scene sequences' samples per pixel: vmean = var / SPP
WEIGHTS = np.float32([0.5, 1.0, 1.75, 2.0, 8.0])  # 8 exceeds the caps n_max = 1 and 4


def build_ref(tmp_dir) -> C.CDLL:
    """Compile tests/temporal_var_ref.c into tmp_dir with the oracle Makefile's
    CFLAGS (as temporal_support.build_ref does) and bind it."""
    mk = (REPO / "oracle" / "Makefile").read_text()
    cflags = re.search(r"^CFLAGS\s*:=\s*(.*)$", mk, flags=re.M).group(1).split()
    so = Path(tmp_dir) / "libtemporal_var_ref.so"
    subprocess.run(["gcc", *cflags, "-shared", "-o", str(so), str(HERE / "temporal_var_ref.c"), "-lm"], check=True)
    L = C.CDLL(str(so))
    P, U, F = C.c_void_p, C.c_uint32, C.c_float
    L.tvref_accumulate.argtypes = [F, F, P, P, P, P, P, P, P, P, P, P, P, P, P, U, F, F, U, U, U, U, U, P, P, P]
    L.tvref_blend.argtypes = [P, P, U, U, U, U, P, P, P, C.c_uint64, F]
    L.tvref_blend.restype = C.c_uint64
    assert L.tvref_n_counts() == len(COUNTS)
    return L


def accumulate_ref(L, view, cams, color, guides, vmean, weight=None, prev=None, n_max=32, tol_z=0.02, w_min=0.25,
                   x0=0, y0=0):
    """(accumulated (n, h, w, 4) float32, its variance (n, h, w) float32, dict
    of the call's counts): the arguments of temporal_support.accumulate_ref,
    and `vmean` (n, h, w), `weight` None or (n, h, w); `prev` None or (color
    (h, w, 4), guides of one frame, camera (10,), variance (h, w))."""
    color = np.ascontiguousarray(color, dtype=np.float32)
    n, h, w, _ = color.shape
    cams = np.ascontiguousarray(cams, dtype=np.float32).reshape(n, 10)
    nd, al, ids = T._guides(guides, n, h, w)
    vm = np.ascontiguousarray(vmean, dtype=np.float32).reshape(n, h, w)
    wt = None if weight is None else np.ascontiguousarray(weight, dtype=np.float32).reshape(n, h, w)
    pp = [None] * 6
    if prev is not None:
        pc = np.ascontiguousarray(prev[0], dtype=np.float32).reshape(h, w, 4)
        pnd, pal, pid = T._guides(prev[1], 1, h, w)
        pcam = np.ascontiguousarray(prev[2], dtype=np.float32).reshape(10)
        pvar = np.ascontiguousarray(prev[3], dtype=np.float32).reshape(h, w)
        keep = (pc, pnd, pal, pid, pcam, pvar)
        pp = [a.ctypes.data for a in keep]
    out = np.zeros_like(color)
    vout = np.zeros((n, h, w), np.float32)
    cnt = np.zeros(len(COUNTS), np.uint64)
    rc = L.tvref_accumulate(view[0], view[1], cams.ctypes.data, color.ctypes.data, nd.ctypes.data, al.ctypes.data,
                            ids.ctypes.data, vm.ctypes.data, None if wt is None else wt.ctypes.data, *pp, n_max, tol_z,
                            w_min, n, x0, y0, w, h, out.ctypes.data, vout.ctypes.data, cnt.ctypes.data)
    assert rc == 0, rc
    return out, vout, dict(zip(COUNTS, (int(x) for x in cnt)))


def blend_ref(L, image, var, x0, y0, pixels, extra, extra_vmean, m):
    """(blended copy of `image` (h, w, 4), of `var` (h, w), entries inside the window)."""
    out = np.array(image, dtype=np.float32, order="C")
    vo = np.array(var, dtype=np.float32, order="C")
    h, w, _ = out.shape
    px = np.ascontiguousarray(pixels, dtype=np.uint32)
    ex = np.ascontiguousarray(extra, dtype=np.float32)
    ev = np.ascontiguousarray(extra_vmean, dtype=np.float32)
    n = L.tvref_blend(out.ctypes.data, vo.ctypes.data, x0, y0, w, h, px.ctypes.data, ex.ctypes.data, ev.ctypes.data,
                      px.shape[0], m)
    return out, vo, int(n)


def synthetic_vmean(shape, seed=None):
    """The synthetic sequence's (4, h, w) float32 variances: random values in
    [0, 1), salted with exact zeros, 1e-40 (a subnormal) and 1e30."""
    w, h = shape
    seed = w * 1000 + h if seed is None else seed
    rng = np.random.default_rng(seed + 4099)
    v = rng.uniform(0.0, 1.0, size=(T.N_FRAMES, h, w)).astype(np.float32)
    salt = rng.integers(0, 12, size=v.shape)
    v[salt == 0] = np.float32(0.0)
    v[salt == 1] = np.float32(1e-40)
    v[salt == 2] = np.float32(1e30)
    return np.ascontiguousarray(v)


def weights(shape, n=T.N_FRAMES, seed=None):
    """A per-pixel weight image (n, h, w) float32 drawn from WEIGHTS in blocks
    3 x 5 pixels wide (neighbouring taps meet equal and unequal weights)."""
    w, h = shape
    seed = w * 1000 + h if seed is None else seed
    rng = np.random.default_rng(seed + 911)
    g = rng.integers(0, len(WEIGHTS), size=(n, -(-h // 3) + 1, -(-w // 5) + 1))
    g = np.repeat(np.repeat(g, 3, axis=1), 5, axis=2)
    oy, ox = rng.integers(0, 3), rng.integers(0, 5)
    return np.ascontiguousarray(WEIGHTS[g[:, oy:oy + h, ox:ox + w]])


def vmean_of(var, count=SPP):
    """var / count as the tests form it: numpy float32, so that the reference
    and the GPU see the same bits."""
    return np.ascontiguousarray(np.asarray(var, dtype=np.float32) / np.float32(count))


def lum(c):
    """The denoiser's luminance of (..., >= 3) colours, float64."""
    c = np.asarray(c, dtype=np.float64)
    return 0.25 * c[..., 0] + 0.5 * c[..., 1] + 0.25 * c[..., 2]
