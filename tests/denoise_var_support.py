"""Shared by tests/test_denoise_var.py and tests/test_gpu_denoise_var.py: the
CPU reference of mm_denoise_frames_var (tests/denoise_var_ref.c, a plain C
statement of the filter in include/mm_api.h) and the variance field the tests
filter beside denoise_support's synthetic colours and guides."""
from __future__ import annotations

import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np

import denoise_support as D
from denoise_support import SHAPES, corridor_view, maze_view, synthetic  # noqa: F401

HERE = Path(__file__).resolve().parent
REPO = HERE.parent
COUNTS = (*D.COUNTS, "pre_out_of_tile", "pre_rej_id", "pre_rej_mh", "pre_rej_normal", "pre_taken", "tiny_product",
          "stop_is_eps")
PASSES = [1, 2, 3, 5, 8]
# (sigma_z, sigma_l, eps_l) of the GPU cases.  MAIN: SVGF's stop.  TINY: a stop of 1e-18 wherever the 3x3 of V is
# zero -- below the guarded quotients' range, luminance steps over it overflow t*t, weights and their squares
# underflow -- beside ordinary stops elsewhere in the same image.
MAIN = (0.02, 4.0, 1e-3)
TINY = (0.3, 0.5, 1e-18)


def build_ref(tmp_dir) -> C.CDLL:
    """Compile tests/denoise_var_ref.c into tmp_dir with the oracle Makefile's
    CFLAGS (as denoise_support.build_ref does) and bind it."""
    mk = (REPO / "oracle" / "Makefile").read_text()
    cflags = re.search(r"^CFLAGS\s*:=\s*(.*)$", mk, flags=re.M).group(1).split()
    so = Path(tmp_dir) / "libdenoise_var_ref.so"
    subprocess.run(["gcc", *cflags, "-shared", "-o", str(so), str(HERE / "denoise_var_ref.c"), "-lm"], check=True)
    L = C.CDLL(str(so))
    P = C.c_void_p
    L.dnvref_filter.argtypes = [P, P, P, P, P, C.c_uint32, C.c_float, C.c_float, C.c_float, C.c_uint32, C.c_uint32,
                                C.c_uint32, P, P, P]
    assert L.dnvref_n_counts() == len(COUNTS)
    return L


def filter_ref(L, color, guides, vmean, n_passes=5, sigma_z=0.02, sigma_l=4.0, eps_l=1e-3):
    """(filtered (n, h, w, 4) float32, filtered variance (n, h, w) float32,
    dict of the call's tap counts) of `color` (h, w, 4) or (n, h, w, 4) with
    guides of matching shapes and `vmean` (h, w) or (n, h, w), the variance
    of the pixel mean."""
    color = np.ascontiguousarray(color, dtype=np.float32)
    if color.ndim == 3:
        color = color[None]
    n, h, w, _ = color.shape
    nd = np.ascontiguousarray(guides["normal_depth"], dtype=np.float32).reshape(n, h, w, 4)
    al = np.ascontiguousarray(guides["albedo"], dtype=np.float32).reshape(n, h, w, 4)
    ids = np.ascontiguousarray(np.asarray(guides["id"]).view(np.uint32)).reshape(n, h, w)
    v = np.ascontiguousarray(vmean, dtype=np.float32).reshape(n, h, w)
    out = np.zeros_like(color)
    vout = np.zeros_like(v)
    cnt = np.zeros(len(COUNTS), np.uint64)
    rc = L.dnvref_filter(color.ctypes.data, nd.ctypes.data, al.ctypes.data, ids.ctypes.data, v.ctypes.data, n_passes,
                         sigma_z, sigma_l, eps_l, n, w, h, out.ctypes.data, vout.ctypes.data, cnt.ctypes.data)
    assert rc == 0, rc
    return out, vout, dict(zip(COUNTS, (int(x) for x in cnt)))


def synthetic_var(n, h, w, seed):
    """A variance-of-the-mean field (n, h, w) float32 made to keep the new
    clauses busy: in blocks 4 x 6 pixels wide, exact 0 (the stop is eps_l
    there), 1e-40 (a subnormal: every product with it is one or zero), or a
    per-pixel spread 1e-12 .. 1e2."""
    rng = np.random.default_rng(seed ^ 0x5EED)
    gh, gw = -(-h // 4) + 1, -(-w // 6) + 1
    kind = rng.integers(0, 4, size=(n, gh, gw))
    kind = np.repeat(np.repeat(kind, 4, axis=1), 6, axis=2)
    oy, ox = rng.integers(0, 4), rng.integers(0, 6)
    kind = kind[:, oy:oy + h, ox:ox + w]
    spread = (10.0 ** rng.uniform(-12.0, 2.0, size=(n, h, w))).astype(np.float32)
    v = np.where(kind == 0, np.float32(0.0), np.where(kind == 1, np.float32(1e-40), spread)).astype(np.float32)
    return np.ascontiguousarray(v)
