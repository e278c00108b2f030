"""Shared by tests/test_variance.py and tests/test_gpu_variance.py: the CPU
reference of the per-pixel sample variance (tests/variance_ref.c, a plain C
statement of the definition in include/mm_api.h over the oracle's samples), and
the frame whose noisy pixels Renderer.refine tops up."""
from __future__ import annotations

import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np

import topup_support as TU

HERE = Path(__file__).resolve().parent
REPO = HERE.parent
VIEW = (64, 48)
TILE = (5, 3, 23, 10)  # x0, y0, w, h: w = 23 keeps pixels from aligning with waves
SPPS_LINEAR = (2, 3, 4, 12)   # k_resolve_var
SPPS_BLOCK = (8, 16, 24, 64)  # k_resolve8_var
# The refine test: one 8-spp frame of the walk's turned camera (topup_support.walk_cameras()[3]) at 160x120.
# REFINE_REL_TOL was derived from variance_ref.c alone (test_variance.py::test_refine_tolerance_from_the_reference
# repeats the derivation): the first round selects REFINE_SELECTED of the 19200 pixels, between 10 % and 50 %.
REFINE_VIEW = TU.WALK_VIEW
REFINE_SPP, REFINE_EXTRA, REFINE_FRAME = 8, 24, 0
REFINE_REL_TOL = 0.26
REFINE_SELECTED = 3882  # 20.2 %; the nearest pixel is 1.5e-4 (relative) from the threshold


def _cflags():
    mk = (REPO / "oracle" / "Makefile").read_text()
    return re.search(r"^CFLAGS\s*:=\s*(.*)$", mk, flags=re.M).group(1).split()


def build_ref(tmp_dir) -> C.CDLL:
    """Compile tests/variance_ref.c (which includes oracle/mm_oracle.c) into
    tmp_dir with the oracle Makefile's CFLAGS and bind it."""
    so = Path(tmp_dir) / "libvariance_ref.so"
    subprocess.run(["gcc", *_cflags(), "-Wno-unused-function", "-shared", "-o", str(so), str(HERE / "variance_ref.c"),
                    "-lm"], check=True)
    L = C.CDLL(str(so))
    P, U = C.c_void_p, C.c_uint32
    L.varref_samples.argtypes = [P, C.c_uint64, U, P, P]
    L.varref_tile.argtypes = [P, P, P, U, U, U, U, U, P, P]
    L.varref_pixels.argtypes = [P, P, P, P, C.c_uint64, P, P]
    L.oracle_trace_tile.argtypes = [P, P, P] + [U] * 5 + [P, P]
    return L


def build_driver(tmp_dir, flags=()) -> Path:
    """The reference's stand-alone driver (-DVARREF_MAIN), e.g. with sanitizers."""
    exe = Path(tmp_dir) / "variance_ref_main"
    subprocess.run(["gcc", *_cflags(), "-Wno-unused-function", *flags, "-DVARREF_MAIN", "-o", str(exe),
                    str(HERE / "variance_ref.c"), "-lm"], check=True)
    return exe


def samples_ref(L, samples):
    """(mean (n, 3), var (n,)) of (n, spp, 3) float32 samples."""
    s = np.ascontiguousarray(samples, dtype=np.float32)
    n, spp, _ = s.shape
    mean, var = np.zeros((n, 3), np.float32), np.zeros(n, np.float32)
    assert L.varref_samples(s.ctypes.data, n, spp, mean.ctypes.data, var.ctypes.data) == 0
    return mean, var


class Ref:
    """variance_ref.c on one scene (an oracle.Oracle holds the arrays)."""

    def __init__(self, L, scene):
        from oracle.oracle import Oracle

        self.L = L
        self.o = Oracle(scene.rects, scene.nodes, scene.idx, scene.is_mirror, scene.emission)

    @staticmethod
    def _args(uniform, ext):
        return C.create_string_buffer(bytes(uniform), 56), C.create_string_buffer(bytes(ext), len(bytes(ext)))

    def tile(self, uniform, ext, x0, y0, w, h, y_stride=1):
        """((h, w, 4) float32 out, (h, w) float32 var)."""
        out, var = np.zeros((h, w, 4), np.float32), np.zeros((h, w), np.float32)
        ub, eb = self._args(uniform, ext)
        assert self.L.varref_tile(C.byref(self.o.sc), ub, eb, x0, y0, w, h, y_stride, out.ctypes.data,
                                  var.ctypes.data) == 0
        return out, var

    def pixels(self, uniform, ext, pixels):
        px = np.ascontiguousarray(pixels, dtype=np.uint32)
        out, var = np.zeros((len(px), 4), np.float32), np.zeros(len(px), np.float32)
        ub, eb = self._args(uniform, ext)
        assert self.L.varref_pixels(C.byref(self.o.sc), ub, eb, px.ctypes.data, len(px), out.ctypes.data,
                                    var.ctypes.data) == 0
        return out, var

    def oracle_tile(self, uniform, ext, x0, y0, w, h, y_stride=1):
        """oracle_trace_tile of this library: (h, w, 4) float32."""
        from oracle.oracle import Stats

        out, st = np.zeros((h, w, 4), np.float32), Stats()
        ub, eb = self._args(uniform, ext)
        assert self.L.oracle_trace_tile(C.byref(self.o.sc), ub, eb, x0, y0, w, h, y_stride, out.ctypes.data,
                                        C.byref(st)) == 0
        return out


def list_pixels(seed=5):
    """The pixel list of the GPU test, (200, 2) uint32: entries of TILE in random
    order with duplicates, four entries outside the 64x48 view and (2^31, 2^31);
    and the mask of the entries inside the view."""
    rng = np.random.default_rng(seed)
    x0, y0, w, h = TILE
    flat = rng.integers(0, w * h, 195)
    flat[10:20] = flat[0:10]  # duplicates for certain
    px = np.stack([x0 + flat % w, y0 + flat // w], axis=1).astype(np.int64)
    out = np.array([[VIEW[0], 3], [3, VIEW[1]], [2**32 - 1, 0], [70, 50], [2**31, 2**31]], dtype=np.int64)
    px = np.concatenate([px, out])
    px = px[rng.permutation(len(px))]
    inside = (px[:, 0] < VIEW[0]) & (px[:, 1] < VIEW[1])
    return np.ascontiguousarray(px.astype(np.uint32)), inside


def view_uniform(cam=0):
    """The mm_uniform of the 64x48 view: camera `cam` of the walk inside the maze
    (from the default camera, outside the N=4 maze, nearly every pixel is black
    and its variance 0)."""
    from mirror_maze import default_uniform, mm_camera

    u = default_uniform(*VIEW, 0)
    u.cam = mm_camera.from_buffer_copy(np.ascontiguousarray(TU.walk_cameras()[cam], dtype=np.float32).tobytes())
    return u


def refine_uniform():
    """The mm_uniform of the refine test's frame."""
    from mirror_maze import default_uniform, mm_camera

    vw, vh = REFINE_VIEW
    u = default_uniform(vw, vh, 0)
    u.cam = mm_camera.from_buffer_copy(np.ascontiguousarray(TU.walk_cameras()[3], dtype=np.float32).tobytes())
    return u


def noisy_numpy(color, var, count, rel_tol, floor=1e-3):
    """The inequality of select_noisy in float64 numpy: (mask, relative margin
    of each pixel to the threshold)."""
    c = np.asarray(color, dtype=np.float64)
    lum = 0.25 * c[..., 0] + 0.5 * c[..., 1] + 0.25 * c[..., 2]
    lhs = np.sqrt(np.asarray(var, dtype=np.float64) / np.asarray(count, dtype=np.float64))
    rhs = rel_tol * (lum + floor)
    return lhs > rhs, np.abs(lhs - rhs) / np.maximum(rhs, 1e-300)
