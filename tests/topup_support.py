"""Shared by tests/test_topup.py and tests/test_gpu_topup.py: the CPU reference
of mm_blend_pixels (tests/topup_ref.c, a plain C statement of the arithmetic in
include/mm_api.h), the inputs both files blend, and the walk whose last frame
is topped up."""
from __future__ import annotations

import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
REPO = HERE.parent
WINDOW = (11, 7, 37, 5)  # x0, y0, w, h
ALPHAS = np.float32([1.0, 2.5, 31.0])
WEIGHTS = (0.5, 3.0, 8.0)
# The walk: four frames at 160x120 inside the N=4 maze, a few centimetres apart, the last one turned by
# TURN_DEG about the vertical axis: the columns the turn brings into view have no history.
WALK_VIEW = (160, 120)
WALK_CELL = (1, 1)
WALK_YAW, TURN_DEG = 90.0, 10.0
WALK_SELECTED = 3569  # pixels of the last frame with N < 2 (test_topup.py derives it on the CPU)


def _cflags():
    mk = (REPO / "oracle" / "Makefile").read_text()
    return re.search(r"^CFLAGS\s*:=\s*(.*)$", mk, flags=re.M).group(1).split()


def build_ref(tmp_dir) -> C.CDLL:
    """Compile tests/topup_ref.c into tmp_dir with the oracle Makefile's CFLAGS
    (as temporal_support.build_ref does) and bind it."""
    so = Path(tmp_dir) / "libtopup_ref.so"
    subprocess.run(["gcc", *_cflags(), "-shared", "-o", str(so), str(HERE / "topup_ref.c"), "-lm"], check=True)
    L = C.CDLL(str(so))
    P, U = C.c_void_p, C.c_uint32
    L.topup_blend.argtypes = [P, U, U, U, U, P, P, C.c_uint64, C.c_float]
    L.topup_blend.restype = C.c_uint64
    return L


def build_driver(tmp_dir, flags=()) -> Path:
    """The reference's stand-alone driver (-DTOPUP_MAIN), e.g. with sanitizers."""
    exe = Path(tmp_dir) / "topup_ref_main"
    subprocess.run(["gcc", *_cflags(), *flags, "-DTOPUP_MAIN", "-o", str(exe), str(HERE / "topup_ref.c"), "-lm"],
                   check=True)
    return exe


def blend_ref(L, image, x0, y0, pixels, extra, m):
    """(blended copy of `image` (h, w, 4), entries inside the window)."""
    out = np.array(image, dtype=np.float32, order="C")
    h, w, _ = out.shape
    px = np.ascontiguousarray(pixels, dtype=np.uint32)
    ex = np.ascontiguousarray(extra, dtype=np.float32)
    n = L.topup_blend(out.ctypes.data, x0, y0, w, h, px.ctypes.data, ex.ctypes.data, px.shape[0], m)
    return out, int(n)


def blend_numpy(image, x0, y0, pixels, extra, m):
    """The definition in include/mm_api.h as float32 numpy operations (each one
    rounds to binary32; the list names no window pixel twice)."""
    out = np.array(image, dtype=np.float32, order="C")
    h, w, _ = out.shape
    px = np.asarray(pixels).astype(np.int64)
    inside = (px[:, 0] >= x0) & (px[:, 0] < x0 + w) & (px[:, 1] >= y0) & (px[:, 1] < y0 + h)
    j, i = px[inside, 1] - y0, px[inside, 0] - x0
    A = out[j, i]
    E = np.asarray(extra, dtype=np.float32)[inside]
    m = np.float32(m)
    Nn = A[:, 3] + m
    rgb = A[:, :3] + ((E[:, :3] - A[:, :3]) * m) / Nn[:, None]
    assert rgb.dtype == np.float32 and Nn.dtype == np.float32
    out[j, i] = np.concatenate([rgb, Nn[:, None]], axis=1)
    return out


def blend_inputs(seed=8):
    """(image (5, 37, 4), pixels (n, 2) uint32, extra (n, 4)): seeded colours,
    alphas from ALPHAS; the list names 120 of the window's pixels once each, in
    random order, among 40 entries outside it -- just left of, right of, above
    and below the window, far away, and (2^31, 2^31)."""
    rng = np.random.default_rng(seed)
    x0, y0, w, h = WINDOW
    image = rng.uniform(0.0, 2.0, size=(h, w, 4)).astype(np.float32)
    image[..., 3] = ALPHAS[rng.integers(0, len(ALPHAS), size=(h, w))]
    flat = rng.permutation(w * h)[:120]
    inside = np.stack([x0 + flat % w, y0 + flat // w], axis=1)
    edge = np.array([[x0 - 1, y0], [x0 + w, y0], [x0, y0 - 1], [x0, y0 + h], [x0 + w - 1, y0 + h], [0, 0],
                     [2**31, 2**31], [2**32 - 1, y0], [x0, 2**32 - 1]], dtype=np.int64)
    far = np.stack([rng.integers(x0 + w, 4000, 31), rng.integers(0, 4000, 31)], axis=1)
    px = np.concatenate([inside, edge, far])
    px = np.ascontiguousarray(px[rng.permutation(len(px))].astype(np.uint32))
    extra = rng.uniform(0.0, 2.0, size=(len(px), 4)).astype(np.float32)
    return image, px, extra


def walk_cameras():
    """The (4, 10) float32 cameras of the walk."""
    from mirror_maze import calculate_quaternion, default_uniform

    vw, vh = WALK_VIEW
    base = -10.0 * 2  # the N=4 maze spans [-20, 20]: cell (i, k) is centred at base + 10 i + 5
    cams = np.tile(np.frombuffer(bytes(default_uniform(vw, vh, 0).cam), dtype=np.float32), (4, 1)).copy()
    for f in range(4):
        yaw = np.radians(WALK_YAW + (TURN_DEG if f == 3 else 0.0))
        cams[f, 0] = base + 10.0 * WALK_CELL[0] + 5.0 + 0.013 * f
        cams[f, 1] = -2.0
        cams[f, 2] = base + 10.0 * WALK_CELL[1] + 5.0 + 0.021 * f
        cams[f, 4:8] = calculate_quaternion(np.float32([np.sin(yaw), 0.0, np.cos(yaw)]))
    return cams
