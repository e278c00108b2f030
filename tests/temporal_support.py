"""Shared by tests/test_temporal.py and tests/test_gpu_temporal.py: the CPU
reference of mm_accumulate_frames (tests/temporal_ref.c, a plain C statement of
the arithmetic in include/mm_api.h) and the sequences both files accumulate."""
from __future__ import annotations

import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np

import denoise_support as D

HERE = Path(__file__).resolve().parent
REPO = HERE.parent
NAMES = ("normal_depth", "albedo", "id")
COUNTS = ("no_frame", "miss", "behind", "out_of_window", "tap_outside", "rej_id", "rej_mh", "rej_normal", "rej_dist",
          "w_below", "blended", "n_capped")
DEFAULTS = dict(n_max=32, tol_z=0.02, w_min=0.25)
N_FRAMES = 4
N_MAX = (1, 4, 65535)
MIRROR_LIMIT = 8
# The sequences.  The two walks move the camera a few centimetres per frame; the jump is the maze walk with a
# step between frames 1 and 2 that shifts the view by more than the narrow windows; the synthetic ones have
# random guides in blocks and random cameras.
SEQUENCES = ("maze4", "corridor", "maze4_jump", "synthetic")
VIEW = {"maze4": (160, 120), "maze4_jump": (160, 120), "corridor": (140, 48)}
STEP = {"maze4": (0.013, 0.021), "maze4_jump": (0.013, 0.021), "corridor": (0.004, 0.05)}  # x, z per frame
JUMP = 8.0  # added to x from frame 2 on: the 1x1 and the 3x40 window lose every pixel, the others a part
# (x0, y0) of the windows: tests/test_gpu_denoise.py's ORIGIN (test_temporal.py checks that they still agree)
ORIGIN = {"maze4": {(67, 5): (40, 54), (64, 1): (50, 61), (1, 1): (80, 63), (3, 40): (78, 40), (130, 9): (15, 50)},
          "corridor": {(67, 5): (40, 18), (64, 1): (50, 25), (1, 1): (70, 25), (3, 40): (70, 4), (130, 9): (6, 16)}}
ORIGIN["maze4_jump"] = ORIGIN["maze4"]
SYN_ORIGIN = (7, 3)  # the synthetic window's origin inside a view 20 x 10 larger than it


def build_ref(tmp_dir) -> C.CDLL:
    """Compile tests/temporal_ref.c into tmp_dir with the oracle Makefile's
    CFLAGS (as denoise_support.build_ref does) and bind it."""
    mk = (REPO / "oracle" / "Makefile").read_text()
    cflags = re.search(r"^CFLAGS\s*:=\s*(.*)$", mk, flags=re.M).group(1).split()
    so = Path(tmp_dir) / "libtemporal_ref.so"
    subprocess.run(["gcc", *cflags, "-shared", "-o", str(so), str(HERE / "temporal_ref.c"), "-lm"], check=True)
    L = C.CDLL(str(so))
    P, U, F = C.c_void_p, C.c_uint32, C.c_float
    L.tpref_accumulate.argtypes = [F, F, P, P, P, P, P, P, P, P, P, P, U, F, F, U, U, U, U, U, P, P]
    assert L.tpref_n_counts() == len(COUNTS)
    return L


def _guides(g, n, h, w):
    nd = np.ascontiguousarray(g["normal_depth"], dtype=np.float32).reshape(n, h, w, 4)
    al = np.ascontiguousarray(g["albedo"], dtype=np.float32).reshape(n, h, w, 4)
    ids = np.ascontiguousarray(np.asarray(g["id"]).view(np.uint32)).reshape(n, h, w)
    return nd, al, ids


def accumulate_ref(L, view, cams, color, guides, prev=None, n_max=32, tol_z=0.02, w_min=0.25, x0=0, y0=0):
    """(accumulated (n, h, w, 4) float32, dict of the call's counts): `view` =
    (view_w, view_h); `cams` (n, 10) float32; `color` (n, h, w, 4); `guides`
    {"normal_depth", "albedo", "id"}; `prev` None or (color (h, w, 4), guides
    of one frame, camera (10,))."""
    color = np.ascontiguousarray(color, dtype=np.float32)
    n, h, w, _ = color.shape
    cams = np.ascontiguousarray(cams, dtype=np.float32).reshape(n, 10)
    nd, al, ids = _guides(guides, n, h, w)
    pp = [None] * 5
    if prev is not None:
        pc = np.ascontiguousarray(prev[0], dtype=np.float32).reshape(h, w, 4)
        pnd, pal, pid = _guides(prev[1], 1, h, w)
        pcam = np.ascontiguousarray(prev[2], dtype=np.float32).reshape(10)
        keep = (pc, pnd, pal, pid, pcam)
        pp = [a.ctypes.data for a in keep]
    out = np.zeros_like(color)
    cnt = np.zeros(len(COUNTS), np.uint64)
    rc = L.tpref_accumulate(view[0], view[1], cams.ctypes.data, color.ctypes.data, nd.ctypes.data, al.ctypes.data,
                            ids.ctypes.data, *pp, n_max, tol_z, w_min, n, x0, y0, w, h, out.ctypes.data, cnt.ctypes.data)
    assert rc == 0, rc
    return out, dict(zip(COUNTS, (int(x) for x in cnt)))


def scene_view(name):
    """(Scene, uniform) of a scene sequence at its view."""
    return (D.corridor_view if name == "corridor" else D.maze_view)(*VIEW[name])


def scene_cameras(name, n=N_FRAMES, step=None):
    """The (n, 10) float32 cameras of a scene sequence: the view's camera moved
    by STEP per frame (and by JUMP from frame 2 on in the jump sequence)."""
    _, u = scene_view(name)
    cams = np.tile(np.frombuffer(bytes(u.cam), dtype=np.float32), (n, 1))
    sx, sz = STEP[name] if step is None else step
    f = np.arange(n, dtype=np.float32)
    cams[:, 0] += np.float32(sx) * f
    cams[:, 2] += np.float32(sz) * f
    if name == "maze4_jump":
        cams[2:, 0] += np.float32(JUMP)
    return cams


def synthetic_view(shape):
    return (float(shape[0] + 20), float(shape[1] + 10))


def synthetic(shape, seed=None):
    """(cams (4, 10), color, guides) of a synthetic sequence over a w x h
    window: frame 0's guides are denoise_support.synthetic's; every later
    frame keeps them except inside random blocks, where it draws its own, so
    history taps meet every rejection.  Distances also hold NaN (and 1e30, from
    denoise_support).  The cameras look down +z from near the origin, a few
    millimetres apart at random; the last one looks the other way, so every
    point it sees is behind the camera of the frame before."""
    w, h = shape
    seed = w * 1000 + h if seed is None else seed
    rng = np.random.default_rng(seed + 77)
    color, g = D.synthetic(N_FRAMES, h, w, seed=seed)
    own = rng.integers(0, 4, size=(N_FRAMES, -(-h // 3), -(-w // 8))) == 0
    own = np.repeat(np.repeat(own, 3, axis=1), 8, axis=2)[:, :h, :w]
    own[0] = True
    out = {}
    for k in NAMES:
        a = np.array(g[k])
        m = own if a.ndim == 3 else own[..., None]
        out[k] = np.ascontiguousarray(np.where(m, a, a[:1]))
    z = out["normal_depth"][..., 3]
    z[rng.integers(0, 40, size=z.shape) == 0] = np.nan
    vw, vh = synthetic_view(shape)
    cams = np.zeros((N_FRAMES, 10), np.float32)
    cams[:, 3] = 1.0                               # focal
    cams[:, 7] = 1.0                               # quat (0, 0, 0, 1)
    cams[:, 8:10] = (2.0 * vw / vh, 2.0)           # viewport
    cams[:, 0:3] = rng.uniform(-0.004, 0.004, size=(N_FRAMES, 3)).astype(np.float32)
    cams[3, 4:8] = (0.0, 1.0, 0.0, 0.0)            # half a turn about y: looks down -z
    return cams, color, out


def mse_ratio(a, raw, truth):
    return D.mse_ratio(a, raw, truth)
