"""Shared by tests/test_upsample.py and tests/test_gpu_upsample.py: the CPU
reference of mm_upsample_frames and mm_fill_pixels (tests/upsample_ref.c, a
plain C statement of the arithmetic in include/mm_api.h) and the inputs both
files upsample."""
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
COUNTS = ("lattice", "tap_outside", "tap_zero", "rej_id", "rej_mh", "rej_normal", "taken", "hole_w", "hole_failed",
          "from_1", "from_2", "from_3", "from_4")
FAILED = 0xFFFFFFFE
SCALES = (2, 4, 8)
W_MINS = (0.25, 0.5, 1.0)
N_FRAMES = (1, 3)
# (w, h) of the synthetic GPU cases: partial waves over two block rows; one whole wave in one row; one pixel;
# narrower than a lattice step of 4 or 8; three waves per row with a ragged right edge, three block rows
SHAPES = D.SHAPES
# the scene cases: the whole view; scales 2 and 4 divide both, and 8 divides the views the premise tests add
VIEW = {"maze4": (160, 120), "corridor": (140, 48)}
VIEW8 = {"maze4": (160, 120), "corridor": (136, 48)}  # (140 is no multiple of 8)
SCENE_SCALES = (2, 4)
MIRROR_LIMIT = 8
SPP = 8


def build_ref(tmp_dir) -> C.CDLL:
    """Compile tests/upsample_ref.c into tmp_dir with the oracle Makefile's
    CFLAGS (as temporal_support.build_ref does) and bind it."""
    mk = (REPO / "oracle" / "Makefile").read_text()
    cflags = re.search(r"^CFLAGS\s*:=\s*(.*)$", mk, flags=re.M).group(1).split()
    so = Path(tmp_dir) / "libupsample_ref.so"
    subprocess.run(["gcc", *cflags, "-shared", "-o", str(so), str(HERE / "upsample_ref.c"), "-lm"], check=True)
    L = C.CDLL(str(so))
    P, U, F = C.c_void_p, C.c_uint32, C.c_float
    L.upref_upsample.argtypes = [P, P, P, P, P, U, F, U, U, U, P, P, P, P]
    L.upref_fill.argtypes = [P, P, P, U, U, U, U, P, P, P, C.c_uint64, F]
    L.upref_fill.restype = C.c_uint64
    assert L.upref_n_counts() == len(COUNTS)
    return L


def lattice_shape(w, h, s):
    return -(-w // s), -(-h // s)


def upsample_ref(L, low, guides, scale, w_min=0.25, low_vmean=None, want_weight=True):
    """(color (n, h, w, 4), weight (n, h, w) or None, var (n, h, w) or None,
    dict of the call's counts): `low` (n, lh, lw, 4) or (lh, lw, 4); `guides`
    {"normal_depth", "albedo", "id"} of the full-resolution frames; `low_vmean`
    None or low's shape without the last axis."""
    low = np.ascontiguousarray(low, dtype=np.float32)
    if low.ndim == 3:
        low = low[None]
    n, lh, lw, _ = low.shape
    ids = np.ascontiguousarray(np.asarray(guides["id"]).view(np.uint32))
    h, w = ids.shape[-2:]
    assert lattice_shape(w, h, scale) == (lw, lh), (w, h, scale, lw, lh)
    ids = ids.reshape(n, h, w)
    nd = np.ascontiguousarray(guides["normal_depth"], dtype=np.float32).reshape(n, h, w, 4)
    al = np.ascontiguousarray(guides["albedo"], dtype=np.float32).reshape(n, h, w, 4)
    vm = None if low_vmean is None else np.ascontiguousarray(low_vmean, dtype=np.float32).reshape(n, lh, lw)
    out = np.full((n, h, w, 4), np.nan, np.float32)
    wt = np.full((n, h, w), np.nan, np.float32) if want_weight else None
    vo = None if vm is None else np.full((n, h, w), np.nan, np.float32)
    cnt = np.zeros(len(COUNTS), np.uint64)
    rc = L.upref_upsample(low.ctypes.data, nd.ctypes.data, al.ctypes.data, ids.ctypes.data,
                          None if vm is None else vm.ctypes.data, scale, w_min, n, w, h, out.ctypes.data,
                          None if wt is None else wt.ctypes.data, None if vo is None else vo.ctypes.data,
                          cnt.ctypes.data)
    assert rc == 0, rc
    return out, wt, vo, dict(zip(COUNTS, (int(x) for x in cnt)))


def fill_ref(L, image, var, weight, x0, y0, pixels, extra, extra_vmean, m):
    """(filled copies of `image` (h, w, 4), `var` and `weight` ((h, w) or
    None), entries inside the window)."""
    out = np.array(image, dtype=np.float32, order="C")
    vo = None if var is None else np.array(var, dtype=np.float32, order="C")
    wo = None if weight is None else np.array(weight, dtype=np.float32, order="C")
    h, w, _ = out.shape
    px = np.ascontiguousarray(pixels, dtype=np.uint32)
    ex = np.ascontiguousarray(extra, dtype=np.float32)
    ev = None if extra_vmean is None else np.ascontiguousarray(extra_vmean, dtype=np.float32)
    n = L.upref_fill(out.ctypes.data, None if vo is None else vo.ctypes.data, None if wo is None else wo.ctypes.data,
                     x0, y0, w, h, px.ctypes.data, ex.ctypes.data, None if ev is None else ev.ctypes.data, px.shape[0], m)
    return out, vo, wo, int(n)


def synthetic(shape, scale, n, seed=None):
    """(low (n, lh, lw, 4), guides, low_vmean (n, lh, lw)) of a synthetic case
    over a w x h window: denoise_support.synthetic's guides -- ids, mirror
    hits and normals in blocks a few pixels wide, so a pixel's four taps meet
    every rejection -- with one id in 40 replaced by MM_AOV_ID_FAILED; random
    lattice colours; variances in [0, 1) salted with exact zeros, 1e-40 and
    1e-44 (subnormals) and 1e30."""
    w, h = shape
    seed = (w * 1000 + h) * 10 + scale if seed is None else seed
    rng = np.random.default_rng(seed + 313)
    _, g = D.synthetic(n, h, w, seed=seed)
    g = {k: np.array(g[k]) for k in NAMES}
    g["id"][rng.integers(0, 40, size=g["id"].shape) == 0] = np.uint32(FAILED)
    lw, lh = lattice_shape(w, h, scale)
    low = rng.uniform(0.0, 2.0, size=(n, lh, lw, 4)).astype(np.float32)
    low[..., 3] = 1.0
    v = rng.uniform(0.0, 1.0, size=(n, lh, lw)).astype(np.float32)
    salt = rng.integers(0, 12, size=v.shape)
    v[salt == 0] = np.float32(0.0)
    v[salt == 1] = np.float32(1e-40)
    v[salt == 2] = np.float32(1e30)
    v[salt == 3] = np.float32(1e-44)
    return np.ascontiguousarray(low), {k: np.ascontiguousarray(a) for k, a in g.items()}, np.ascontiguousarray(v)


def scene_view(name, view=None):
    """(Scene, uniform) of a scene case at its view."""
    w, h = VIEW[name] if view is None else view
    return (D.corridor_view if name == "corridor" else D.maze_view)(w, h)


def low_uniform(u, scale):
    """The uniform of the (view / scale) view: the same camera."""
    from mirror_maze import _lib

    lo = _lib.mm_uniform.from_buffer_copy(bytes(u))
    assert int(u.view_w) % scale == 0 and int(u.view_h) % scale == 0
    lo.view_w, lo.view_h = float(int(u.view_w) // scale), float(int(u.view_h) // scale)
    return lo


def holes_of(weight):
    """The (n, 2) uint32 (x, y) list of one frame's holes, row-major."""
    j, i = np.nonzero(np.asarray(weight) == 0)
    return np.ascontiguousarray(np.stack([i, j], axis=1).astype(np.uint32))


def mse_ratio(a, raw, truth):
    return D.mse_ratio(a, raw, truth)
