"""Shared by tests/test_denoise.py and tests/test_gpu_denoise.py: the CPU
reference of mm_denoise_frames (tests/denoise_ref.c, a plain C statement of the
filter in include/mm_api.h) and the inputs the tests filter."""
from __future__ import annotations

import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
REPO = HERE.parent
MISS = 0xFFFFFFFF
COUNTS = ("out_of_tile", "rej_id", "rej_mh", "rej_normal", "soft_z", "soft_l", "taken")
DEFAULTS = dict(n_passes=4, sigma_z=0.02, sigma_l=0.5)
# (w, h) of the GPU cases: a ragged last wave over more than one block row; one whole wave; one pixel; narrower
# than the taps' reach at every pass; three waves per row, the last ragged, three block rows
SHAPES = [(67, 5), (64, 1), (1, 1), (3, 40), (130, 9)]
PASSES = [1, 2, 3, 4, 5, 8]


def build_ref(tmp_dir) -> C.CDLL:
    """Compile tests/denoise_ref.c into tmp_dir with the oracle Makefile's
    CFLAGS (as aov_support.build_ref does) and bind it."""
    mk = (REPO / "oracle" / "Makefile").read_text()
    cflags = re.search(r"^CFLAGS\s*:=\s*(.*)$", mk, flags=re.M).group(1).split()
    so = Path(tmp_dir) / "libdenoise_ref.so"
    subprocess.run(["gcc", *cflags, "-shared", "-o", str(so), str(HERE / "denoise_ref.c"), "-lm"], check=True)
    L = C.CDLL(str(so))
    P = C.c_void_p
    L.dnref_filter.argtypes = [P, P, P, P, C.c_uint32, C.c_float, C.c_float, C.c_uint32, C.c_uint32, C.c_uint32, P, P]
    assert L.dnref_n_counts() == len(COUNTS)
    return L


def filter_ref(L, color, guides, n_passes=4, sigma_z=0.02, sigma_l=0.5):
    """(filtered (n, h, w, 4) float32, dict of the call's tap counts) of
    `color` (h, w, 4) or (n, h, w, 4) with guides {"normal_depth", "albedo",
    "id"} of matching shapes."""
    color = np.ascontiguousarray(color, dtype=np.float32)
    if color.ndim == 3:
        color = color[None]
    n, h, w, _ = color.shape
    nd = np.ascontiguousarray(guides["normal_depth"], dtype=np.float32).reshape(n, h, w, 4)
    al = np.ascontiguousarray(guides["albedo"], dtype=np.float32).reshape(n, h, w, 4)
    ids = np.ascontiguousarray(np.asarray(guides["id"]).view(np.uint32)).reshape(n, h, w)
    out = np.zeros_like(color)
    cnt = np.zeros(len(COUNTS), np.uint64)
    rc = L.dnref_filter(color.ctypes.data, nd.ctypes.data, al.ctypes.data, ids.ctypes.data, n_passes, sigma_z, sigma_l,
                        n, w, h, out.ctypes.data, cnt.ctypes.data)
    assert rc == 0, rc
    return out, dict(zip(COUNTS, (int(x) for x in cnt)))


def synthetic(n, h, w, seed):
    """(color, guides) made to keep every clause of the filter busy: ids from
    a set of 5 with MISS among them, in blocks a few pixels wide; mirror hits
    0..2; normals +-axis; distances from 0.2 to 1e30; colours whose
    luminance steps between neighbours span the luminance term's range."""
    rng = np.random.default_rng(seed)

    def blocks(values, by, bx):
        """A field that is constant over by x bx blocks (edges every few pixels)."""
        gh, gw = -(-h // by) + 1, -(-w // bx) + 1
        g = rng.integers(0, len(values), size=(n, gh, gw))
        g = np.repeat(np.repeat(g, by, axis=1), bx, axis=2)
        oy, ox = rng.integers(0, by), rng.integers(0, bx)
        return np.asarray(values)[g[:, oy:oy + h, ox:ox + w]]

    ids = blocks(np.uint32([3 | 1 << 30, 7 | 1 << 30, 7 | 2 << 30, 0x00ABCDEF | 1 << 30, MISS]), 3, 7).astype(np.uint32)
    mh = blocks(np.float32([0, 0, 0, 1, 2]), 4, 9).astype(np.float32)
    axes = np.float32([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [1, 0, 0], [1, 0, 0]])
    nrm = axes[blocks(np.arange(len(axes)), 5, 11)]
    z = blocks(np.float32([0.2, 0.2, 0.21, 0.5, 3.0, 3.05, 250.0, 1e30]), 2, 5).astype(np.float32)
    z = (z * rng.uniform(0.995, 1.005, size=z.shape).astype(np.float32)).astype(np.float32)
    nd = np.concatenate([nrm, z[..., None]], axis=-1).astype(np.float32)
    al = np.concatenate([rng.uniform(0, 1, size=(n, h, w, 3)).astype(np.float32), mh[..., None]], axis=-1)
    base = blocks(np.float32([0.05, 0.3, 0.3, 0.9, 2.5]), 6, 13)[..., None]
    color = (base * rng.uniform(0.7, 1.3, size=(n, h, w, 3))).astype(np.float32)
    color = np.concatenate([color, np.ones((n, h, w, 1), np.float32)], axis=-1)
    return np.ascontiguousarray(color), {"normal_depth": np.ascontiguousarray(nd), "albedo": np.ascontiguousarray(al),
                                         "id": np.ascontiguousarray(ids)}


def maze_view(w, h):
    """(Scene, uniform) of the maze N=4 at a w x h view."""
    from mirror_maze import Scene, default_uniform

    return Scene.build(4, 0), default_uniform(w, h, 0)


def corridor_view(w, h):
    """(Scene, uniform) of aov_support's corridor at a w x h view (its camera's
    viewport is as wide as the scene: any aspect shows the mirror chains)."""
    import aov_support as A

    s, u = A.corridor()
    u.view_w, u.view_h = float(w), float(h)
    return s, u


def mse_ratio(filtered, raw, truth):
    """MSE(filtered) / MSE(raw) against truth over rgb, in float64."""
    f, r, t = (np.asarray(a, dtype=np.float64)[..., :3] for a in (filtered, raw, truth))
    return float(((f - t) ** 2).mean() / ((r - t) ** 2).mean())
