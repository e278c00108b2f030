"""mm_accumulate_frames, host side (no GPU): the C-ABI symbol and its argument
checks, the structs' layout, the reference accumulation (tests/temporal_ref.c)
judged against a converged frame, its chaining property, and the input
conditions the GPU cases (tests/test_gpu_temporal.py) rely on."""
from __future__ import annotations

import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import aov_support as A
import denoise_support as D
import temporal_support as T
from conftest import oracle_tile

REPO = Path(__file__).resolve().parent.parent
_CACHE = {}


@pytest.fixture(scope="module")
def tp_lib(tmp_path_factory):
    return T.build_ref(tmp_path_factory.mktemp("temporal_ref"))


@pytest.fixture(scope="module")
def dn_lib(tmp_path_factory):
    return D.build_ref(tmp_path_factory.mktemp("denoise_ref"))


@pytest.fixture(scope="module")
def aov_lib(tmp_path_factory):
    return A.build_ref(tmp_path_factory.mktemp("aov_ref"))


def _view_guides(aov_lib, scene, u, cams, w, h):
    """aov_ref.c's guides of the whole w x h view for every camera, stacked."""
    ref = A.Ref(aov_lib, scene)
    gs = []
    for cam in cams:
        C.memmove(C.byref(u), np.ascontiguousarray(cam, dtype=np.float32).ctypes.data, 40)
        gs.append(ref.tile(u, T.MIRROR_LIMIT, 0, 0, w, h))
    return {k: np.stack([g[k] for g in gs]) for k in T.NAMES}


def _sequence(aov_lib, name):
    """(view, cams, color, guides) of a whole-view sequence: guides from
    aov_ref.c (what mm_trace_aov writes), colours at random (no count and no
    decision of the accumulation depends on a colour); built once, read-only."""
    if name not in _CACHE:
        s, u = T.scene_view(name)
        vw, vh = T.VIEW[name]
        cams = T.scene_cameras(name)
        g = _view_guides(aov_lib, s, u, cams, vw, vh)
        color = np.random.default_rng(len(name)).uniform(0, 1, size=(T.N_FRAMES, vh, vw, 4)).astype(np.float32)
        for a in (cams, color, *g.values()):
            a.setflags(write=False)
        _CACHE[name] = ((vw, vh), cams, color, g)
    return _CACHE[name]


def _window(seq, x0, y0, w, h):
    view, cams, color, g = seq
    return (view, cams, np.ascontiguousarray(color[:, y0:y0 + h, x0:x0 + w]),
            {k: np.ascontiguousarray(g[k][:, y0:y0 + h, x0:x0 + w]) for k in T.NAMES})


def _add(total, cnt):
    for k, v in cnt.items():
        total[k] = total.get(k, 0) + v


def test_symbol_exists_and_rejects_bad_arguments_without_a_gpu():
    """The argument checks need no context, so they run here: every call below
    returns MM_ERR_INVALID before anything touches a device."""
    from mirror_maze import _lib

    L = _lib.lib()
    assert "mm_accumulate_frames" in _lib.EXPORTS
    inv = _lib.MM_ERR_INVALID
    buf = (C.c_float * 128)()  # 16-byte aligned stand-ins; never dereferenced
    base = (C.addressof(buf) + 15) & ~15
    col, nd, al, ids, out, pcol, pnd, pal, pid = (base + 16 * i for i in range(9))
    uni = _lib.mm_uniform()
    uni.view_w, uni.view_h = 8.0, 8.0
    cams = (_lib.mm_camera * 1)()
    good = dict(uni=uni, cams=cams, col=col, aov=_lib.mm_aov(nd, al, ids), prev=None,
                p=_lib.mm_temporal_params(32, 0.02, 0.25, 0), n=1, x0=0, y0=0, w=1, h=1, out=out)

    def call(**kw):
        a = {**good, **kw}
        ref = lambda v: None if v is None else C.byref(v)  # noqa: E731
        return L.mm_accumulate_frames(None, ref(a["uni"]), a["cams"], a["col"], ref(a["aov"]), ref(a["prev"]),
                                      ref(a["p"]), a["n"], a["x0"], a["y0"], a["w"], a["h"], a["out"])

    # with everything in order the null context is what is left to refuse
    assert call() == inv
    # null arguments, by name; a null in the guides; a null in prev
    for name in ("uni", "cams", "col", "aov", "p", "out"):
        assert call(**{name: None}) == inv, name
    for hole in range(3):
        g = [nd, al, ids]
        g[hole] = None
        assert call(aov=_lib.mm_aov(*g)) == inv
    for hole in range(4):
        q = [pcol, pnd, pal, pid]
        q[hole] = None
        assert call(prev=_lib.mm_temporal_prev(q[0], _lib.mm_aov(*q[1:]), cams[0])) == inv
    # parameters out of range
    nan = float("nan")
    for bad in ((0, 0.02, 0.25, 0), (65536, 0.02, 0.25, 0), (32, 0.0, 0.25, 0), (32, -0.02, 0.25, 0), (32, nan, 0.25, 0),
                (32, float("inf"), 0.25, 0), (32, 0.02, 0.0, 0), (32, 0.02, 1.5, 0), (32, 0.02, nan, 0),
                (32, 0.02, 0.25, 1), (32, 0.02, 0.25, 0x80000000)):
        assert call(p=_lib.mm_temporal_params(*bad)) == inv, bad
    # empty shapes, misaligned pointers, overlap, windows beyond 2^24, too many pixels
    for kw in (dict(n=0), dict(w=0), dict(h=0), dict(col=col + 4), dict(out=out + 8), dict(aov=_lib.mm_aov(nd + 4, al, ids)),
               dict(aov=_lib.mm_aov(nd, al + 8, ids)), dict(aov=_lib.mm_aov(nd, al, ids + 2)),
               dict(prev=_lib.mm_temporal_prev(pcol + 4, _lib.mm_aov(pnd, pal, pid), cams[0])),
               dict(prev=_lib.mm_temporal_prev(pcol, _lib.mm_aov(pnd, pal, pid + 1), cams[0])),
               dict(out=col), dict(out=nd), dict(out=al), dict(out=ids),
               dict(prev=_lib.mm_temporal_prev(out, _lib.mm_aov(pnd, pal, pid), cams[0])),
               dict(prev=_lib.mm_temporal_prev(pcol, _lib.mm_aov(pnd, out, pid), cams[0])),
               dict(x0=(1 << 24)), dict(y0=(1 << 24) - 1, h=2), dict(w=1 << 16, h=1 << 15), dict(w=1 << 12, h=1 << 12, n=1 << 17)):
        assert call(**kw) == inv, kw


def test_struct_layouts_match_the_header():
    from mirror_maze import _lib

    txt = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "mm_types.h").read_text(), flags=re.S)
    body = re.search(r"typedef struct mm_temporal_params \{(.*?)\} mm_temporal_params;", txt, flags=re.S).group(1)
    fields = re.findall(r"(\w+)\s+(\w+)\s*;", body)
    assert fields == [("uint32_t", "n_max"), ("float", "tol_z"), ("float", "w_min"), ("uint32_t", "flags")]
    assert [n for n, _ in _lib.mm_temporal_params._fields_] == [f[1] for f in fields]
    assert C.sizeof(_lib.mm_temporal_params) == 16
    body = re.search(r"typedef struct mm_temporal_prev \{(.*?)\} mm_temporal_prev;", txt, flags=re.S).group(1)
    fields = re.findall(r"([\w ]+?\*?)\s+(\w+)\s*;", body)
    assert [(t.strip(), n) for t, n in fields] == [("const float*", "color"), ("mm_aov", "guides"), ("mm_camera", "cam")]
    assert [n for n, _ in _lib.mm_temporal_prev._fields_] == ["color", "guides", "cam"]
    assert C.sizeof(_lib.mm_temporal_prev) == 72 and _lib.mm_temporal_prev.cam.offset == 32
    check = (REPO / "mirror-maze_amd" / "csrc" / "mm_layout_check.cpp").read_text()
    assert "sizeof(mm_temporal_params) == 16" in check and "sizeof(mm_temporal_prev) == 72" in check


def test_windows_are_the_denoise_tests():
    import test_gpu_denoise as G

    for name in ("maze4", "corridor"):
        assert T.VIEW[name] == G.VIEW[name]
        assert {k: v[:2] for k, v in G.ORIGIN[name].items()} == T.ORIGIN[name]
    assert sorted(T.ORIGIN["maze4"]) == sorted(D.SHAPES)


def test_gpu_case_inputs_keep_every_outcome_busy(tp_lib, aov_lib):
    """Input conditions of tests/test_gpu_temporal.py, on the reference alone.
    Over its cases every outcome of a pixel and of a tap is counted; in the
    two walks at least half of the non-miss pixels of every frame after the
    first are blended (whole view), the corridor's through 1..7 mirrors too;
    the jump leaves the 1x1 and the 3x40 window behind entirely."""
    total = {}
    for name in T.SEQUENCES:
        for shape in D.SHAPES:
            w, h = shape
            if name == "synthetic":
                cams, color, g = T.synthetic(shape)
                view, (x0, y0) = T.synthetic_view(shape), T.SYN_ORIGIN
            else:
                x0, y0 = T.ORIGIN[name][shape]
                view, cams, color, g = _window(_sequence(aov_lib, name), x0, y0, w, h)
            two, _ = T.accumulate_ref(tp_lib, view, cams[:2], color[:2], {k: g[k][:2] for k in T.NAMES}, x0=x0, y0=y0)
            prev = (two[1], {k: g[k][1:2] for k in T.NAMES}, cams[1])
            for n_max in T.N_MAX:
                for pv in (None, prev):
                    _, cnt = T.accumulate_ref(tp_lib, view, cams, color, g, prev=pv, n_max=n_max, x0=x0, y0=y0)
                    _add(total, cnt)
            if name == "maze4_jump" and shape in ((1, 1), (3, 40)):
                _, cnt = T.accumulate_ref(tp_lib, view, cams[1:3], color[1:3], {k: g[k][1:3] for k in T.NAMES}, x0=x0, y0=y0)
                assert cnt["blended"] == 0 and cnt["out_of_window"] + cnt["miss"] == w * h and cnt["out_of_window"] > 0
    print("all GPU cases:", total)
    assert all(total[k] > 0 for k in T.COUNTS), total
    assert all(total[k] >= 1000 for k in T.COUNTS if k != "rej_normal"), total
    for name in ("maze4", "corridor"):
        view, cams, color, g = _sequence(aov_lib, name)
        out, cnt = T.accumulate_ref(tp_lib, view, cams, color, g, **T.DEFAULTS)
        ids = g["id"].view(np.uint32)
        for f in range(1, T.N_FRAMES):
            hit = ids[f] < 0xFFFFFFFE
            share = float((out[f][..., 3] > 1.0)[hit].mean())
            print(name, "frame", f, "blended share of the non-miss pixels", share)
            assert share >= 0.5, (name, f, share)
            assert not (out[f][..., 3] > 1.0)[~hit].any()
        if name == "corridor":
            blended = out[1:][..., 3] > 1.0
            assert set(np.unique(g["albedo"][1:][..., 3][blended])) >= {1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0}
        # the history grows by one per frame (N is interpolated like a colour: equal to the frame count to rounding)
        assert abs(float(out[T.N_FRAMES - 1][..., 3].max()) - T.N_FRAMES) < 1e-5


def test_chaining_and_frame_zero(tp_lib, aov_lib):
    """Frames 0..3 in one call equal frames 0..1, then frames 2..3 with prev
    taken from frame 1, bit for bit; frame 0 without prev is (C.rgb, 1)."""
    for name in T.SEQUENCES:
        if name == "synthetic":
            shape = (130, 9)
            cams, color, g = T.synthetic(shape)
            view, (x0, y0) = T.synthetic_view(shape), T.SYN_ORIGIN
        else:
            view, cams, color, g = _sequence(aov_lib, name)
            x0 = y0 = 0
        for n_max in (3, 32):
            whole, _ = T.accumulate_ref(tp_lib, view, cams, color, g, n_max=n_max, x0=x0, y0=y0)
            head, _ = T.accumulate_ref(tp_lib, view, cams[:2], color[:2], {k: g[k][:2] for k in T.NAMES}, n_max=n_max,
                                       x0=x0, y0=y0)
            tail, _ = T.accumulate_ref(tp_lib, view, cams[2:], color[2:], {k: g[k][2:] for k in T.NAMES},
                                       prev=(head[1], {k: g[k][1:2] for k in T.NAMES}, cams[1]), n_max=n_max, x0=x0, y0=y0)
            assert np.array_equal(whole.view(np.uint32), np.concatenate([head, tail]).view(np.uint32)), (name, n_max)
            assert np.array_equal(whole[0][..., :3].view(np.uint32), color[0][..., :3].view(np.uint32))
            assert (whole[0][..., 3] == 1.0).all() and (whole[..., 3] >= 1.0).all() and whole[..., 3].max() <= n_max
        assert whole[..., 3].max() > 1.0, name


def _walk(aov_lib, scene, u, w, h, n=8):
    """(8-spp frames of an n-frame slow walk, their guides, the cameras, a
    512-spp frame of the last camera) of the whole w x h view from the oracle
    and aov_ref.c."""
    from mirror_maze import make_ext
    from oracle.oracle import Oracle

    o = Oracle.from_scene(scene)
    cams = np.tile(np.frombuffer(bytes(u.cam), dtype=np.float32), (n, 1))
    cams[:, 0] += np.float32(0.013) * np.arange(n, dtype=np.float32)
    cams[:, 2] += np.float32(0.021) * np.arange(n, dtype=np.float32)
    frames = []
    for f in range(n):
        C.memmove(C.byref(u), cams[f].ctypes.data, 40)
        frames.append(oracle_tile(o, u, make_ext(8, 8, T.MIRROR_LIMIT, frame=f), 0, 0, w, h)[0])
    truth, _ = oracle_tile(o, u, make_ext(512, 8, T.MIRROR_LIMIT, frame=n), 0, 0, w, h)
    return np.stack(frames), _view_guides(aov_lib, scene, u, cams, w, h), cams, truth


@pytest.mark.parametrize("name,view", [("maze4", (160, 120)), ("corridor", (140, 32))])
def test_reference_accumulation_beats_the_raw_frame(tp_lib, dn_lib, aov_lib, name, view):
    """Eight 8-spp frames of a slow walk, accumulated with the defaults: MSE of
    the last accumulated frame / MSE of the last raw frame against a 512-spp
    frame of the last camera, and the same after the reference denoiser on
    both.  Where the history is valid throughout the ideal is 1/8.
    Measured: maze 0.112 accumulated, 0.0157 accumulated + denoised (0.0183
    denoised alone); corridor 0.171, 0.130 (0.116 denoised alone: there the
    denoiser's own bias is what is left, and the history cannot remove it).
    Both accumulated ratios are at most 0.25, so the bound is the denoiser
    test's 0.5."""
    w, h = view
    s, u = D.maze_view(w, h) if name == "maze4" else D.corridor_view(w, h)
    frames, guides, cams, truth = _walk(aov_lib, s, u, w, h)
    acc, cnt = T.accumulate_ref(tp_lib, (w, h), cams, frames, guides, **T.DEFAULTS)
    ratio = T.mse_ratio(acc[-1], frames[-1], truth)
    last = {k: guides[k][-1:] for k in T.NAMES}
    dn_acc, _ = D.filter_ref(dn_lib, acc[-1], last, **D.DEFAULTS)
    dn_raw, _ = D.filter_ref(dn_lib, frames[-1], last, **D.DEFAULTS)
    ratio_dn = T.mse_ratio(dn_acc[0], frames[-1], truth)
    ratio_dn_raw = T.mse_ratio(dn_raw[0], frames[-1], truth)
    print(name, view, "MSE ratio accumulated", ratio, "accumulated + denoised", ratio_dn, "denoised alone", ratio_dn_raw,
          "history length mean", float(acc[-1][..., 3].mean()), cnt)
    assert np.isfinite(acc).all()
    assert ratio < 0.5, ratio
    assert ratio_dn < 0.5, ratio_dn


def test_flythrough_accumulate_argument(capsys):
    """--accumulate parses (alone and with --denoise); with --no-render nothing
    is rendered or written, and the camera path is printed as before."""
    import importlib.util
    import sys

    path0 = list(sys.path)
    try:
        spec = importlib.util.spec_from_file_location("flythrough_acc", REPO / "scripts" / "flythrough.py")
        fly = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(fly)
        for extra in ([], ["--denoise"]):
            rc = fly.main(["--maze", "4", "--frames", "3", "--width", "64", "--height", "48", "--accumulate",
                           "--no-render", *extra])
            assert rc == 0
            assert len([ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("frame ")]) == 3
        assert "--accumulate" in (REPO / "scripts" / "flythrough.py").read_text()
    finally:
        sys.path[:] = path0
