"""mm_upsample_frames and mm_fill_pixels, host side (no GPU): the C-ABI symbols
and their argument checks, the struct's layout, the premise that a view traced
at 1/s is the full view's lattice (on tests/aov_ref.c), the reference upsample
(tests/upsample_ref.c) and its properties, the input conditions the GPU cases
(tests/test_gpu_upsample.py) rely on, and the reference judged against a
converged frame."""
from __future__ import annotations

import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import aov_support as A
import upsample_support as U
from conftest import oracle_tile

REPO = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def up_lib(tmp_path_factory):
    return U.build_ref(tmp_path_factory.mktemp("upsample_ref"))


@pytest.fixture(scope="module")
def aov_lib(tmp_path_factory):
    return A.build_ref(tmp_path_factory.mktemp("aov_ref"))


_GUIDES = {}


def _scene_guides(aov_lib, name, view=None):
    """aov_ref.c's guides of a scene case's whole view (what mm_trace_aov
    writes); built once, read-only."""
    key = (name, view)
    if key not in _GUIDES:
        s, u = U.scene_view(name, view)
        w, h = int(u.view_w), int(u.view_h)
        g = A.Ref(aov_lib, s).tile(u, U.MIRROR_LIMIT, 0, 0, w, h)
        for a in g.values():
            a.setflags(write=False)
        _GUIDES[key] = (s, u, g)
    return _GUIDES[key]


def _add(total, cnt):
    for k, v in cnt.items():
        total[k] = total.get(k, 0) + v


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_symbols_exist_and_reject_bad_arguments_without_a_gpu():
    """The argument checks need no context, so they run here: every call below
    returns MM_ERR_INVALID before anything touches a device.  (Which check
    refuses what, with its message: tests/test_upsample_args.py.)"""
    from mirror_maze import _lib

    L = _lib.lib()
    assert "mm_upsample_frames" in _lib.EXPORTS and "mm_fill_pixels" in _lib.EXPORTS
    inv = _lib.MM_ERR_INVALID
    buf = (C.c_float * 256)()  # 16-byte aligned stand-ins; never dereferenced
    base = (C.addressof(buf) + 15) & ~15
    low, nd, al, ids, vm, out, wo, vo = (base + 64 * i for i in range(8))
    good = dict(low=low, aov=_lib.mm_aov(nd, al, ids), vm=vm, p=_lib.mm_upsample_params(2, 0.25, 0, 0), n=1, w=2, h=2,
                out=out, wo=wo, vo=vo)

    def up(**kw):
        a = {**good, **kw}
        ref = lambda v: None if v is None else C.byref(v)  # noqa: E731
        return L.mm_upsample_frames(None, a["low"], ref(a["aov"]), a["vm"], ref(a["p"]), a["n"], a["w"], a["h"],
                                    a["out"], a["wo"], a["vo"])

    assert up() == inv  # with everything in order the null context is what is left to refuse
    assert up(vm=None, vo=None, wo=None) == inv
    for name in ("low", "aov", "p", "out"):
        assert up(**{name: None}) == inv, name
    for hole in range(3):
        g = [nd, al, ids]
        g[hole] = None
        assert up(aov=_lib.mm_aov(*g)) == inv
    nan = float("nan")
    for bad in ((0, 0.25, 0, 0), (1, 0.25, 0, 0), (3, 0.25, 0, 0), (16, 0.25, 0, 0), (2, 0.0, 0, 0), (2, 1.5, 0, 0),
                (2, nan, 0, 0), (2, -0.25, 0, 0), (2, 0.25, 1, 0), (2, 0.25, 0, 1)):
        assert up(p=_lib.mm_upsample_params(*bad)) == inv, bad
    for kw in (dict(n=0), dict(w=0), dict(h=0), dict(low=low + 4), dict(out=out + 8), dict(wo=wo + 2), dict(vo=vo + 1),
               dict(vm=vm + 2), dict(aov=_lib.mm_aov(nd + 4, al, ids)), dict(aov=_lib.mm_aov(nd, al, ids + 2)),
               dict(vm=None), dict(out=low), dict(out=nd), dict(wo=ids), dict(vo=vm), dict(wo=out), dict(vo=wo),
               dict(w=1 << 16, h=1 << 15), dict(w=1 << 12, h=1 << 12, n=1 << 17), dict(w=64, h=4, n=1 << 26)):
        assert up(**kw) == inv, kw

    img, var, wt, px, ex, ev = (base + 64 * i for i in range(6))
    gf = dict(img=img, var=var, wt=wt, x0=0, y0=0, w=2, h=2, px=px, ex=ex, ev=ev, n=2, m=1.0)

    def fill(**kw):
        a = {**gf, **kw}
        return L.mm_fill_pixels(None, a["img"], a["var"], a["wt"], a["x0"], a["y0"], a["w"], a["h"], a["px"], a["ex"],
                                a["ev"], a["n"], a["m"])

    assert fill() == inv
    assert fill(var=None, ev=None, wt=None) == inv
    assert fill(n=0, px=None, ex=None, ev=None) == inv  # (an empty list is in order: the null context is refused)
    for kw in (dict(img=None), dict(w=0), dict(h=0), dict(w=1 << 16, h=1 << 15), dict(m=0.0), dict(m=nan),
               dict(m=float("inf")), dict(img=img + 4), dict(var=var + 2), dict(wt=wt + 1), dict(var=img), dict(wt=var),
               dict(px=None), dict(ex=None), dict(ev=None), dict(var=None), dict(px=px + 4), dict(ex=ex + 8),
               dict(ev=ev + 2), dict(n=(1 << 38) + 1), dict(ex=img), dict(px=var), dict(ev=wt)):
        assert fill(**kw) == inv, kw


def test_struct_layout_matches_the_header():
    from mirror_maze import _lib

    txt = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "mm_types.h").read_text(), flags=re.S)
    body = re.search(r"typedef struct mm_upsample_params \{(.*?)\} mm_upsample_params;", txt, flags=re.S).group(1)
    fields = re.findall(r"(\w+)\s+(\w+)\s*;", body)
    assert fields == [("uint32_t", "scale"), ("float", "w_min"), ("uint32_t", "flags"), ("uint32_t", "reserved")]
    assert [n for n, _ in _lib.mm_upsample_params._fields_] == [f[1] for f in fields]
    assert C.sizeof(_lib.mm_upsample_params) == 16 and _lib.mm_upsample_params.w_min.offset == 4
    check = (REPO / "mirror-maze_amd" / "csrc" / "mm_layout_check.cpp").read_text()
    assert "sizeof(mm_upsample_params) == 16" in check


@pytest.mark.parametrize("name", ["maze4", "corridor"])
@pytest.mark.parametrize("scale", U.SCALES)
def test_low_view_is_the_full_views_lattice(aov_lib, name, scale):
    """The premise: aov_ref.c's three buffers of the (view / s) view equal the
    full view's [::s, ::s] on all bits -- primary_dir has no half-pixel offset
    and s is a power of two.  (s = 8: the corridor at 136 x 48, since 140 is no
    multiple of 8.)"""
    view = U.VIEW8[name] if scale == 8 else U.VIEW[name]
    s, u, full = _scene_guides(aov_lib, name, view)
    w, h = view
    lo = A.Ref(aov_lib, s).tile(U.low_uniform(u, scale), U.MIRROR_LIMIT, 0, 0, w // scale, h // scale)
    for k in U.NAMES:
        assert np.array_equal(_bits(lo[k]), _bits(full[k][::scale, ::scale])), (name, scale, k)
    assert len(np.unique(full["id"])) > 1  # (more than one surface in view)


def test_reference_properties(up_lib):
    """Lattice pixels return low, vmean and weight 1 on all bits; weight is 0
    or in [1, 4]; a hole is all zeros; with every guide equal and low an affine
    function of (X, Y) with small-integer values the output is that function
    exactly."""
    for shape in U.SHAPES:
        for scale in U.SCALES:
            low, g, vm = U.synthetic(shape, scale, 3)
            for w_min in U.W_MINS:
                out, wt, vo, cnt = U.upsample_ref(up_lib, low, g, scale, w_min, vm)
                assert not np.isnan(out).any() and not np.isnan(wt).any() and not np.isnan(vo).any()
                lat = g["id"][:, ::scale, ::scale] != U.FAILED
                assert np.array_equal(_bits(out[:, ::scale, ::scale][lat][:, :3]), _bits(low[lat][:, :3]))
                assert np.array_equal(_bits(vo[:, ::scale, ::scale][lat]), _bits(vm[lat]))
                assert (wt[:, ::scale, ::scale][lat] == 1.0).all() and (out[:, ::scale, ::scale][lat][:, 3] == 1.0).all()
                hole = wt == 0
                assert ((wt >= 1.0) & (wt <= 4.0) | hole).all()
                assert (out[hole] == 0).all() and (vo[hole] == 0).all() and (out[~hole][:, 3] == 1.0).all()
                assert hole[g["id"] == U.FAILED].all()
                assert cnt["hole_w"] + cnt["hole_failed"] == int(hole.sum())
                # without the optional buffers the colour is the same
                plain, none_w, none_v, _ = U.upsample_ref(up_lib, low, g, scale, w_min, None, want_weight=False)
                assert none_w is None and none_v is None and np.array_equal(_bits(plain), _bits(out))
    for scale in U.SCALES:
        w, h = 37, 21
        lw, lh = U.lattice_shape(w, h, scale)
        g = {"normal_depth": np.tile(np.float32([0, 1, 0, 2.5]), (1, h, w, 1)),
             "albedo": np.tile(np.float32([0.5, 0.5, 0.5, 1]), (1, h, w, 1)),
             "id": np.full((1, h, w), 5 | 1 << 30, np.uint32)}
        X, Y = np.meshgrid(np.arange(lw, dtype=np.float32), np.arange(lh, dtype=np.float32))
        low = np.stack([8 * X + 16 * Y + 3, 24 * X, 8 * Y + 1, np.ones_like(X)], axis=-1)[None].astype(np.float32)
        out, wt, _, cnt = U.upsample_ref(up_lib, low, g, scale, 0.25)
        x, y = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
        # inside the lattice's hull all four taps count and the interpolation is exact (multiples of 1/8 below 2^10);
        # beyond its last column / row the taps outside are left out and the pixel takes the nearest lattice values
        xc, yc = np.minimum(x / scale, lw - 1), np.minimum(y / scale, lh - 1)
        want = np.stack([8 * xc + 16 * yc + 3, 24 * xc, 8 * yc + 1], axis=-1)
        assert cnt["hole_w"] == 0 and cnt["rej_id"] + cnt["rej_mh"] + cnt["rej_normal"] == 0
        assert np.array_equal(out[0][..., :3].astype(np.float64), want), scale


def _gpu_case_counts(up_lib, aov_lib):
    total, scenes = {}, {}
    for shape in U.SHAPES:
        for scale in U.SCALES:
            for n in U.N_FRAMES:
                low, g, vm = U.synthetic(shape, scale, n)
                for w_min in U.W_MINS:
                    _add(total, U.upsample_ref(up_lib, low, g, scale, w_min, vm)[3])
    for name in U.VIEW:
        _, _, g = _scene_guides(aov_lib, name)
        w, h = U.VIEW[name]
        for scale in U.SCENE_SCALES:
            lw, lh = U.lattice_shape(w, h, scale)
            low = np.random.default_rng(scale).uniform(0, 1, size=(1, lh, lw, 4)).astype(np.float32)
            cnt = U.upsample_ref(up_lib, low, {k: g[k][None] for k in U.NAMES}, scale, 0.25)[3]
            _add(total, cnt)
            scenes[(name, scale)] = (cnt, w * h)
    return total, scenes


def test_gpu_case_inputs_keep_every_outcome_busy(up_lib, aov_lib):
    """Input conditions of tests/test_gpu_upsample.py, on the reference alone:
    over its cases every outcome of a pixel and of a tap is counted; in every
    scene case the holes stay under half of the pixels off the lattice and
    the interpolated ones are at least half of them."""
    total, scenes = _gpu_case_counts(up_lib, aov_lib)
    print("all GPU cases:", total)
    assert all(total[k] > 0 for k in U.COUNTS), total
    for (name, scale), (cnt, n_pix) in scenes.items():
        off = n_pix - cnt["lattice"]
        interp = cnt["from_1"] + cnt["from_2"] + cnt["from_3"] + cnt["from_4"]
        print(name, scale, "holes / off-lattice", (cnt["hole_w"] + cnt["hole_failed"]) / off, "interpolated", interp / off)
        assert cnt["hole_w"] + cnt["hole_failed"] < 0.5 * off, (name, scale, cnt)
        assert interp >= 0.5 * off, (name, scale, cnt)


def test_fill_reference(up_lib):
    """upref_fill replaces exactly the listed pixels inside the window."""
    rng = np.random.default_rng(5)
    img = rng.uniform(0, 1, size=(6, 9, 4)).astype(np.float32)
    var, wt = rng.uniform(0, 1, size=(2, 6, 9)).astype(np.float32)
    px = np.uint32([[10, 20], [18, 25], [9, 20], [19, 20], [10, 26], [14, 23]])
    ex = rng.uniform(2, 3, size=(6, 4)).astype(np.float32)
    ev = rng.uniform(2, 3, size=6).astype(np.float32)
    o, v, w_, n = U.fill_ref(up_lib, img, var, wt, 10, 20, px, ex, ev, 1.0)
    assert n == 3
    for e in (0, 1, 5):
        i, j = px[e][0] - 10, px[e][1] - 20
        assert np.array_equal(o[j, i], ex[e]) and v[j, i] == ev[e] and w_[j, i] == 1.0
    assert int((o != img).any(axis=-1).sum()) == 3 and int((v != var).sum()) == 3 and int((w_ != wt).sum()) == 3
    o2, v2, w2, _ = U.fill_ref(up_lib, img, None, None, 10, 20, px, ex, None, 1.0)
    assert v2 is None and w2 is None and np.array_equal(o2, o)


def test_select_holes_lists_the_zero_weights():
    """select_holes and select_holes_frames on CPU tensors: the pixels with weight 0, row-major, offset by the
    window's origin; the frames' lists back to back with their offsets; an empty frame in between."""
    import torch

    from mirror_maze import select_holes, select_holes_frames

    rng = np.random.default_rng(3)
    wt = rng.choice(np.float32([0.0, 1.0, 2.5]), size=(3, 9, 13), p=[0.2, 0.5, 0.3])
    wt[1] = 1.0
    x0, y0 = 6, 40
    lists = []
    for f in range(3):
        want = U.holes_of(wt[f]).astype(np.int64) + np.int64([x0, y0])
        got = select_holes(torch.from_numpy(wt[f]), x0, y0)
        assert got.dtype == torch.int32 and np.array_equal(got.numpy(), want)
        lists.append(want)
    assert len(lists[0]) > 0 and len(lists[1]) == 0
    assert np.array_equal(select_holes(torch.from_numpy(wt[0])).numpy(), U.holes_of(wt[0]))
    px, offs = select_holes_frames(torch.from_numpy(wt), x0, y0)
    assert offs.dtype == np.uint64 and list(offs) == [0, len(lists[0]), len(lists[0]), len(lists[0]) + len(lists[2])]
    assert np.array_equal(px.numpy(), np.concatenate(lists))
    with pytest.raises(ValueError):
        select_holes(torch.from_numpy(wt))
    with pytest.raises(ValueError):
        select_holes_frames(torch.from_numpy(wt[0]))


@pytest.mark.parametrize("name", ["maze4", "corridor"])
def test_reference_upsample_is_no_worse_than_the_raw_frame(up_lib, aov_lib, name):
    """s = 2, 8 spp, w_min 0.25: the low view traced by the oracle, upsampled
    by the reference with aov_ref.c's guides, holes filled from an 8-spp oracle
    frame of the full view.  MSE against a 512-spp frame / the raw full 8-spp
    frame's MSE must be below 1.0: a quarter to a third of the rays must not
    give a worse frame than tracing every pixel.  (A float64 prototype measured
    0.66 on the maze and 0.76 on the corridor.)  Measured with this reference:
    maze4 160x120 0.541 with no holes (0.25 of the full frame's
    rays), corridor 140x48 0.830 with 4.5 % holes (0.295 of the rays)."""
    from mirror_maze import make_ext
    from oracle.oracle import Oracle

    scale = 2
    s, u, g = _scene_guides(aov_lib, name)
    w, h = U.VIEW[name]
    o = Oracle.from_scene(s)
    low, _ = oracle_tile(o, U.low_uniform(u, scale), make_ext(U.SPP, 8, U.MIRROR_LIMIT, frame=0), 0, 0, w // scale, h // scale)
    raw, _ = oracle_tile(o, u, make_ext(U.SPP, 8, U.MIRROR_LIMIT, frame=0), 0, 0, w, h)
    truth, _ = oracle_tile(o, u, make_ext(512, 8, U.MIRROR_LIMIT, frame=1), 0, 0, w, h)
    out, wt, _, cnt = U.upsample_ref(up_lib, low, {k: g[k][None] for k in U.NAMES}, scale, 0.25)
    hole = wt[0] == 0
    filled = np.where(hole[..., None], raw, out[0])
    ratio = U.mse_ratio(filled, raw, truth)
    traced = (low.shape[0] * low.shape[1] + int(hole.sum())) / (w * h)
    print(name, "MSE ratio", ratio, "holes", float(hole.mean()), "rays traced (share of full)", traced, cnt)
    assert np.isfinite(filled).all()
    assert ratio < 1.0, ratio


def test_flythrough_upsample_argument(capsys):
    """--upsample parses, alone and with the filters it composes with; with
    --no-render nothing is rendered or written, and the camera path is printed
    as before."""
    import importlib.util
    import sys

    path0 = list(sys.path)
    try:
        spec = importlib.util.spec_from_file_location("flythrough_up", REPO / "scripts" / "flythrough.py")
        fly = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(fly)
        for extra in (["--upsample", "2"], ["--upsample", "4:0.5"], ["--upsample", "2", "--denoise"],
                      ["--upsample", "2", "--accumulate-var", "--denoise-var"], ["--upsample", "8:1", "--accumulate-var"]):
            rc = fly.main(["--maze", "4", "--frames", "3", "--width", "64", "--height", "48", "--no-render", *extra])
            assert rc == 0, extra
            assert len([ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("frame ")]) == 3
        for bad in ("3", "2:0", "2:1.5", "x"):
            with pytest.raises(SystemExit):
                fly.main(["--maze", "4", "--frames", "1", "--no-render", "--upsample", bad])
            capsys.readouterr()
    finally:
        sys.path[:] = path0
