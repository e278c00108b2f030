"""mm_denoise_frames, host side (no GPU): the C-ABI symbol and its argument
checks, the parameter struct's layout, the reference filter
(tests/denoise_ref.c) judged against converged frames, and the input
conditions the GPU cases (tests/test_gpu_denoise.py) rely on."""
from __future__ import annotations

import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import aov_support as A
import denoise_support as D
from conftest import oracle_tile

REPO = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def dn_lib(tmp_path_factory):
    return D.build_ref(tmp_path_factory.mktemp("denoise_ref"))


@pytest.fixture(scope="module")
def aov_lib(tmp_path_factory):
    return A.build_ref(tmp_path_factory.mktemp("aov_ref"))


def test_symbol_exists_and_rejects_bad_arguments_without_a_gpu():
    """The argument checks need no context, so they run here: every call below
    returns MM_ERR_INVALID before anything touches a device."""
    from mirror_maze import _lib

    L = _lib.lib()
    assert "mm_denoise_frames" in _lib.EXPORTS
    inv = _lib.MM_ERR_INVALID
    buf = (C.c_float * 64)()  # 16-byte aligned stand-ins; never dereferenced
    base = (C.addressof(buf) + 15) & ~15
    col, nd, al, ids, out = (C.c_void_p(base + 16 * i) for i in range(5))
    a = _lib.mm_aov(nd, al, ids)
    ok = _lib.mm_denoise_params(4, 0.02, 0.5, 0)
    call = L.mm_denoise_frames
    # a null context, with everything else in order
    assert call(None, col, C.byref(a), C.byref(ok), 1, 1, 1, out) == inv
    fake = None  # (no context exists without a GPU; tests/test_gpu_denoise.py repeats these with a real one)
    # null pointers: the parameters, the guides, each guide buffer, the colour, the output
    assert call(fake, col, C.byref(a), None, 1, 1, 1, out) == inv
    assert call(fake, col, None, C.byref(ok), 1, 1, 1, out) == inv
    for hole in range(3):
        g = [nd, al, ids]
        g[hole] = None
        assert call(fake, col, C.byref(_lib.mm_aov(*g)), C.byref(ok), 1, 1, 1, out) == inv
    assert call(fake, None, C.byref(a), C.byref(ok), 1, 1, 1, out) == inv
    assert call(fake, col, C.byref(a), C.byref(ok), 1, 1, 1, None) == inv
    # n_passes 0 and 9, unknown flag bits, empty shapes
    for bad in (_lib.mm_denoise_params(0, 0.02, 0.5, 0), _lib.mm_denoise_params(9, 0.02, 0.5, 0),
                _lib.mm_denoise_params(4, 0.02, 0.5, 2), _lib.mm_denoise_params(4, 0.02, 0.5, 0x80000001)):
        assert call(fake, col, C.byref(a), C.byref(bad), 1, 1, 1, out) == inv
    for n, w, h in ((0, 1, 1), (1, 0, 1), (1, 1, 0)):
        assert call(fake, col, C.byref(a), C.byref(ok), n, w, h, out) == inv
    assert _lib.MM_DENOISE_MAX_PASSES == 8 and _lib.MM_DN_RGBA8 == 1


def test_params_layout_matches_the_header():
    from mirror_maze import _lib

    txt = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "mm_types.h").read_text(), flags=re.S)
    body = re.search(r"typedef struct mm_denoise_params \{(.*?)\} mm_denoise_params;", txt, flags=re.S).group(1)
    fields = re.findall(r"(\w+)\s+(\w+)\s*;", body)
    assert fields == [("uint32_t", "n_passes"), ("float", "sigma_z"), ("float", "sigma_l"), ("uint32_t", "flags")]
    assert [n for n, _ in _lib.mm_denoise_params._fields_] == [f[1] for f in fields]
    assert C.sizeof(_lib.mm_denoise_params) == 16
    check = (REPO / "mirror-maze_amd" / "csrc" / "mm_layout_check.cpp").read_text()
    assert "sizeof(mm_denoise_params) == 16" in check


def _frames(aov_lib, scene, u, w, h, mirror_limit=8):
    """(8-spp frame, 512-spp frame, guides) of the whole w x h view from the
    oracle and aov_ref.c."""
    from mirror_maze import make_ext
    from oracle.oracle import Oracle

    o = Oracle.from_scene(scene)
    noisy, _ = oracle_tile(o, u, make_ext(8, 8, mirror_limit, frame=0), 0, 0, w, h)
    truth, _ = oracle_tile(o, u, make_ext(512, 8, mirror_limit, frame=1), 0, 0, w, h)
    guides = A.Ref(aov_lib, scene).tile(u, mirror_limit, 0, 0, w, h)
    return noisy, truth, guides


@pytest.mark.parametrize("name,view", [("maze4", (160, 120)), ("corridor", (140, 32))])
def test_reference_filter_beats_the_raw_frame(dn_lib, aov_lib, name, view):
    """With the defaults, MSE(filtered 8 spp) / MSE(raw 8 spp) against a 512-spp
    frame is below 0.5 (a float64 prototype measured 0.016 on the maze and
    0.154 on the corridor); the filter keeps alpha."""
    w, h = view
    s, u = D.maze_view(w, h) if name == "maze4" else D.corridor_view(w, h)
    noisy, truth, guides = _frames(aov_lib, s, u, w, h)
    out, cnt = D.filter_ref(dn_lib, noisy, guides, **D.DEFAULTS)
    ratio = D.mse_ratio(out[0], noisy, truth)
    print(name, view, "MSE ratio", ratio, cnt)
    assert np.isfinite(out).all()
    assert ratio < 0.5, ratio
    assert np.array_equal(out[0][..., 3], noisy[..., 3])
    if name == "corridor":  # mirror chains: the guides name surfaces seen through 0..7 mirrors
        assert guides["albedo"][..., 3].max() == 7.0 and len(np.unique(guides["albedo"][..., 3])) >= 4


def test_gpu_case_inputs_keep_every_clause_busy(dn_lib):
    """Input conditions of tests/test_gpu_denoise.py's synthetic cases, on the
    reference alone: every rejection clause, the out-of-tile skip and both soft
    terms are counted non-zero -- thousands of taps each on the larger shapes."""
    for (w, h) in D.SHAPES:
        color, guides = D.synthetic(3, h, w, seed=w * 1000 + h)
        _, cnt = D.filter_ref(dn_lib, color, guides, n_passes=5, sigma_z=0.02, sigma_l=0.5)
        print((w, h), cnt)
        assert cnt["taken"] >= 3 * w * h * 5 and cnt["out_of_tile"] > 0
        if (w, h) == (1, 1):
            assert cnt["taken"] == 3 * 5 and cnt["out_of_tile"] == 3 * 5 * 24
        if w * h >= 120:
            assert all(cnt[k] > 0 for k in D.COUNTS), cnt
        if (w, h) in ((67, 5), (130, 9)):
            assert all(cnt[k] >= 1000 for k in D.COUNTS), cnt
    # z spans 0.2 .. 1e30, ids hold MISS, mirror hits 0..2
    color, guides = D.synthetic(3, 9, 130, seed=130009)
    assert guides["normal_depth"][..., 3].min() < 0.21 and guides["normal_depth"][..., 3].max() > 9e29
    assert (guides["id"] == D.MISS).any() and sorted(np.unique(guides["albedo"][..., 3])) == [0.0, 1.0, 2.0]
    # at (3, 40) and (1, 1) every far tap is out of tile: only the centre column / the centre is left at s >= 4
    _, far = D.filter_ref(dn_lib, *D.synthetic(1, 40, 3, seed=5), n_passes=8, sigma_z=0.0, sigma_l=0.0)
    assert far["soft_z"] == 0 and far["soft_l"] == 0 and far["out_of_tile"] > far["taken"]


def test_terms_off_and_single_surface_is_the_plain_b3_blur(dn_lib):
    """With both soft terms off and one surface everywhere the filter is the
    separable B3-spline blur renormalised at the borders: a constant image
    stays constant to rounding, and the counts show no rejection."""
    h, w = 9, 20
    color = np.full((1, h, w, 4), 0.375, np.float32)
    color[..., 3] = 1.0
    guides = {"normal_depth": np.tile(np.float32([0, 0, 1, 2.0]), (1, h, w, 1)),
              "albedo": np.zeros((1, h, w, 4), np.float32), "id": np.full((1, h, w), 5 | 1 << 30, np.uint32)}
    out, cnt = D.filter_ref(dn_lib, color, guides, n_passes=3, sigma_z=0.0, sigma_l=0.0)
    assert np.abs(out[..., :3] - 0.375).max() <= 2 ** -22
    assert cnt["rej_id"] == cnt["rej_mh"] == cnt["rej_normal"] == cnt["soft_z"] == cnt["soft_l"] == 0
    assert cnt["taken"] + cnt["out_of_tile"] == 3 * 25 * h * w


def test_flythrough_denoise_argument(capsys):
    """--denoise parses (with and without --aov); with --no-render nothing is
    rendered or written, and the camera path is printed as before."""
    import importlib.util
    import sys

    path0 = list(sys.path)
    try:
        spec = importlib.util.spec_from_file_location("flythrough_dn", REPO / "scripts" / "flythrough.py")
        fly = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(fly)
        for extra in ([], ["--aov", "unused_aov_dir"]):
            rc = fly.main(["--maze", "4", "--frames", "3", "--width", "64", "--height", "48", "--denoise",
                           "--no-render", *extra])
            assert rc == 0
            assert len([ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("frame ")]) == 3
        assert not (Path.cwd() / "unused_aov_dir").exists()
        assert "--denoise" in (REPO / "scripts" / "flythrough.py").read_text()
    finally:
        sys.path[:] = path0
