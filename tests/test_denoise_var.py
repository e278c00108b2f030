"""mm_denoise_frames_var, host side (no GPU): the C-ABI symbol and its argument
checks, the parameter struct's layout, the reference filter
(tests/denoise_var_ref.c) against denoise_ref.c and against the squared-weight
rule worked out by hand, and the input conditions the GPU cases
(tests/test_gpu_denoise_var.py) rely on."""
from __future__ import annotations

import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import denoise_support as D
import denoise_var_support as V

REPO = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def dnv_lib(tmp_path_factory):
    return V.build_ref(tmp_path_factory.mktemp("denoise_var_ref"))


@pytest.fixture(scope="module")
def dn_lib(tmp_path_factory):
    return D.build_ref(tmp_path_factory.mktemp("denoise_ref"))


def test_symbol_exists_and_rejects_bad_arguments_without_a_gpu():
    """The argument checks need no context, so they run here: every call below
    returns MM_ERR_INVALID before anything touches a device -- also the one
    with everything in order, whose only fault is the null context."""
    from mirror_maze import _lib

    L = _lib.lib()
    assert "mm_denoise_frames_var" in _lib.EXPORTS
    inv = _lib.MM_ERR_INVALID
    buf = (C.c_float * 96)()  # 16-byte aligned stand-ins, 16 bytes apart (w = h = 1); never dereferenced
    base = (C.addressof(buf) + 15) & ~15
    col, nd, al, ids, var, out, vout = (base + 16 * i for i in range(7))
    a = _lib.mm_aov(nd, al, ids)

    def params(n_passes=5, sigma_z=0.02, sigma_l=4.0, eps_l=1e-3, flags=0, reserved=0):
        return _lib.mm_denoise_var_params(n_passes, sigma_z, sigma_l, eps_l, flags, reserved)

    def call(color=col, aov=a, v=var, p=params(), n=1, w=1, h=1, o=out, vo=vout):
        return L.mm_denoise_frames_var(None, color, C.byref(aov) if aov is not None else None, v,
                                       C.byref(p) if p is not None else None, n, w, h, o, vo)

    assert call() == inv  # a null context, with everything else in order
    # null pointers: the parameters, the guides, each guide buffer, the colour, the variance, the output
    assert call(p=None) == inv and call(aov=None) == inv and call(color=None) == inv
    assert call(v=None) == inv and call(o=None) == inv
    for hole in range(3):
        g = [nd, al, ids]
        g[hole] = None
        assert call(aov=_lib.mm_aov(*g)) == inv
    # n_passes 0 and 9, unknown flag bits, reserved, empty shapes
    for bad in (params(n_passes=0), params(n_passes=9), params(flags=2), params(flags=0x80000001),
                params(reserved=1)):
        assert call(p=bad) == inv
    for n, w, h in ((0, 1, 1), (1, 0, 1), (1, 1, 0)):
        assert call(n=n, w=w, h=h) == inv
    # eps_l: finite and > 0 when the luminance term is on; ignored when it is off
    for eps in (0.0, -1e-3, float("inf"), float("nan")):
        assert call(p=params(eps_l=eps)) == inv
    # misaligned variance buffers, outputs overlapping an input or each other
    assert call(v=var + 2) == inv and call(vo=vout + 2) == inv
    assert call(o=col) == inv and call(o=var) == inv and call(vo=var) == inv and call(vo=col + 4) == inv
    assert call(vo=out + 8) == inv and call(vo=ids) == inv
    assert _lib.MM_DNV_RGBA8 == 1
    # (a null context has no error text of its own, and returns MM_ERR_INVALID whatever the checks do: that each
    # rejection above is this call's own, with its message, and that the null context is refused after them, is
    # tests/test_filter_args.py's; the messages with a context: tests/test_gpu_denoise_var.py)


def test_params_layout_matches_the_header():
    from mirror_maze import _lib

    txt = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "mm_types.h").read_text(), flags=re.S)
    body = re.search(r"typedef struct mm_denoise_var_params \{(.*?)\} mm_denoise_var_params;", txt, flags=re.S).group(1)
    fields = re.findall(r"(\w+)\s+(\w+)\s*;", body)
    assert fields == [("uint32_t", "n_passes"), ("float", "sigma_z"), ("float", "sigma_l"), ("float", "eps_l"),
                      ("uint32_t", "flags"), ("uint32_t", "reserved")]
    assert [n for n, _ in _lib.mm_denoise_var_params._fields_] == [f[1] for f in fields]
    assert C.sizeof(_lib.mm_denoise_var_params) == 24
    check = (REPO / "mirror-maze_amd" / "csrc" / "mm_layout_check.cpp").read_text()
    assert "sizeof(mm_denoise_var_params) == 24" in check


def test_gpu_case_inputs_keep_every_clause_busy(dnv_lib):
    """Input conditions of tests/test_gpu_denoise_var.py's synthetic cases, on
    the reference alone, for both of its parameter sets: every counter is
    non-zero at every shape that has more than a handful of pixels -- the
    denoiser's seven, the stop's 3x3 taps taken and rejected by each clause,
    stops that are eps_l exactly, and variance products that are subnormal or
    zero."""
    for (w, h) in V.SHAPES:
        color, guides = V.synthetic(3, h, w, seed=w * 1000 + h)
        var = V.synthetic_var(3, h, w, seed=w * 1000 + h)
        for params in (V.MAIN, V.TINY):
            _, vout, cnt = V.filter_ref(dnv_lib, color, guides, var, 5, *params)
            print((w, h), params, cnt)
            assert np.isfinite(vout).all() and (vout >= 0).all()
            assert cnt["taken"] >= 3 * w * h * 5 and cnt["out_of_tile"] > 0 and cnt["pre_out_of_tile"] > 0
            assert cnt["pre_taken"] >= 3 * w * h * 5
            if (w, h) == (1, 1):
                assert cnt["pre_taken"] == 3 * 5 and cnt["pre_out_of_tile"] == 3 * 5 * 8
            if w * h >= 120:
                assert all(cnt[k] > 0 for k in V.COUNTS), cnt
            if (w, h) in ((67, 5), (130, 9)):
                assert all(cnt[k] >= 100 for k in V.COUNTS), cnt
    var = V.synthetic_var(3, 9, 130, seed=130009)
    sub = (var > 0) & (var < np.float32(2.0 ** -126))
    assert (var == 0).any() and sub.any() and var.max() > 10.0 and var[(var > 0) & ~sub].min() < 1e-10
    # the tiny stop takes weights below the normal range: with it the last pass's variance differs from MAIN's
    color, guides = V.synthetic(1, 9, 130, seed=130009)
    a = V.filter_ref(dnv_lib, color, guides, var[:1], 1, *V.TINY)[1]
    b = V.filter_ref(dnv_lib, color, guides, var[:1], 1, *V.MAIN)[1]
    assert not np.array_equal(a, b)


@pytest.mark.parametrize("sigma_z", [0.02, 0.0])
def test_luminance_term_off_is_the_denoiser_on_all_bits(dnv_lib, dn_lib, sigma_z):
    """With sigma_l <= 0 the colour is denoise_ref.c's with sigma_l = 0, whatever the variance holds."""
    for (w, h), n_passes in (((67, 5), 5), ((130, 9), 3), ((3, 40), 8), ((1, 1), 2)):
        color, guides = V.synthetic(2, h, w, seed=w * 1000 + h)
        var = V.synthetic_var(2, h, w, seed=7)
        for off in (0.0, -2.0):
            got, _, _ = V.filter_ref(dnv_lib, color, guides, var, n_passes, sigma_z, off, 0.0)
            want, _ = D.filter_ref(dn_lib, color, guides, n_passes, sigma_z, 0.0)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), ((w, h), n_passes, off)


def test_constant_variance_follows_the_squared_weight_rule(dnv_lib):
    """One surface, both terms off, V = v0 everywhere: an interior pixel of pass
    0 takes all 25 taps with weights hk x hk that sum to 1, so Vout = v0 * sum of
    their squares = v0 * (35/128)^2 (sum hk^2 = 70/256), within 4 ulp.  The
    squared weights are k * 2^-16 with integers k <= 1296 that sum to 4900, and
    W is 1 exactly; v0 is taken with a mantissa of one or two bits, so that
    every product and every partial sum of the 25-term running sum is exact and
    the bound has room to spare.  (For a general v0 each product and each step
    of the sum rounds once, 12.5 ulp in the worst case: the specified order
    gives 5 ulp at v0 = 0.3f, which is the sum's rounding, not the rule's.)"""
    h, w = 9, 20
    color = np.full((1, h, w, 4), 0.375, np.float32)
    color[..., 3] = 1.0
    guides = {"normal_depth": np.tile(np.float32([0, 0, 1, 2.0]), (1, h, w, 1)),
              "albedo": np.zeros((1, h, w, 4), np.float32), "id": np.full((1, h, w), 5 | 1 << 30, np.uint32)}
    for v0 in (np.float32(0.25), np.float32(2.0 ** -20), np.float32(96.0)):
        var = np.full((1, h, w), v0, np.float32)
        _, vout, cnt = V.filter_ref(dnv_lib, color, guides, var, 1, 0.0, 0.0, 0.0)
        want = np.float32(float(v0) * (35.0 / 128.0) ** 2)
        inner = vout[0, 2:-2, 2:-2]
        assert np.abs(inner.astype(np.float64) - float(want)).max() <= 4 * float(np.spacing(want)), (v0, inner, want)
        assert cnt["rej_id"] == cnt["rej_mh"] == cnt["rej_normal"] == 0 and cnt["pre_taken"] == 0
        # at the border fewer taps share the weight: the variance is higher there
        assert vout[0, 0, 0] > inner.max()
    # with the luminance term on and an even image the stop changes nothing: t = 0 for every tap
    _, von, cnt = V.filter_ref(dnv_lib, color, guides, var, 1, 0.0, 4.0, 1e-3)
    assert np.array_equal(von, vout) and cnt["pre_taken"] > 0 and cnt["soft_l"] == 0


def test_flythrough_denoise_var_argument(capsys):
    """--denoise-var parses, alone and with --refine; with --no-render nothing is
    rendered; with --accumulate it is rejected with a message."""
    import importlib.util
    import sys

    path0 = list(sys.path)
    try:
        spec = importlib.util.spec_from_file_location("flythrough_dnv", REPO / "scripts" / "flythrough.py")
        fly = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(fly)
        for extra in ([], ["--refine", "0.1"]):
            rc = fly.main(["--maze", "4", "--frames", "3", "--width", "64", "--height", "48", "--denoise-var",
                           "--no-render", *extra])
            assert rc == 0
            assert len([ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("frame ")]) == 3
        with pytest.raises(SystemExit):
            fly.main(["--maze", "4", "--frames", "3", "--denoise-var", "--accumulate", "--no-render"])
        assert "--denoise-var does not go with --accumulate" in capsys.readouterr().err
    finally:
        sys.path[:] = path0
