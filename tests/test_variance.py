"""CPU tests of the per-pixel sample variance: the C reference
(tests/variance_ref.c) against the oracle's mean and a float64 numpy variance,
its stand-alone driver plain and sanitized, select_noisy / merge_samples on CPU
tensors, the new symbols' argument checks, and the tolerance the GPU refine test
pins (derived here from the reference alone)."""
from __future__ import annotations

import subprocess

import numpy as np
import pytest

import variance_support as V


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def var_lib(tmp_path_factory):
    return V.build_ref(tmp_path_factory.mktemp("variance_ref"))


@pytest.fixture(scope="module")
def ref(var_lib):
    from mirror_maze import Scene

    return V.Ref(var_lib, Scene.build(4, 0))


def _sum_T(x):
    """The resolve's order over the last axis of a float32 array."""
    spp = x.shape[-1]
    if spp % 8 == 0:
        acc = None
        for b in range(0, spp, 8):
            blk = ((x[..., b] + x[..., b + 1]) + (x[..., b + 2] + x[..., b + 3])) + \
                  ((x[..., b + 4] + x[..., b + 5]) + (x[..., b + 6] + x[..., b + 7]))
            acc = blk if acc is None else acc + blk
        return acc
    acc = x[..., 0]
    for k in range(1, spp):
        acc = acc + x[..., k]
    return acc


@pytest.mark.parametrize("spp", V.SPPS_LINEAR + V.SPPS_BLOCK)
def test_tile_mean_is_the_oracles(ref, spp):
    """The restated sample loop draws the oracle's samples: the mean equals
    oracle_trace_tile on all bits, with y_stride 1 and 2; a list entry is its
    pixel of the tile, and entries outside the view are zero."""
    from mirror_maze import make_ext

    u = V.view_uniform()
    e = make_ext(spp, 8, 8, frame=3)
    x0, y0, w, h = V.TILE
    for ys in (1, 2):
        out, var = ref.tile(u, e, x0, y0, w, h, ys)
        assert np.array_equal(_bits(out), _bits(ref.oracle_tile(u, e, x0, y0, w, h, ys)))
        assert np.isfinite(var).all() and (var >= 0).all() and (var > 0).mean() > 0.1  # not a black tile
    out, var = ref.tile(u, e, x0, y0, w, h)
    px, inside = V.list_pixels()
    lo, lv = ref.pixels(u, e, px)
    assert len(px) == 200 and (~inside).sum() == 5
    j, i = px[inside, 1].astype(np.int64) - y0, px[inside, 0].astype(np.int64) - x0
    assert np.array_equal(_bits(lo[inside]), _bits(out[j, i])) and np.array_equal(_bits(lv[inside]), _bits(var[j, i]))
    assert not lo[~inside].any() and not lv[~inside].any()


@pytest.mark.parametrize("spp", V.SPPS_LINEAR + V.SPPS_BLOCK)
def test_variance_of_synthetic_samples(var_lib, spp):
    """Samples in [0, 4]: var agrees with a float64 two-pass variance to 1e-5
    relative (about 100 ulp of headroom over a float32 two-pass sum of <= 64
    terms) and equals the header's statement in float32 numpy on all bits;
    equal samples give exactly 0; the mean is the statement's too.

    The float64 comparison is made on the pixels whose luminances spread by a
    standard deviation of at least 0.25: a binary32 l_k below 4 carries up to
    2 x 2^-23 of rounding (its two additions; the products by 0.25 and 0.5 are
    exact), so does ml, and a deviation d = l_k - ml of size sigma is then off
    by up to about 5e-7 / sigma relative, its square by twice that -- 4e-6 at
    sigma = 0.25, inside the bound; samples closer together than that are
    ill-conditioned for any binary32 luminance, whatever the summation."""
    rng = np.random.default_rng(spp)
    s = rng.uniform(0.0, 4.0, size=(257, spp, 3)).astype(np.float32)
    s[0] = 4.0
    s[1] = 0.0
    s[2] = s[2, 0]  # equal samples
    mean, var = V.samples_ref(var_lib, s)
    lum64 = 0.25 * s[..., 0].astype(np.float64) + 0.5 * s[..., 1] + 0.25 * s[..., 2]
    want = ((lum64 - lum64.mean(axis=1, keepdims=True)) ** 2).sum(axis=1) / (spp - 1)
    assert (want > 0).sum() == 254
    live = np.sqrt(want) >= 0.25
    assert live.sum() >= 150
    assert (np.abs(var[live] - want[live]) / want[live]).max() < 1e-5
    assert np.array_equal(_bits(var[:3]), np.zeros(3, np.uint32))
    # the statement, operation by operation in float32
    lum = (np.float32(0.25) * s[..., 0] + np.float32(0.5) * s[..., 1]) + np.float32(0.25) * s[..., 2]
    ml = _sum_T(lum) / np.float32(spp)
    q = (lum - ml[:, None]) * (lum - ml[:, None])
    v32 = _sum_T(q) / np.float32(spp - 1)
    assert lum.dtype == np.float32 and v32.dtype == np.float32
    assert np.array_equal(_bits(var), _bits(v32))
    m32 = np.stack([_sum_T(s[..., c]) / np.float32(spp) for c in range(3)], axis=1)
    assert np.array_equal(_bits(mean), _bits(m32))


def test_two_samples_closed_form(var_lib):
    """spp = 2: var is exactly the statement's closed form in float32 numpy,
    ((l0 - ml)^2 + (l1 - ml)^2) / 1 with ml = (l0 + l1) / 2."""
    rng = np.random.default_rng(2)
    s = rng.uniform(0.0, 4.0, size=(1000, 2, 3)).astype(np.float32)
    _, var = V.samples_ref(var_lib, s)
    lum = (np.float32(0.25) * s[..., 0] + np.float32(0.5) * s[..., 1]) + np.float32(0.25) * s[..., 2]
    ml = (lum[:, 0] + lum[:, 1]) / np.float32(2)
    want = ((lum[:, 0] - ml) * (lum[:, 0] - ml) + (lum[:, 1] - ml) * (lum[:, 1] - ml)) / np.float32(1)
    assert want.dtype == np.float32 and np.array_equal(_bits(var), _bits(want))


def test_reference_driver_runs_clean(tmp_path):
    """The reference's stand-alone driver, plain and under the address and
    undefined-behaviour sanitizers (a host program of its own); both builds
    print the same checksum."""
    outs = []
    for name, flags in (("plain", ()), ("sanitized", ("-O1", "-g", "-fsanitize=address,undefined",
                                                      "-fno-sanitize-recover=all"))):
        (tmp_path / name).mkdir()
        exe = V.build_driver(tmp_path / name, flags)
        r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
        assert r.stdout.startswith("lit ") and "checksum" in r.stdout
        outs.append(r.stdout)
    assert outs[0] == outs[1]


def test_merge_samples_pools_two_halves():
    """The pooled (mean, var, n) of two halves of a sample set is the whole
    set's, to 1e-5 relative (1e-6 absolute), for equal and unequal halves and
    for scalar and per-pixel counts."""
    import torch

    from mirror_maze import merge_samples

    rng = np.random.default_rng(7)
    s = rng.uniform(0.0, 4.0, size=(300, 32, 3))

    def moments(x):
        lum = 0.25 * x[..., 0] + 0.5 * x[..., 1] + 0.25 * x[..., 2]
        return x.mean(axis=1), lum.var(axis=1, ddof=1)

    def t(x):
        return torch.from_numpy(np.asarray(x, dtype=np.float32))

    whole_m, whole_v = moments(s)
    for na in (8, 16, 2, 30):
        (ma, va), (mb, vb) = moments(s[:, :na]), moments(s[:, na:])
        for n_a, n_b in ((na, 32 - na), (t(np.full(300, na)), t(np.full(300, 32 - na)))):
            m, v, n = merge_samples(t(ma), t(va), n_a, t(mb), t(vb), n_b)
            assert m.dtype == torch.float32 and v.dtype == torch.float32 and tuple(m.shape) == (300, 3)
            assert np.allclose(m.numpy(), whole_m, rtol=1e-5, atol=1e-6)
            assert np.allclose(v.numpy(), whole_v, rtol=1e-5, atol=1e-6)
            assert np.all(n.numpy() == 32)


def test_select_noisy_on_cpu_tensors():
    """Exactly the pixels a float64 numpy statement of the inequality picks (on
    inputs whose margin to the threshold is above 1e-4 relative), row-major,
    without duplicates; per-pixel counts, the id mask, the window offset, and
    an infinite tolerance."""
    import torch

    from mirror_maze import MM_AOV_ID_FAILED, MM_AOV_ID_MISS, select_noisy

    rng = np.random.default_rng(11)
    h, w = 24, 31
    color = rng.uniform(0.0, 2.0, size=(h, w, 4)).astype(np.float32)
    color[3, 4, :3] = 0.0  # a black pixel: the floor decides
    var = (rng.uniform(0.0, 1.5, size=(h, w)) ** 2).astype(np.float32)
    count = rng.integers(2, 64, size=(h, w)).astype(np.float32)
    tol = 0.2
    for cnt in (8.0, count):
        want, margin = V.noisy_numpy(color, var, cnt, tol)
        # move the pixels near the threshold clear of it
        near = margin <= 1e-3
        v = var.copy()
        v[near] *= 4.0
        want, margin = V.noisy_numpy(color, v, cnt, tol)
        assert margin.min() > 1e-4 and 0.1 < want.mean() < 0.9
        got = select_noisy(torch.from_numpy(color), torch.from_numpy(v),
                           cnt if np.isscalar(cnt) else torch.from_numpy(cnt), tol)
        assert got.dtype == torch.int32 and got.is_contiguous() and got.device.type == "cpu"
        jj, ii = np.nonzero(want)  # row-major
        assert got.tolist() == np.stack([ii, jj], axis=1).tolist()
        assert len({tuple(p) for p in got.tolist()}) == got.shape[0]
    ids = torch.full((1, h, w), 7 | 0x40000000, dtype=torch.int32)
    jj, ii = np.nonzero(want)
    ids[0, jj[0], ii[0]] = MM_AOV_ID_MISS - (1 << 32)
    ids[0, jj[1], ii[1]] = MM_AOV_ID_FAILED - (1 << 32)
    got = select_noisy(torch.from_numpy(color), torch.from_numpy(v), torch.from_numpy(count), tol, ids=ids, x0=100, y0=40)
    assert got.tolist() == np.stack([ii[2:] + 100, jj[2:] + 40], axis=1).tolist()
    none = select_noisy(torch.from_numpy(color), torch.from_numpy(v), 8, float("inf"))
    assert tuple(none.shape) == (0, 2) and none.dtype == torch.int32
    with pytest.raises(ValueError):
        select_noisy(torch.from_numpy(color)[None], torch.from_numpy(v), 8, tol)


def test_symbols_exist_and_reject_a_null_context():
    """Both entry points are bound; a null context is MM_ERR_INVALID."""
    from mirror_maze import Renderer, _lib

    L = _lib.lib()
    assert "mm_trace_tile_var" in _lib.EXPORTS and "mm_trace_pixels_var" in _lib.EXPORTS
    assert L.mm_trace_tile_var(None, None, None, None, 1, 0, 0, 1, 1, 1, None, None, None) == _lib.MM_ERR_INVALID
    assert L.mm_trace_pixels_var(None, None, None, None, 0, None, None, None) == _lib.MM_ERR_INVALID
    for name in ("trace_tile_var", "trace_pixels_var", "refine"):
        assert callable(getattr(Renderer, name))


def test_refine_tolerance_from_the_reference(ref):
    """The condition of the GPU refine test, from the reference alone: on the
    8-spp frame of the walk's turned camera at 160x120, rel_tol =
    variance_support.REFINE_REL_TOL selects REFINE_SELECTED of the 19200
    pixels -- between 10 % and 50 % --, no pixel is within 1e-4 (relative) of
    the threshold, and select_noisy names exactly those pixels."""
    import torch

    from mirror_maze import make_ext, select_noisy

    vw, vh = V.REFINE_VIEW
    out, var = ref.tile(V.refine_uniform(), make_ext(V.REFINE_SPP, 8, 8, frame=V.REFINE_FRAME), 0, 0, vw, vh)
    want, margin = V.noisy_numpy(out, var, V.REFINE_SPP, V.REFINE_REL_TOL)
    assert int(want.sum()) == V.REFINE_SELECTED and 0.1 < want.mean() < 0.5
    assert margin.min() > 1e-4
    px = select_noisy(torch.from_numpy(out), torch.from_numpy(var), V.REFINE_SPP, V.REFINE_REL_TOL)
    jj, ii = np.nonzero(want)
    assert px.tolist() == np.stack([ii, jj], axis=1).tolist()


def test_flythrough_refine_argument(capsys):
    """--refine TOL[:SPP[:ROUNDS]] parses and is refused when malformed; with
    --no-render nothing is rendered."""
    import importlib.util
    import sys
    from pathlib import Path

    path0 = list(sys.path)
    try:
        spec = importlib.util.spec_from_file_location("flythrough_refine",
                                                      Path(V.REPO) / "scripts" / "flythrough.py")
        fly = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(fly)
        base = ["--maze", "4", "--frames", "3", "--width", "64", "--height", "48", "--no-render"]
        for value in ("0.2", "0.2:16", "0.1:24:3"):
            assert fly.main([*base, "--refine", value]) == 0
            assert len([ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("frame ")]) == 3
        for bad in ("tol", "0.2:1", "0.2:8:0", "-1", "0.2:8:2:1"):
            with pytest.raises(SystemExit):
                fly.main([*base, "--refine", bad])
        capsys.readouterr()
    finally:
        sys.path[:] = path0
