"""Rewritten forms of the trace kernel's bounce block and chunk prologue against
the forms they replace, bit for bit, on tests/bounce_identities.c -- a C
restatement of both, compiled with -ffp-contract=off.  The kernel uses the
walk's start cell clamped in float and shade_step's shared tail and side test;
msign and rsq's range check on the bits and the prologue's pix / w by
reciprocal and correction are exact too but gained nothing in the ISA census
and stayed out."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

HERE = Path(__file__).resolve().parent
N = 1_000_000


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = tmp_path_factory.mktemp("bounce_identities") / "libbounce_identities.so"
    subprocess.run(["gcc", "-O2", "-std=c11", "-fPIC", "-ffp-contract=off", "-Wall", "-shared", "-o", str(so),
                    str(HERE / "bounce_identities.c"), "-lm"], check=True)
    L = C.CDLL(str(so))
    P, U, Q = C.c_void_p, C.c_uint32, C.c_uint64
    for name, args in (("bi_msign", [P, Q]), ("bi_rsq_range", [P, Q, P]), ("bi_first_cell", [P, P, P, P, Q, P]),
                       ("bi_pix_div", [U, U, U, C.c_int]), ("bi_spp_shift", [U, U, U]), ("bi_tail", [P, P, P, Q])):
        f = getattr(L, name)
        f.argtypes, f.restype = args, Q
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _f32(*v):
    return np.array(v, dtype=np.float32)


def test_msign(lib):
    """Every float class -- +-0, the denormals' ends, the normals' ends, +-inf,
    quiet and signalling NaNs under both sign bits -- and 1e6 random patterns."""
    classes = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00800000,
                        0x80800000, 0x3F800000, 0xBF800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000,
                        0x7F800001, 0xFF800001, 0x7FC00000, 0xFFC00000, 0x7FFFFFFF, 0xFFFFFFFF], dtype=np.uint32)
    rnd = np.random.default_rng(1).integers(0, 1 << 32, N, dtype=np.uint64).astype(np.uint32)
    bits = np.concatenate([classes, rnd])
    assert lib.bi_msign(_p(bits), bits.size) == 0


def test_rsq_range(lib):
    """The eight floats around 2^-40 and 2^40 (two below, the bound, one above
    -- and mirrored), their negatives, +-0, +-inf, NaNs, and random patterns."""
    lo, hi = 0x2B800000, 0x53800000
    edge = [lo - 2, lo - 1, lo, lo + 1, hi - 1, hi, hi + 1, hi + 2]
    bits = np.array(edge + [b | 0x80000000 for b in edge] +
                    [0, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF, 1,
                     0x80000001, 0xBF800000], dtype=np.uint32)
    n_fast = C.c_uint64(0)
    assert lib.bi_rsq_range(_p(bits), bits.size, C.byref(n_fast)) == 0
    assert n_fast.value == 4  # lo, lo + 1, hi - 1, hi: nothing else of the list is in range
    rnd = np.random.default_rng(2).integers(0, 1 << 32, N, dtype=np.uint64).astype(np.uint32)
    assert lib.bi_rsq_range(_p(rnd), rnd.size, C.byref(n_fast)) == 0
    assert 0 < n_fast.value < N


def test_first_cell(lib):
    """The float clamp of the start cell against the integer clamp: 1e6 random
    (o, mn, inv, nm1) -- a third inside the grid, a third up to a few cells
    outside, a third far outside (up to 1e30: the convert saturates) -- plus
    origins on exact cell boundaries, at -0, and non-finite ones."""
    g = np.random.default_rng(3)
    nm1 = g.integers(0, 64, N).astype(np.int32)
    cell = g.choice(_f32(10.0, 7.5, 1.0, 0.3333), N)
    inv = (np.float32(1.0) / cell).astype(np.float32)
    mn = g.uniform(-400, 10, N).astype(np.float32)
    u = g.uniform(0, 1, N)
    span = (nm1 + 1) * cell
    kind = g.integers(0, 3, N)
    o = np.where(kind == 0, mn + u * span,
                 np.where(kind == 1, mn + (u * 9 - 4) * cell + g.integers(0, 2, N) * span,
                          g.choice([-1.0, 1.0], N) * 10.0 ** g.uniform(3, 30, N))).astype(np.float32)
    # exact boundaries (mn + b cell for a power-of-two-free cell is inexact: use cell = 1 and integer mn)
    nb = 4096
    bmn = g.integers(-50, 50, nb).astype(np.float32)
    bnm1 = g.integers(0, 64, nb).astype(np.int32)
    bo = (bmn + g.integers(-3, 68, nb)).astype(np.float32)
    special = _f32(-0.0, 0.0, np.inf, -np.inf, np.nan, -1e-45, 1e-45, 3.4e38, -3.4e38)
    o = np.concatenate([o, bo, special])
    mn = np.concatenate([mn, bmn, np.zeros(special.size, np.float32)])
    inv = np.concatenate([inv, np.ones(nb, np.float32), np.ones(special.size, np.float32)])
    nm1 = np.concatenate([nm1, bnm1, np.full(special.size, 31, np.int32)])
    n_clamped = C.c_uint64(0)
    assert lib.bi_first_cell(_p(o), _p(mn), _p(inv), _p(nm1), o.size, C.byref(n_clamped)) == 0
    assert N // 4 < n_clamped.value < o.size  # the clamp was at work


@pytest.mark.parametrize("w", [1, 3, 64, 1919, 1920, 4093])
def test_pix_div(lib, w):
    """Every pix in [0, 2^22): quotient and remainder, with the reciprocal
    estimate correctly rounded and one ulp to either side (the hardware's
    reciprocal is within one ulp)."""
    for ulps in (-1, 0, 1):
        assert lib.bi_pix_div(w, 0, 1 << 22, ulps) == 0


def test_pix_div_to_the_bound(lib):
    """The proof's bound: pix < 2^24 with a quotient below 2^22 (w >= 4)."""
    for w in (4, 5, 1920, (1 << 24) - 1):
        for ulps in (-1, 0, 1):
            assert lib.bi_pix_div(w, (1 << 24) - (1 << 20), 1 << 24, ulps) == 0


@pytest.mark.parametrize("spp", [1, 2, 8, 64])
def test_spp_shift(lib, spp):
    assert lib.bi_spp_shift(spp, 0, 1 << 22) == 0
    assert lib.bi_spp_shift(spp, 0xFFFF0000, 0xFFFFFFFF) == 0


def test_shared_tail(lib):
    """1e6 random (dir, nn, rn): unit-scale vectors, axis-aligned normals of
    both signs (the maze's) and directions with zero components among them."""
    g = np.random.default_rng(4)
    d = g.normal(size=(N, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True).astype(np.float32)
    nn = g.normal(size=(N, 3)).astype(np.float32)
    nn /= np.linalg.norm(nn, axis=1, keepdims=True).astype(np.float32)
    ax = np.eye(3, dtype=np.float32)[g.integers(0, 3, N // 2)] * g.choice(_f32(-1.0, 1.0), (N // 2, 1))
    nn[: N // 2] = ax
    d[:1000, 0] = 0.0
    d[1000:2000, 1] = -0.0
    d[2000:3000] = ax[2000:3000]  # head-on: dot = +-1
    rn = g.normal(size=(N, 3)).astype(np.float32)
    d, nn, rn = (np.ascontiguousarray(a, dtype=np.float32) for a in (d, nn, rn))
    assert lib.bi_tail(_p(d), _p(nn), _p(rn), N) == 0
