"""Exact rewrites of IEEE operations, checked exhaustively on the MI355X.

mm::rsq (mm_device.h) computes the reference's fast_rsqrt with its IEEE
meaning -- RN(1 / RN(sqrt(x))), the AIR intrinsic as the oracle states it --
from the hardware v_sqrt_f32 / v_rcp_f32 with exact corrections on
[2^-40, 2^40].  lib/verify_fast_rsq (scripts/verify_fast_rsq.hip, built by the
library's Makefile with its flags) compares it with the IEEE expansion
1.0f / sqrtf(x) for every float x in [2^-44, 2^44], and mm::rcp_guarded (the
per-ray RN(1/d) the Markstein quotients read: one Newton step on v_rcp_f32)
with 1.0f / d for every d of either sign with |d| in [2^-40, 2^40]; and
mm::ray_fast_ok_boxed (the per-query guard as integer compares on the
magnitudes' bits) with mm::ray_fast_ok on every 32-bit pattern.

Those rows compare two device computations.  The ieee_* rows compare the
device with values computed in the program's host code -- a / d, sqrtf(x) and
1.0f / sqrtf(x) in float, cross-checked there against the double-precision
route rounded once (host_ref) -- over 4100 mantissas (0, 1, 0x7FFFFF, 0x7FFFFE
and 4096 seeded ones) in each of the 277 binades from the smallest denormal to
the largest finite float, plus +-0, +-inf, NaN: the device's sqrtf and mm::rsq
(rsq_ieee outside [2^-40, 2^40], the branch the cameras of
tests/test_gpu_guard_edges.py reach), a / d, and the Markstein quotient
qdiv(a, d, rcp_guarded(d)) inside the guarded ranges for nonzero a; cvt_u32_sat
and unorm8 against host restatements around 0, 2^32, the 0.5 / 255 ties, NaN
and +-inf.  markstein_zero pins qdiv's zeros: a = +-0 gives the zero a / d is,
except +0 for a = -0 over d > 0 (measured on the MI355X: 20466 such pairs of a
first sample differed from a / d in that one bit and in nothing else; every
caller compares the quotient, mm_trace.h qdiv)."""
from __future__ import annotations

import subprocess

import pytest

from conftest import PKG

pytestmark = pytest.mark.gpu


def test_fast_rsq_is_bit_identical_to_the_ieee_expansion(gpu):
    exe = PKG / "lib" / "verify_fast_rsq"
    assert exe.exists(), "build the library first (make -C mirror-maze_amd)"
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0, p.stdout + p.stderr
    rows = {ln.split()[0]: ln.split() for ln in p.stdout.splitlines() if ln.strip()}
    for name, binades in (("rsq", 88), ("rcp_guarded", 80)):  # (rcp_guarded: each value with both signs)
        w = rows[name]
        checked, bad = int(w[2]), int(w[4])
        assert checked > binades * (1 << 23) and bad == 0, w
    # the per-query guard in integer form (mm::ray_fast_ok_boxed) equals the
    # float compares on every 32-bit pattern (origin: where the box can pass)
    w = rows["ray_guard"]
    assert int(w[2]) == 1 << 32 and int(w[4]) == 0, w
    # device against host: the sample sizes of scripts/verify_fast_rsq.hip check_against_host
    per_binade, specials = 4 + 4096, 8
    unary = (23 + 254) * per_binade + specials           # every binade, denormal ones included
    guarded = 4 * (80 * per_binade + 1)                  # |d| in [2^-40, 2^40], four a per d
    small = specials + 2 * 18 + 256 * 2 * 5              # conversions: the listed values, k / 255 and (k + 0.5) / 255 +- 2 ulp
    sizes = {"ieee_sqrt": unary, "ieee_rsq": unary, "ieee_div": 2 * unary, "ieee_div_markstein": guarded,
             "markstein_zero": guarded, "cvt_u32_sat": small, "unorm8": small, "host_ref": 4 * unary + guarded}
    for name, n in sizes.items():
        w = rows[name]
        assert int(w[2]) == n and int(w[4]) == 0, w
