"""The grid search's fast certificate (mm_grid.h: the hit point inside R*'s inner window, from an origin within
omax) against the full one (R*'s reference leaf box passes intersect_aabb at every t > best), on the CPU twin
of both (tests/cert_fast_ref.c): wherever the fast one passes the full one must.  The answers (best, R*) are
the reference walk's (tests/aov_ref.c).  Also: the windows the host build writes into the grid image are the
twin's, bit for bit, so the twin's verdicts are about the data the kernels read."""
from __future__ import annotations

import numpy as np
import pytest

import aov_support as A
import cert_fast_support as S
import grid_forms_support as G

ROWS = (7, 240, 479)  # rows of a 640 x 480 frame of the N = 10 maze: sky and far walls, the horizon, the floor


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return S.build_twin(tmp_path_factory.mktemp("cert_fast_ref"))


@pytest.fixture(scope="module")
def ref_lib(tmp_path_factory):
    return A.build_ref(tmp_path_factory.mktemp("aov_ref"))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("grid_forms_host")
    exe = G.build_host(tmp)
    return lambda rects: G.run_host(exe, rects, tmp, dump=True)


def _scenes():
    return {"maze": S.maze(), "gallery": G.scene("base")[0]}


@pytest.mark.parametrize("name", ["maze", "gallery"])
def test_host_windows_are_the_twins(twin, host, name):
    """The 24 B per rect at off_box of the image grid_build.cpp makes are the twin's windows; every bounded
    window, with the rounding of its test, lies at least m inside its leaf's box; exactly the rects with area are covered."""
    s = _scenes()[name]
    c = S.Certs(twin, s)
    f, image = host(s.rects)
    assert f["flat_ok"] == 1
    win = np.frombuffer(image, dtype=np.float32, count=6 * s.n_rects, offset=f["off_box"]).reshape(-1, 3, 2)
    assert np.array_equal(win.view(np.uint32), c.win.view(np.uint32))
    covered = c.win[np.arange(s.n_rects), np.maximum(c.axis, 0), 1] == np.inf  # (half-width on the normal axis)
    # every rect with area is covered (the maze also holds zero-area rects, which nothing hits)
    area = (np.abs(s.rects[:, 3:6]).max(axis=1) > 0) & (np.abs(s.rects[:, 6:9]).max(axis=1) > 0)
    assert np.array_equal(covered, area), (int(covered.sum()), int(area.sum()))
    b, w = c.box[covered].astype(np.float64), c.win[covered].astype(np.float64)
    fin = np.isfinite(w[..., 1])
    reach = w[..., 1] * (1.0 + 2.0 ** -23)  # |RN(p - c)| <= h admits |p - c| up to this
    assert (w[..., 0][fin] - reach[fin] >= b[..., 0][fin] + c.m).all()
    assert (w[..., 0][fin] + reach[fin] <= b[..., 1][fin] - c.m).all()
    assert (fin.sum(axis=1) == 2).all()  # the normal axis, and only it, is unbounded
    assert (c.win[~covered][..., 1] == -1.0).all()


def test_every_query_of_some_maze_rows(twin, ref_lib):
    """Every query of three rows of a 640 x 480 frame of the N = 10 maze at 8 spp, 8 / 8 bounces (the walk's own
    record of them): fast => full and
    fast => the proof's condition (cert_fast_support.sufficient), and nearly all of them are fast (the kernel's
    common path)."""
    from mirror_maze import default_uniform, make_ext

    s = S.maze()
    ref, c = A.Ref(ref_lib, s), S.Certs(twin, s)
    u, e = default_uniform(640, 480, 0), make_ext(8, 8, 8, frame=1)
    total = fast = 0
    for y in ROWS:
        _, q = ref.recorded(lambda: ref.trace_tile(u, e, 0, y, 640, 1))
        q = q[S.guarded(q)]
        fl = c.flags(q)
        hit = fl != S.NO_CERT
        bad = hit & (fl & S.FAST != 0) & (fl & S.FULL == 0)
        assert not bad.any(), (y, int(bad.sum()), q[bad][:4])
        unsound = hit & (fl & S.FAST != 0) & ~S.sufficient(c, q)
        assert not unsound.any(), (y, int(unsound.sum()), q[unsound][:4])
        total += int(hit.sum())
        fast += int((hit & (fl & S.FAST != 0)).sum())
    print(f"rows {ROWS}: {total} certified queries, {fast} fast ({fast / total:.5f})")
    assert total > 100_000 and fast >= 0.99 * total, (total, fast)


@pytest.mark.parametrize("name", ["maze", "gallery"])
def test_aimed_rays(twin, ref_lib, name):
    """Rays aimed at the band (cert_fast_support.aimed_rays).  On every one the walk answers: fast => full, and
    fast => the condition the proof derives (cert_fast_support.sufficient, exact arithmetic), which does not
    depend on the full certificate ever failing (it never does on these rays).  That the rays bite: the same
    test without its margin (cert_fast_support.naive_fast: the hit point inside the leaf's box itself) accepts
    some of them in breach of that condition (maze 1, gallery 3).
    The construction is where it should be: of the rays that mm_query_rays brings to the certificate (inside
    the guards, origin in the grid box, answered) at least a quarter take the full certificate and at least a
    quarter the fast one (measured on the twin: maze 0.36 slow / 0.64 fast, gallery 0.57 / 0.43; printed), and
    the rays from the grid box's faces -- the largest |o| such a ray can have -- are on both sides too."""
    s = _scenes()[name]
    ref, c = A.Ref(ref_lib, s), S.Certs(twin, s)
    rays, target, kind, (t, k) = S.aimed_rays(s, c, ref)
    q = S.answered(rays, t, k)
    assert S.guarded(q).all()
    fl = c.flags(q)
    hit = fl != S.NO_CERT
    fast = hit & (fl & S.FAST != 0)
    bad = fast & (fl & S.FULL == 0)
    assert not bad.any(), (name, int(bad.sum()), q[bad][:4])
    unsound = fast & ~S.sufficient(c, q)
    assert not unsound.any(), (name, int(unsound.sum()), q[unsound][:4])
    breach = S.naive_fast(c, q) & ~S.sufficient(c, q)
    reach = hit & S.reaches(S.grid_of(s), q)
    n = int(reach.sum())
    slow_share, fast_share = float((reach & ~fast).sum()) / n, float((reach & fast).sum()) / n
    on_target = float((k[reach] == target[reach]).mean())
    per_kind = [(int((reach & (kind == j)).sum()), int((reach & fast & (kind == j)).sum())) for j in range(4)]
    far = hit & (kind == 3)
    print(f"{name}: {int(hit.sum())} of {len(rays)} answered, {n} reach the certificate on the device, on target "
          f"{on_target:.3f}, slow {slow_share:.3f}, fast {fast_share:.3f}, (reaching, fast) per origin kind {per_kind}, "
          f"beyond the box: {int(far.sum())} answered, {int((far & fast).sum())} fast; breaches of the test without margin {int(breach.sum())}, "
          f"full fails {int((hit & (fl & S.FULL == 0)).sum())}")
    assert breach.any()
    assert n >= 0.4 * len(rays)  # (kinds 0 - 2 are three quarters of the rays; 7 of the 15 offsets point out of the rect)
    assert slow_share >= 0.25 and fast_share >= 0.25, (name, slow_share, fast_share)
    for j in (0, 1, 2):  # each origin kind that reaches the certificate is on both paths
        assert 0 < per_kind[j][1] < per_kind[j][0], (j, per_kind)
    assert per_kind[3][0] == 0 and far.sum() > 0 and not (far & fast & (np.abs(q[:, 0:3]).max(axis=1) > c.omax)).any()


def test_bounce_rays_with_coarse_origins(twin, ref_lib):
    """The queries of tests/test_gpu_cert_fast.py's telephoto windows (cert_fast_support.telephoto_gallery), as the
    walk records them: bounce rays, which GridQuery takes without the box check, from origins rounded at
    ulp(D) = 2^-12 C.  None is beyond omax, and fast => full and fast => the proof's condition on every one.
    Measured: 1649 bounce rays, 753 at a certificate, all of them fast and none from outside the grid box (the
    gallery's planes lie on the hit points' float grid, and most diffuse bounces leave through the open roof).
    An origin beyond omax = 8 C needs a hit point rounded at more than C, i.e. a camera more than 2^23 C away;
    neighbouring float directions are then more than C apart at the scene -- grid_stress_support.telephoto
    records that at 2^20 C the pixels already share one direction -- so no traced frame brings such a lane to
    the kernel's `<= omax` clause, and mm_query_rays cannot either: its rays pass grid_ray_ok first, which
    holds |o| within C (1 + 2^-14).  On the device that clause is therefore always true in these tests; what it
    is for is checked on the twin, by test_aimed_rays' origins beyond the box."""
    from mirror_maze import make_ext

    s, u = S.telephoto_gallery()
    ref, c = A.Ref(ref_lib, s), S.Certs(twin, s)
    e = make_ext(8, 8, 8, frame=1)
    q = np.concatenate([ref.recorded(lambda: ref.trace_tile(u, e, x0, y0, 32, 16))[1] for (x0, y0) in S.TELE_WINDOWS])
    cam = np.frombuffer(bytes(u), dtype=np.float32, count=3)
    bounce = (q[:, 0:3] != cam).any(axis=1) & S.guarded(q)
    fl = c.flags(q)
    cert = bounce & (fl != S.NO_CERT)
    fast = cert & (fl & S.FAST != 0)
    print(f"telephoto: {len(q)} queries, {int(bounce.sum())} bounce rays, {int(cert.sum())} at a certificate, "
          f"{int(fast.sum())} fast, {int((cert & S.outside(S.grid_of(s), q[:, 0:3])).sum())} from outside the box")
    assert cert.sum() >= 500 and fast.sum() > 0
    assert (np.abs(q[cert, 0:3]).max(axis=1) <= c.omax).all()
    assert not (fast & (fl & S.FULL == 0)).any()
    assert not (fast & ~S.sufficient(c, q)).any()
