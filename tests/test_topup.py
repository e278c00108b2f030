"""CPU tests of the top-up path: the C reference of mm_blend_pixels
(tests/topup_ref.c) against a float32 numpy statement of include/mm_api.h's
definition, the pixel-selection helper on CPU tensors, the launch plan of a
pixel-list launch (mm_plan.cpp plan_pixels), the argument checks of
mm_blend_pixels, and the count of short-history pixels the GPU end-to-end test
relies on."""
from __future__ import annotations

import ctypes as C
import json
import subprocess
from pathlib import Path

import numpy as np
import pytest

import aov_support as A
import temporal_support as T
import topup_support as S

REPO = Path(__file__).resolve().parents[1]
CSRC = REPO / "mirror-maze_amd" / "csrc"
MM_OK, MM_ERR_INVALID, MM_ERR_UNSUPPORTED = 0, -1, -6
MM_PIPE_WAVEFRONT, MM_PIPE_REFERENCE = 2, 3


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def tu_lib(tmp_path_factory):
    return S.build_ref(tmp_path_factory.mktemp("topup_ref"))


@pytest.mark.parametrize("m", S.WEIGHTS)
def test_reference_is_the_header_statement(tu_lib, m):
    """10. topup_ref.c and the numpy statement agree on every bit, on the
    inputs the GPU test blends."""
    image, px, extra = S.blend_inputs()
    x0, y0, w, h = S.WINDOW
    got, inside = S.blend_ref(tu_lib, image, x0, y0, px, extra, m)
    want = S.blend_numpy(image, x0, y0, px, extra, m)
    assert inside == 120 and len(px) == 160
    assert np.array_equal(_bits(got), _bits(want))
    # listed pixels end with alpha + m, the others keep their bits
    listed = np.zeros((h, w), bool)
    for x, y in px.astype(np.int64):
        if x0 <= x < x0 + w and y0 <= y < y0 + h:
            listed[y - y0, x - x0] = True
    assert listed.sum() == 120
    assert np.array_equal(got[listed][:, 3], image[listed][:, 3] + np.float32(m))
    assert np.array_equal(_bits(got[~listed]), _bits(image[~listed]))
    assert not np.array_equal(_bits(got[listed][:, :3]), _bits(image[listed][:, :3]))
    assert set(np.unique(image[..., 3])) == set(S.ALPHAS)


def test_reference_driver_runs_clean(tmp_path):
    """The reference's stand-alone driver, plain and under the address and
    undefined-behaviour sanitizers (a host program of its own); both builds
    print the same checksum."""
    outs = []
    for name, flags in (("plain", ()), ("sanitized", ("-O1", "-g", "-fsanitize=address,undefined",
                                                      "-fno-sanitize-recover=all"))):
        (tmp_path / name).mkdir()
        exe = S.build_driver(tmp_path / name, flags)
        r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
        assert r.stdout.startswith("inside ") and "checksum" in r.stdout
        outs.append(r.stdout)
    assert outs[0] == outs[1]


def test_selection_helper_on_cpu_tensors():
    """11. Threshold, MISS / FAILED exclusion, row-major order, window offset,
    empty result."""
    import torch

    from mirror_maze import MM_AOV_ID_FAILED, MM_AOV_ID_MISS, select_short_history

    h, w = 4, 6
    acc = torch.zeros((h, w, 4), dtype=torch.float32)
    acc[..., 3] = 8.0
    ids = torch.full((h, w), 5 | 0x40000000, dtype=torch.int32)
    short = [(0, 0), (5, 0), (2, 1), (3, 1), (0, 3), (5, 3)]  # (x, y)
    alphas = [1.0, 1.5, 1.999, 1.0, 1.0, 1.0]
    for (x, y), a in zip(short, alphas):
        acc[y, x, 3] = a
    acc[2, 4, 3] = 2.0  # at the threshold: not short
    ids[1, 3] = MM_AOV_ID_MISS - (1 << 32)
    ids[3, 0] = MM_AOV_ID_FAILED - (1 << 32)
    got = select_short_history(acc, ids, 2.0)
    assert got.dtype == torch.int32 and got.is_contiguous() and got.device.type == "cpu"
    assert got.tolist() == [[0, 0], [5, 0], [2, 1], [5, 3]]
    # a (1, h, w) id buffer, a window offset, another threshold
    got = select_short_history(acc, ids.reshape(1, h, w), 1.75, x0=100, y0=40)
    assert got.tolist() == [[100, 40], [105, 40], [105, 43]]
    none = select_short_history(acc, ids, 1.0)
    assert tuple(none.shape) == (0, 2) and none.dtype == torch.int32
    with pytest.raises(ValueError):
        select_short_history(acc[None], ids, 2.0)


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = tmp_path_factory.mktemp("plan_pixels") / "plan_pixels_test"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", f"-I{CSRC}", f"-I{REPO / 'include'}", "-o", str(exe),
                    str(Path(__file__).resolve().parent / "topup" / "plan_pixels_test.cpp"), str(CSRC / "mm_plan.cpp")],
                   check=True)

    def run(**kw):
        r = subprocess.run([str(exe), *(f"{k}={v}" for k, v in kw.items())], capture_output=True, text=True,
                           timeout=60)
        assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
        return json.loads(r.stdout)

    return run


def test_list_launch_plan(plan):
    """12. Never deferral; fuse iff 64 % spp == 0 (and MM_OPT_FUSE_RESOLVE);
    the queue and staging bounds are MM_ERR_INVALID."""
    for spp in (1, 2, 3, 4, 5, 8, 12, 16, 24, 32, 64, 96, 128, 4096):
        for defer, defer_min in ((-1, 1 << 24), (0, 0), (32, 0), (64, 0), (32, 1 << 24)):
            for n in (1, 185, 1 << 22):
                if n * spp > 2**29 and 64 % spp:
                    continue
                p = plan(n=n, spp=spp, defer=defer, defer_min=defer_min)
                assert p["code"] == MM_OK, p
                assert not p["defer"] and p["ring"] == 0 and p["rows_per_batch"] == 1
                assert p["fuse"] == (64 % spp == 0), (spp, p)
    assert not plan(spp=8, fuse=0)["fuse"]
    p = plan(spp=8, pipe=MM_PIPE_REFERENCE)
    assert p["code"] == MM_OK and not p["fuse"] and not p["defer"]
    # the pre-pass is the tile launch's
    assert (plan(bounce=8)["predraw"], plan(bounce=8)["predraw_pool"]) == (14, 7)
    r = plan(pipe=MM_PIPE_WAVEFRONT)
    assert r["code"] == MM_ERR_UNSUPPORTED and "MM_PIPE_WAVEFRONT" in r["error"]
    # the staging cap: 2^29 staged paths
    assert plan(n=2**29 // 3, spp=3)["code"] == MM_OK
    r = plan(n=2**29 // 3 + 1, spp=3)
    assert r["code"] == MM_ERR_INVALID
    assert r["error"] == "mm_trace_pixels: the list's staged samples exceed 6 GiB (2^29 paths); use a shorter list"
    assert plan(n=2**26, spp=8, fuse=0)["code"] == MM_OK
    assert plan(n=2**26 + 1, spp=8, fuse=0)["code"] == MM_ERR_INVALID
    assert plan(n=2**26 + 1, spp=8, pipe=MM_PIPE_REFERENCE)["code"] == MM_ERR_INVALID
    assert plan(n=2**26 + 1, spp=8)["code"] == MM_OK  # fused: nothing staged
    # the 32-bit queue: chunks padded to 64, less the 2^24 the waves' last claims may overshoot
    top = 2**32 - 1 - 2**24
    assert plan(n=top // 64 * 64, spp=1)["code"] == MM_OK
    for n, spp in ((top // 64 * 64 + 1, 1), (2**32 - 2**24, 1), (2**20, 4096), (2**32, 1), (2**40, 1), (2**62, 8)):
        r = plan(n=n, spp=spp)
        assert r["code"] == MM_ERR_INVALID and r["error"] == "mm_trace_pixels: more paths than one launch holds (2^32)"


def test_blend_symbol_exists_and_rejects_bad_arguments_without_a_gpu():
    """mm_blend_pixels' argument checks need no context, so they run here."""
    from mirror_maze import _lib

    L = _lib.lib()
    assert "mm_blend_pixels" in _lib.EXPORTS and "mm_trace_pixels" in _lib.EXPORTS
    inv = _lib.MM_ERR_INVALID
    buf = (C.c_float * 256)()  # 16-byte aligned stand-ins; never dereferenced
    base = (C.addressof(buf) + 15) & ~15
    image, px, extra = base, base + 256, base + 512
    good = dict(image=image, x0=0, y0=0, w=4, h=4, px=px, extra=extra, n=4, m=3.0)

    def call(**kw):
        a = {**good, **kw}
        return L.mm_blend_pixels(None, a["image"], a["x0"], a["y0"], a["w"], a["h"], a["px"], a["extra"], a["n"], a["m"])

    assert call() == inv  # with everything in order the null context is what is left to refuse
    assert call(n=0) == inv
    for kw in (dict(image=None), dict(px=None), dict(extra=None), dict(image=image + 4), dict(px=px + 4),
               dict(extra=extra + 8), dict(w=0), dict(h=0), dict(w=1 << 16, h=1 << 15), dict(m=0.0), dict(m=-1.0),
               dict(m=float("nan")), dict(m=float("inf")), dict(extra=image), dict(extra=image + 16 * 15),
               dict(image=extra + 16 * 3)):
        assert call(**kw) == inv, kw
    assert L.mm_trace_pixels(None, None, None, None, 0, None, None) == inv


def test_walk_selects_enough_pixels(tmp_path_factory):
    """The condition of the GPU end-to-end test, on the CPU: the walk's last
    frame, accumulated by tests/temporal_ref.c over aov_ref.c's guides (what
    mm_trace_aov writes; no decision of the accumulation depends on a colour),
    has topup_support.WALK_SELECTED = 3569 pixels with N < 2 that are neither
    MISS nor FAILED -- at least 300."""
    import torch

    from mirror_maze import select_short_history

    tp = T.build_ref(tmp_path_factory.mktemp("temporal_ref"))
    al = A.build_ref(tmp_path_factory.mktemp("aov_ref"))
    s, u = T.scene_view("maze4")
    vw, vh = S.WALK_VIEW
    u.view_w, u.view_h = float(vw), float(vh)
    cams = S.walk_cameras()
    ref = A.Ref(al, s)
    gs = []
    for cam in cams:
        C.memmove(C.byref(u), np.ascontiguousarray(cam, dtype=np.float32).ctypes.data, 40)
        gs.append(ref.tile(u, T.MIRROR_LIMIT, 0, 0, vw, vh))
    g = {k: np.stack([x[k] for x in gs]) for k in T.NAMES}
    color = np.random.default_rng(1).uniform(0, 1, size=(4, vh, vw, 4)).astype(np.float32)
    out, _ = T.accumulate_ref(tp, (vw, vh), cams, color, g, **T.DEFAULTS)
    ids = np.asarray(g["id"][3]).view(np.uint32)
    n = int(((out[3, ..., 3] < 2) & (ids < 0xFFFFFFFE)).sum())
    assert n == S.WALK_SELECTED >= 300
    px = select_short_history(torch.from_numpy(out[3]), torch.from_numpy(ids.view(np.int32).copy()), 2.0)
    assert px.shape[0] == n
    # the turn, not the walk, leaves them short: the frame before has its full history almost everywhere
    assert (out[2, ..., 3] >= 2).mean() > 0.95


def test_flythrough_top_up_argument(capsys):
    """--top-up N[:SPP] parses with --accumulate and is refused without it or
    with a malformed value; with --no-render nothing is rendered."""
    import importlib.util
    import sys

    path0 = list(sys.path)
    try:
        spec = importlib.util.spec_from_file_location("flythrough_topup", REPO / "scripts" / "flythrough.py")
        fly = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(fly)
        base = ["--maze", "4", "--frames", "3", "--width", "64", "--height", "48", "--no-render"]
        for value in ("2", "2:24", "4.5:1"):
            assert fly.main([*base, "--accumulate", "--top-up", value]) == 0
            assert len([ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("frame ")]) == 3
        for bad in ([*base, "--top-up", "2"], [*base, "--accumulate", "--top-up", "two"],
                    [*base, "--accumulate", "--top-up", "2:0"], [*base, "--accumulate", "--top-up", "1"]):
            with pytest.raises(SystemExit):
                fly.main(bad)
        capsys.readouterr()
    finally:
        sys.path[:] = path0
