"""CPU test of the launch policy (mirror-maze_amd/csrc/mm_plan.cpp): query method, LDS placement, tail deferral
and its ring kind, fused resolve, the staging bound and rows per launch, as pure functions of scene facts,
options and the tile.  tests/launch_plan/launch_plan_test.cpp builds the N = 10 / 32 / 64 mazes as
mm_upload_scene does and prints the plan of one call; the expected plans are the ones the GPU suite asserts on
full-size frames (test_gpu_grid.py test_auto_tail_deferral_policy, test_gpu_camera_sequence.py
test_staging_bound_for_multi_frame_launches, test_gpu_random_scene.py).  Built twice: plain, and with the
address and undefined-behaviour sanitizers (a stand-alone host program).
"""
from __future__ import annotations

import json
import subprocess
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parents[1]
CSRC = REPO / "mirror-maze_amd" / "csrc"
SRC = [Path(__file__).resolve().parent / "launch_plan" / "launch_plan_test.cpp",
       *(CSRC / f for f in ("scene.cpp", "rect_compact.cpp", "grid_build.cpp", "mm_plan.cpp"))]
BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}

MM_OK, MM_ERR_INVALID, MM_ERR_UNSUPPORTED = 0, -1, -6
MM_PIPE_WAVEFRONT = 2
MM_EXT_ACCUMULATE = 2
FRAMES, CAMERAS = "mm_trace_tile_frames", "mm_trace_tile_cameras"
LDS_PER_BLOCK = 80 * 1024
# rank 0's rows of an 8-way row split of 1920x1080
RANK0 = dict(w=1920, h=135)


@pytest.fixture(scope="module", params=list(BUILDS))
def plan(request, tmp_path_factory):
    exe = tmp_path_factory.mktemp("launch_plan") / f"launch_plan_{request.param}"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *BUILDS[request.param], f"-I{CSRC}",
                    f"-I{REPO / 'include'}", "-o", str(exe), *map(str, SRC)], check=True)

    def run(**kw):
        r = subprocess.run([str(exe), *(f"{k}={v}" for k, v in kw.items())], capture_output=True, text=True,
                           timeout=60)
        assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
        return json.loads(r.stdout)

    return run


def ok(r):
    """The plan of a call every stage accepted."""
    assert r["method"]["code"] == MM_OK and r["placement"]["code"] == MM_OK and r["plan"]["code"] == MM_OK, r
    return r["plan"]


def test_c3_scene_plans(plan):
    """N = 32, 1920x1080, 8 spp, 8/8 bounces: the whole grid image in LDS; deferral from 2^24 paths on."""
    r = plan(n=32)  # one frame: 16.6 M paths
    assert r["facts"]["grid_ok"] and r["facts"]["grid_flat"] and r["facts"]["lean_ok"]
    assert r["placement"]["mode"] == 11 and r["placement"]["built"]
    p = ok(r)
    assert not p["defer"] and p["ring"] == 0 and p["fuse"] and p["rows_per_batch"] == 1080
    p = ok(plan(n=32, frames=20, multi=FRAMES, **RANK0))  # 41 M paths
    assert p["defer"] and p["ring"] == 2 and not p["fuse"] and p["rows_per_batch"] == 135
    p = ok(plan(n=32, frames=2, multi=FRAMES, bounce=4, mirror=4))  # short paths: no deferral at any size
    assert not p["defer"] and p["fuse"]
    p = ok(plan(n=32, frames=20, multi=FRAMES, defer=0, **RANK0))
    assert not p["defer"] and p["fuse"]
    p = ok(plan(n=32, w=16, h=8, pipe=MM_PIPE_WAVEFRONT))  # always on
    assert p["defer"] and p["ring"] == 2 and not p["fuse"]
    p = ok(plan(n=32, w=16, h=8, defer=32))  # forced on, but below MM_OPT_DEFER_MIN paths
    assert not p["defer"]
    p = ok(plan(n=32, w=16, h=8, defer=32, defer_min=0))
    assert p["defer"] and p["ring"] == 2


def test_n64_scene_plan(plan):
    """N = 64: records + class table + index in LDS (mode 14), leaf boxes global; no deferral there."""
    r = plan(n=64, bounce=16, mirror=16, frames=20, multi=FRAMES)
    assert r["facts"]["bytes"] > LDS_PER_BLOCK >= r["facts"]["off_box"]
    assert r["placement"]["mode"] == 14 and r["placement"]["built"]
    p = ok(r)
    assert not p["defer"] and p["fuse"]
    # samples staged anyway (64 % spp != 0): deferral on, and the rings' records in global memory (no room)
    p = ok(plan(n=64, bounce=16, mirror=16, spp=3, frames=20, multi=FRAMES))
    assert p["defer"] and p["ring"] == 1


def test_staging_bound(plan):
    # 33 frames of 1920x1080 at 8 spp: more than 2^29 paths -> fused resolve instead of the rings
    assert 33 * 1920 * 1080 * 8 > 2**29 > 32 * 1920 * 1080 * 8
    p = ok(plan(n=32, frames=32, multi=CAMERAS))
    assert p["defer"] and not p["fuse"]
    p = ok(plan(n=32, frames=33, multi=CAMERAS))
    assert not p["defer"] and p["ring"] == 0 and p["fuse"] and p["rows_per_batch"] == 1080
    # 3 spp cannot fuse: refused
    assert 87 * 1920 * 1080 * 3 > 2**29 > 86 * 1920 * 1080 * 3
    p = ok(plan(n=32, spp=3, frames=86, multi=CAMERAS))
    assert p["defer"] and not p["fuse"]
    r = plan(n=32, spp=3, frames=87, multi=CAMERAS)
    assert r["plan"]["code"] == MM_ERR_INVALID
    assert r["plan"]["error"] == ("mm_trace_tile_cameras: the frames' staged samples exceed 6 GiB (2^29 paths) per "
                                  "launch; use fewer frames per launch")
    # a single frame over the bound is split into row batches
    p = ok(plan(n=32, spp=3, w=65536, h=4096))
    assert p["defer"] and p["rows_per_batch"] == 2**29 // (65536 * 3) < 4096


def test_ring_kind_by_lds_room(plan):
    """A dynamic-LDS placement (BVH nodes + records, mode 3): the ring kind whose static LDS still fits."""
    base = dict(n=10, ww=7, defer=32, defer_min=0)
    r = plan(**base, s1="room+0", s2="room+0")
    assert r["placement"]["mode"] == 3 and r["placement"]["form"] == 7 and r["placement"]["defer_built"]
    assert r["placement"]["staged"] == 32 * r["facts"]["n_nodes"] + 40 * r["facts"]["n_rects"] < LDS_PER_BLOCK
    p = ok(r)
    assert p["defer"] and p["ring"] == 2
    p = ok(plan(**base, s1="room+0", s2="room+1"))  # kind 2 is one byte over
    assert p["defer"] and p["ring"] == 1
    p = ok(plan(**base, s1="room-16", s2="nb"))
    assert p["defer"] and p["ring"] == 1
    for s1, s2 in (("room+1", "room+1"), ("nb", "nb"), ("nb", "room+16")):
        p = ok(plan(**base, s1=s1, s2=s2))
        assert not p["defer"] and p["ring"] == 0 and p["fuse"]
        r = plan(**base, s1=s1, s2=s2, pipe=MM_PIPE_WAVEFRONT)
        assert r["plan"]["code"] == MM_ERR_UNSUPPORTED
        assert r["plan"]["error"] == "MM_PIPE_WAVEFRONT: grid image + tail ring exceed the LDS budget"
    # no deferral kernel for the placement at all
    r = plan(n=10, ww=5, pipe=MM_PIPE_WAVEFRONT)
    assert r["placement"]["mode"] == 3 and r["placement"]["form"] == 5 and not r["placement"]["defer_built"]
    assert r["plan"]["code"] == MM_ERR_UNSUPPORTED
    assert r["plan"]["error"] == ("MM_PIPE_WAVEFRONT: no tail-deferral kernel for this scene's query method / LDS "
                                  "placement (grid search, or BVH form 7 with nodes + records in LDS)")


def test_method_errors(plan):
    r = plan(n=10, ww=11, grid_ok=0)
    assert r["method"]["code"] == MM_ERR_UNSUPPORTED
    assert r["method"]["error"] == "grid search unavailable for this scene: overridden by the test"
    r = plan(n=10, ww=7, lean_ok=0)
    assert r["method"]["code"] == MM_ERR_UNSUPPORTED
    assert r["method"]["error"] == "loop form 7 needs compact records for every rect"
    for kw in (dict(grid_slow=1), dict(lean_ok=0)):
        r = plan(n=32, **kw)
        assert r["facts"]["grid_flat"]
        assert r["method"]["code"] == MM_ERR_UNSUPPORTED and r["method"]["error"] == "maze grid with SLOW records"
    # auto without a grid: the lean BVH loop, or form 5 without compact records
    assert plan(n=10, grid_ok=0)["placement"]["form"] == 7
    assert plan(n=10, grid_ok=0, lean_ok=0)["placement"]["form"] == 5
    # forced form 7 whose nodes + records do not fit LDS
    r = plan(n=64, ww=7)
    assert r["placement"]["code"] == MM_ERR_UNSUPPORTED
    assert r["placement"]["error"] == ("loop form 7 needs the BVH nodes + compact records in LDS (its other "
                                       "placements measured slower and were removed, DESIGN.md §4)")


def test_multi_frame_refusals(plan):
    r = plan(n=32, spp=3, defer=0, frames=2, multi=FRAMES)
    assert r["plan"]["code"] == MM_ERR_UNSUPPORTED
    assert r["plan"]["error"] == ("mm_trace_tile_frames: needs the wave-persistent kernel with the fused resolve "
                                  "(64 % spp == 0) or tail deferral")
    r = plan(n=32, frames=2, multi=CAMERAS, flags=MM_EXT_ACCUMULATE)
    assert r["plan"]["code"] == MM_ERR_INVALID
    assert r["plan"]["error"] == "mm_trace_tile_cameras: frames of one launch cannot accumulate into one image"
    assert 258 * 1920 * 1080 * 8 + 2**24 > 2**32 - 1 >= 257 * 1920 * 1080 * 8 + 2**24
    assert ok(plan(n=32, frames=257, multi=FRAMES))["fuse"]
    r = plan(n=32, frames=258, multi=FRAMES)
    assert r["plan"]["code"] == MM_ERR_INVALID
    assert r["plan"]["error"] == "mm_trace_tile_frames: more paths than one launch holds (2^32)"
    # one frame of more than 2^31 paths: two row batches, which a multi-frame entry point refuses
    p = ok(plan(n=32, w=65536, h=4100, defer=0))
    assert p["fuse"] and p["rows_per_batch"] == 4096
    r = plan(n=32, w=65536, h=4100, multi=CAMERAS)
    assert r["plan"]["code"] == MM_ERR_INVALID
    assert r["plan"]["error"] == "mm_trace_tile_cameras: tile too large for one launch"


@pytest.mark.parametrize("n", [10, 32, 64])
def test_every_chosen_variant_is_built(plan, n):
    """Whatever (placement, form) choose_placement returns for these scenes and options is an instantiated kernel."""
    seen = set()
    for ww in (-1, 5, 7, 11):
        for lds in (1, 0):
            for lds_rects in (1, 0):
                for grid_wide in (1, 0):
                    r = plan(n=n, ww=ww, lds=lds, lds_rects=lds_rects, grid_wide=grid_wide)
                    assert r["method"]["code"] == MM_OK, r
                    pl = r["placement"]
                    if pl["code"] != MM_OK:  # the one refusal: forced form 7 outside LDS
                        assert ww == 7 and "loop form 7 needs the BVH nodes + compact records in LDS" in pl["error"]
                        continue
                    assert pl["built"], pl
                    seen.add((pl["mode"], pl["form"]))
    # (not vacuous: grid placements and BVH placements were both chosen)
    assert any(mode >= 11 for mode, _ in seen) and any(mode < 11 for mode, _ in seen), seen
