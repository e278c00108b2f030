"""Feature buffers and batch ray queries, host side (no GPU): the two C-ABI
symbols, the mm_aov layout, the CPU reference (tests/aov_ref.c) against
itself, the input conditions the GPU tests (tests/test_gpu_aov.py) rely on,
and scripts/flythrough.py's --aov argument."""
from __future__ import annotations

import ctypes as C
import importlib.util
import re
import sys
from pathlib import Path

import numpy as np
import pytest

import aov_support as A

REPO = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def ref_lib(tmp_path_factory):
    return A.build_ref(tmp_path_factory.mktemp("aov_ref"))


@pytest.fixture(scope="module")
def corridor(ref_lib):
    s, u = A.corridor()
    return s, u, A.Ref(ref_lib, s)


def test_symbols_exist_and_reject_a_null_context():
    from mirror_maze import _lib

    L = _lib.lib()
    a = _lib.mm_aov(None, None, None)
    u = _lib.mm_uniform()
    assert L.mm_query_rays(None, None, 0, None) == _lib.MM_ERR_INVALID
    assert L.mm_query_rays(None, None, 5, None) == _lib.MM_ERR_INVALID
    assert L.mm_trace_aov(None, C.byref(u), None, 1, 15, 0, 0, 1, 1, 1, C.byref(a)) == _lib.MM_ERR_INVALID


def test_mm_aov_layout_matches_the_header():
    """ctypes mm_aov = the header's struct: three pointers in the header's order
    (the static assert in mm_layout_check.cpp pins the C side: 24 B, 8, 16)."""
    from mirror_maze import _lib

    txt = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "mm_types.h").read_text(), flags=re.S)
    body = re.search(r"typedef struct mm_aov \{(.*?)\} mm_aov;", txt, flags=re.S).group(1)
    fields = re.findall(r"(\w+)\s*\*\s*(\w+)\s*;", body)
    assert [f[1] for f in fields] == ["normal_depth", "albedo", "id"]
    assert [f[0] for f in fields] == ["float", "float", "uint32_t"]
    assert [n for n, _ in _lib.mm_aov._fields_] == [f[1] for f in fields]
    p = C.sizeof(C.c_void_p)
    assert C.sizeof(_lib.mm_aov) == 3 * p == 24
    assert (_lib.mm_aov.normal_depth.offset, _lib.mm_aov.albedo.offset, _lib.mm_aov.id.offset) == (0, 8, 16)
    check = (REPO / "mirror-maze_amd" / "csrc" / "mm_layout_check.cpp").read_text()
    assert "sizeof(mm_aov) == 24" in check and "offsetof(mm_aov, id) == 16" in check
    assert _lib.lib().mm_layout_ok() == 1


def test_corridor_golden_is_the_generator_s_scene():
    z = np.load(A.CORRIDOR)
    d = A.make_corridor()
    assert sorted(z.files) == sorted(d)
    for k, v in d.items():
        assert z[k].dtype == v.dtype and z[k].tobytes() == v.tobytes(), k
    # two parallel mirrors facing each other, matte floor and far wall
    assert list(z["is_mirror"]) == [1, 1, 0, 0]
    r = z["rects"]
    n0, n1 = np.cross(r[0, 3:6], r[0, 6:9]), np.cross(r[1, 3:6], r[1, 6:9])
    # (the kernel's normal is cross(v, u) in the IR's operand order: v x u)
    assert n0[0] > 0 and n1[0] < 0 and not n0[1:].any() and not n1[1:].any()
    assert r[0, 0] == -1.0 and r[1, 0] == 1.0


@pytest.mark.parametrize("scene_name", ["maze4", "corridor"])
def test_first_hit_buffers_equal_the_query_on_the_primary_ray(ref_lib, corridor, scene_name):
    """aovref_pixel with mirror_limit = 1 (and 0) is aovref_query on the
    pixel's primary ray: same rect, same t, normal turned against the ray."""
    from mirror_maze import Scene, default_uniform
    from oracle.oracle import lib as olib

    if scene_name == "corridor":
        s, u, ref = corridor
    else:
        s = Scene.build(4, 0)
        u = default_uniform(67, 48, 0)
        ref = A.Ref(ref_lib, s)
    seen = set()
    for py in range(0, 48, 5):
        for px in range(0, 67, 3):
            d = np.zeros(3, np.float32)
            olib().oracle_primary_dir(C.create_string_buffer(bytes(u), 56), px, py, d.ctypes.data)
            t, k = ref.query_one(list(u.cam.center), d)
            for limit in (0, 1):
                nd, al, i = ref.pixel(u, px, py, limit)
                if k == A.MISS:
                    assert i == A.MISS and nd.tolist() == [0, 0, 0, np.float32(1e30)] and not al.any()
                    assert t == np.float32(1e30)
                    continue
                assert i & A.RECT == k and i >> 30 in (1, 2)
                assert nd[3] == np.float32(t)  # dist = 0 + t
                assert al[3] == 0.0 and al[:3].tolist() == s.rects[k, 9:12].tolist()
                n = np.cross(s.rects[k, 3:6].astype(np.float64), s.rects[k, 6:9].astype(np.float64))
                assert np.dot(nd[:3], d) <= 0 and abs(abs(np.dot(nd[:3], n / np.linalg.norm(n))) - 1) < 1e-6
                assert (i >> 30 == 2) == bool(s.is_mirror[k] and np.dot(d, n) < 0)
            seen.add(k == A.MISS)
    assert seen == {True, False}


def test_corridor_covers_the_three_results_and_long_chains(corridor):
    """Input conditions of the GPU tests, on the helper alone: at mirror_limit
    = 15 each of MISS, SURFACE and MIRROR_END covers >= 1 % of the 67x48 pixels;
    at 200 some pixel's chain has >= 50 mirror hits."""
    s, u, ref = corridor
    t = ref.tile(u, 15, 0, 0, 67, 48)
    shares = [float(m.mean()) for m in A.kinds(t["id"])]
    print("corridor, mirror_limit 15: miss / surface / mirror_end shares", shares)
    assert all(x >= 0.01 for x in shares), shares
    assert abs(sum(shares) - 1.0) < 1e-12
    assert t["albedo"][..., 3].max() == 14.0
    t = ref.tile(u, 200, 0, 0, 67, 48)
    print("corridor, mirror_limit 200: longest chain", t["albedo"][..., 3].max())
    assert t["albedo"][..., 3].max() >= 50.0
    # the distance grows along a chain: a 14-hit chain is longer than the corridor is wide
    m = t["albedo"][..., 3] >= 14
    assert (t["normal_depth"][..., 3][m] > 14 * 2.0).all()


def test_maze_alone_is_a_poor_input(ref_lib):
    """Why the corridor exists: in the maze no chain is long (Scene.build(4, 0),
    default camera, mirror_limit 15)."""
    from mirror_maze import Scene, default_uniform

    s = Scene.build(4, 0)
    t = A.Ref(ref_lib, s).tile(default_uniform(67, 48, 0), 15, 0, 0, 67, 48)
    assert not A.kinds(t["id"])[2].any() and t["albedo"][..., 3].max() <= 3


def _flythrough():
    spec = importlib.util.spec_from_file_location("flythrough_aov", REPO / "scripts" / "flythrough.py")
    fly = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fly)
    return fly


def test_flythrough_aov_argument(tmp_path, capsys):
    """--aov DIR parses; with --no-render nothing is rendered or written; --aov
    without a folder is a usage error."""
    path0 = list(sys.path)
    try:
        fly = _flythrough()
        aov = tmp_path / "aov"
        rc = fly.main(["--maze", "4", "--frames", "3", "--width", "64", "--height", "48", "--aov", str(aov),
                       "--no-render"])
        assert rc == 0 and not aov.exists()
        assert len([ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("frame ")]) == 3
        with pytest.raises(SystemExit) as e:
            fly.main(["--maze", "4", "--frames", "3", "--no-render", "--aov"])
        assert e.value.code == 2
    finally:
        sys.path[:] = path0
