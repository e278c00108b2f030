"""CPU test of mm_trace_rays' argument checks (mirror-maze_amd/csrc/mm_trace_args.cpp check_trace_rays) and plan
(mm_plan.cpp plan_rays) as pure functions, in the manner of tests/test_trace_args.py.
tests/rays_args/rays_args_test.cpp drives every MM_ERR_INVALID condition include/mm_api.h states for the call, with
its full message and its place in the order; the 2^32 queue and 2^29 staging bounds at the boundary value and one
past it; the fuse / stage choice at spp 8, 3, 24 and 64 with and without a variance buffer; and the refusal of
MM_PIPE_WAVEFRONT.  A stand-alone host program: no GPU, no library loaded into Python.
"""
from __future__ import annotations

import subprocess
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parents[1]
CSRC = REPO / "mirror-maze_amd" / "csrc"
SRC = [Path(__file__).resolve().parent / "rays_args" / "rays_args_test.cpp", CSRC / "mm_trace_args.cpp",
       CSRC / "mm_filter_args.cpp", CSRC / "mm_plan.cpp"]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("rays_args") / "rays_args_test"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O2", f"-I{CSRC}", f"-I{REPO / 'include'}", "-o", str(out),
                    *map(str, SRC)], check=True)
    return out


def test_checks_and_plan(exe):
    """Codes, full messages, precedence, the bounds' two sides and the plan's choices."""
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stderr == "" and r.stdout.startswith("ok "), r.stdout + r.stderr
    assert int(r.stdout.split()[1]) >= 100  # (not vacuous)
