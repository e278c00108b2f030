"""CPU test of the trace and query calls' argument checks (mirror-maze_amd/csrc/mm_trace_args.cpp) and of the
staging rings' policy (mirror-maze_amd/csrc/mm_stage_ring.h ring_place), as pure functions.
tests/trace_args/trace_args_test.cpp drives, per family -- the tile calls, the list calls, mm_trace_aov and
mm_query_rays -- every rejection the code makes and asserts its code and full message, which check wins when two
fail, and the accepted neighbours; and the ring's sequences for both rings' parameters (from empty, filled exactly,
doubling, the wrap, a request beyond a wrap-sized ring), against the two rings the policy replaced.  Built twice:
plain, and with the address and undefined-behaviour sanitizers (a stand-alone host program; no GPU, no library
loaded into Python).

The GPU tests of these calls assert return codes and substrings of messages, and reach the checks only with a
device; this program needs none and pins the whole text and the precedence.
"""
from __future__ import annotations

import subprocess
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parents[1]
CSRC = REPO / "mirror-maze_amd" / "csrc"
SRC = [Path(__file__).resolve().parent / "trace_args" / "trace_args_test.cpp", CSRC / "mm_trace_args.cpp",
       CSRC / "mm_filter_args.cpp", CSRC / "mm_plan.cpp"]
BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@pytest.fixture(scope="module", params=list(BUILDS))
def exe(request, tmp_path_factory):
    out = tmp_path_factory.mktemp("trace_args") / f"trace_args_{request.param}"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *BUILDS[request.param], f"-I{CSRC}",
                    f"-I{REPO / 'include'}", "-o", str(out), *map(str, SRC)], check=True)
    return out


@pytest.mark.parametrize("families", ["tile", "lists", "aov query", "ring"])
def test_checks(exe, families):
    """The families' calls: codes, messages, precedence and accepted neighbours; the ring: its sequences."""
    r = subprocess.run([str(exe), *families.split()], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stderr == "" and r.stdout.startswith("ok "), r.stdout + r.stderr
    assert int(r.stdout.split()[1]) >= 100  # (not vacuous)
