"""CPU test of the per-call status bookkeeping (mirror-maze_amd/csrc/mm_calls.cpp, mm::CallTracker): the slot
ring, the calls that own its launches, the failed list and the ring-timeout record, as plain host logic over an
array of words.  tests/call_tracker/call_tracker_test.cpp runs a tracker of 4 slots that keeps 2 failed calls
and writes the status words itself, as the device would -- the cases the GPU suite reaches only by looping past
1024 slots or 64 failures (test_gpu_errors.py).  Built twice: plain, and with the address and undefined-behaviour
sanitizers (a stand-alone host program).
"""
from __future__ import annotations

import subprocess
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parents[1]
CSRC = REPO / "mirror-maze_amd" / "csrc"
SRC = [Path(__file__).resolve().parent / "call_tracker" / "call_tracker_test.cpp", CSRC / "mm_calls.cpp"]
CASES = ["clean_call", "failing_launch", "multi_launch_call", "occupant_not_done", "never_enqueued",
         "failed_list_overflow", "ring_record", "error_bits"]
BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@pytest.fixture(scope="module", params=list(BUILDS))
def driver(request, tmp_path_factory):
    exe = tmp_path_factory.mktemp("call_tracker") / f"call_tracker_{request.param}"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *BUILDS[request.param], f"-I{CSRC}",
                    f"-I{REPO / 'include'}", "-o", str(exe), *map(str, SRC)], check=True)
    return exe


def test_cases_listed(driver):
    r = subprocess.run([str(driver), "--list"], capture_output=True, text=True, timeout=60)
    assert r.stdout.split() == CASES


@pytest.mark.parametrize("case", CASES)
def test_call_tracker(driver, case):
    r = subprocess.run([str(driver), case], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout == f"ok {case}\n" and r.stderr == "", r.stdout + r.stderr
