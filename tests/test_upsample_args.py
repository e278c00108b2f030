"""CPU test of the argument checks of mm_upsample_frames and mm_fill_pixels
(mirror-maze_amd/csrc/mm_filter_args.cpp: check_upsample, check_fill), pure functions of the arguments.
tests/upsample_args/upsample_args_test.cpp drives, per call, every rejection include/mm_api.h lists and asserts its
code and full message, which check wins when two fail, and the accepted neighbours (the optional buffers left out,
an output directly beside an input, an empty list).  Built twice, as tests/test_filter_args.py builds its program:
plain, and with the address and undefined-behaviour sanitizers (a stand-alone host program; no GPU, no library
loaded into Python).
"""
from __future__ import annotations

import subprocess
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parents[1]
CSRC = REPO / "mirror-maze_amd" / "csrc"
SRC = [Path(__file__).resolve().parent / "upsample_args" / "upsample_args_test.cpp", CSRC / "mm_filter_args.cpp"]
BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@pytest.fixture(scope="module", params=list(BUILDS))
def exe(request, tmp_path_factory):
    out = tmp_path_factory.mktemp("upsample_args") / f"upsample_args_{request.param}"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *BUILDS[request.param], f"-I{CSRC}",
                    f"-I{REPO / 'include'}", "-o", str(out), *map(str, SRC)], check=True)
    return out


@pytest.mark.parametrize("call", ["upsample", "fill"])
def test_checks(exe, call):
    """One call: codes, messages, precedence and accepted neighbours."""
    r = subprocess.run([str(exe), call], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stderr == "" and r.stdout.startswith("ok "), r.stdout + r.stderr
    assert int(r.stdout.split()[1]) >= 60  # (not vacuous)
