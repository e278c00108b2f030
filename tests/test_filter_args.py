"""CPU test of the frame filters' argument checks (mirror-maze_amd/csrc/mm_filter_args.cpp): the checks of
mm_denoise_frames, mm_accumulate_frames, mm_blend_pixels and their _var forms as pure functions of the arguments.
tests/filter_args/filter_args_test.cpp drives, per call, every rejection include/mm_api.h lists and asserts its
code and full message, which check wins when two fail, and the accepted neighbours (an output directly beside an
input, the optional buffers left out, an empty list).  Built twice: plain, and with the address and
undefined-behaviour sanitizers (a stand-alone host program; no GPU, no library loaded into Python).

The null-context tests of the six calls (test_denoise.py, test_denoise_var.py, test_temporal.py, ...) cannot tell
one rejection from another -- a null context returns MM_ERR_INVALID in the end whatever the checks do; this
program can, and a good argument set returning MM_OK from the check shows that the null context is refused after
the checks, not instead of them.
"""
from __future__ import annotations

import subprocess
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parents[1]
CSRC = REPO / "mirror-maze_amd" / "csrc"
SRC = [Path(__file__).resolve().parent / "filter_args" / "filter_args_test.cpp", CSRC / "mm_filter_args.cpp"]
BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@pytest.fixture(scope="module", params=list(BUILDS))
def exe(request, tmp_path_factory):
    out = tmp_path_factory.mktemp("filter_args") / f"filter_args_{request.param}"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *BUILDS[request.param], f"-I{CSRC}",
                    f"-I{REPO / 'include'}", "-o", str(out), *map(str, SRC)], check=True)
    return out


@pytest.mark.parametrize("pair", ["denoise", "accumulate", "blend"])
def test_checks(exe, pair):
    """Both calls of the pair: codes, messages, precedence and accepted neighbours."""
    r = subprocess.run([str(exe), pair], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stderr == "" and r.stdout.startswith("ok "), r.stdout + r.stderr
    assert int(r.stdout.split()[1]) >= 100  # (not vacuous)

