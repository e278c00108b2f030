"""CPU tests of mm_trace_pixel_lists' host side: the pure plan (mirror-maze_amd/csrc/mm_plan.cpp
plan_pixel_lists) through tests/pixel_lists/plan_pixel_lists_test.cpp, a stand-alone host program built plain and
with the address and undefined-behaviour sanitizers -- per-list chunk prefixes, the chunk-to-list search over
them, the queue and staging bounds at their edges, the offsets' refusals -- and select_noisy_frames against the
per-frame select_noisy on CPU tensors.
"""
from __future__ import annotations

import json
import subprocess
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parents[1]
CSRC = REPO / "mirror-maze_amd" / "csrc"
SRC = [Path(__file__).resolve().parent / "pixel_lists" / "plan_pixel_lists_test.cpp", CSRC / "mm_plan.cpp"]
BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}

MM_OK, MM_ERR_INVALID, MM_ERR_UNSUPPORTED = 0, -1, -6
MM_PIPE_WAVEFRONT, MM_PIPE_REFERENCE = 2, 3
TOO_MANY = "mm_trace_pixel_lists: more paths than one launch holds (2^32)"
# the most chunks a queue holds: 64 * chunks + 2^24 (what the waves' last claims may overshoot) <= 2^32 - 1
MAX_CHUNKS = (2**32 - 1 - 2**24) // 64


@pytest.fixture(scope="module", params=list(BUILDS))
def plan(request, tmp_path_factory):
    exe = tmp_path_factory.mktemp("plan_pixel_lists") / f"plan_pixel_lists_{request.param}"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *BUILDS[request.param], f"-I{CSRC}",
                    f"-I{REPO / 'include'}", "-o", str(exe), *map(str, SRC)], check=True)

    def run(offsets, **kw):
        kw["offsets"] = ",".join(str(int(o)) for o in offsets)
        r = subprocess.run([str(exe), *(f"{k}={v}" for k, v in kw.items())], capture_output=True, text=True,
                           timeout=60)
        assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
        return json.loads(r.stdout)

    return run


def _expected(lengths, spp):
    """(spans, owner): what the definition gives for lists of these lengths -- every list's paths padded to
    whole 64-path chunks, and for every chunk of the queue the list whose span holds it."""
    spans, owner, chunk, entry = [], [], 0, 0
    for f, n in enumerate(lengths):
        k = -(-n * spp // 64)
        spans.append([chunk, k, entry, n, n * spp])
        owner += [f] * k
        chunk += k
        entry += n
    return spans, owner


def _offsets(lengths):
    return [0, *np.cumsum(lengths).tolist()]


# 0 entries, 1 entry, exactly 64 paths (8 entries at 8 spp), 65 paths' worth (9 entries: 72 paths, two chunks);
# consecutive empty lists at the start, in the middle and at the end
CASES = {
    "edges": [0, 1, 8, 9, 0, 200],
    "empty-start": [0, 0, 0, 5, 8],
    "empty-middle": [3, 0, 0, 0, 17, 0, 1],
    "empty-end": [9, 1, 0, 0, 0],
    "empty-everywhere": [0, 0, 8, 0, 0, 9, 0, 0],
    "single": [37],
}


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("spp", [1, 3, 8, 64, 65])
def test_chunk_prefixes_and_the_search(plan, case, spp):
    lengths = CASES[case]
    r = plan(_offsets(lengths), spp=spp)
    spans, owner = _expected(lengths, spp)
    assert r["code"] == MM_OK and r["n_entries"] == sum(lengths) and r["n_chunks"] == len(owner)
    assert r["lists"] == spans
    # every chunk's list is a non-empty one whose span holds the chunk
    assert r["owner"] == owner
    assert r["fuse"] == (64 % spp == 0)


def test_exactly_64_and_65_paths(plan):
    """One chunk exactly full, and one path more: 64 paths -> 1 chunk, 65 -> 2 (at 1 spp, so paths = entries)."""
    r = plan(_offsets([64, 65, 1]), spp=1)
    assert [l[:2] for l in r["lists"]] == [[0, 1], [1, 2], [3, 1]] and r["owner"] == [0, 1, 1, 2]


def test_many_short_lists_search_depth(plan):
    """300 lists of 0..3 entries: the search lands on the right list at every depth."""
    lengths = np.random.default_rng(300).integers(0, 4, 300).tolist()
    r = plan(_offsets(lengths), spp=8)
    spans, owner = _expected(lengths, 8)
    assert r["lists"] == spans and r["owner"] == owner and 0 in lengths


def test_all_lists_empty_is_a_valid_plan(plan):
    r = plan([0, 0, 0])
    assert r["code"] == MM_OK and r["n_entries"] == 0 and r["n_chunks"] == 0 and r["owner"] == []


def test_fuse_or_stage_by_plan_pixels_rule(plan):
    off = _offsets([3, 4])
    assert plan(off, spp=8)["fuse"] == 1
    assert plan(off, spp=8, fuse=0)["fuse"] == 0
    assert plan(off, spp=24)["fuse"] == 0
    assert plan(off, spp=8, pipe=MM_PIPE_REFERENCE)["fuse"] == 0
    r = plan(off, pipe=MM_PIPE_WAVEFRONT)
    assert r["code"] == MM_ERR_UNSUPPORTED and "MM_PIPE_WAVEFRONT" in r["error"]


def test_queue_bound_at_its_edge(plan):
    """The queue counts PADDED lists.  At 64 spp an entry is a chunk: MAX_CHUNKS entries fit, one more does not.
    At 8 spp two one-entry lists ahead of a long one take a chunk each: the same entries that fit as one list
    are one chunk too many as three."""
    assert 64 * MAX_CHUNKS + 2**24 <= 2**32 - 1 < 64 * (MAX_CHUNKS + 1) + 2**24
    r = plan([0, 5, MAX_CHUNKS], spp=64)
    assert r["code"] == MM_OK and r["n_chunks"] == MAX_CHUNKS and r["lists"][1] == [5, MAX_CHUNKS - 5, 5,
                                                                                   MAX_CHUNKS - 5, 64 * (MAX_CHUNKS - 5)]
    r = plan([0, 5, MAX_CHUNKS + 1], spp=64)
    assert r["code"] == MM_ERR_INVALID and r["error"] == TOO_MANY
    n = 8 * (MAX_CHUNKS - 1)
    assert plan([0, n + 2], spp=8)["n_chunks"] == MAX_CHUNKS
    assert plan([0, 1, n + 1], spp=8)["n_chunks"] == MAX_CHUNKS
    r = plan([0, 1, 2, n + 2], spp=8)
    assert r["code"] == MM_ERR_INVALID and r["error"] == TOO_MANY
    # entries alone past 32 bits, and offsets whose products would wrap 64 bits
    for off in ([0, 2**32], [0, 1, 2**63], [0, 2**64 - 1]):
        r = plan(off, spp=4096)
        assert r["code"] == MM_ERR_INVALID and r["error"] == TOO_MANY


def test_staging_bound_at_its_edge(plan):
    """Staged samples: 2^29 paths in all lists together, not padded."""
    staged = ("mm_trace_pixel_lists: the lists' staged samples exceed 6 GiB (2^29 paths); use shorter lists")
    n3 = 2**29 // 3
    assert 3 * n3 <= 2**29 < 3 * (n3 + 1)
    assert plan([0, 100, n3], spp=3)["code"] == MM_OK
    r = plan([0, 100, n3 + 1], spp=3)
    assert r["code"] == MM_ERR_INVALID and r["error"] == staged
    assert plan([0, 2**26], spp=8, fuse=0)["code"] == MM_OK
    assert plan([0, 2**25, 2**26 + 1], spp=8, fuse=0)["code"] == MM_ERR_INVALID
    assert plan([0, 2**25, 2**26 + 1], spp=8)["code"] == MM_OK  # fused: nothing is staged
    assert plan([0, 2**26 + 1], spp=8, pipe=MM_PIPE_REFERENCE)["code"] == MM_ERR_INVALID


def test_offsets_refusals(plan):
    r = plan([1, 2, 3])
    assert r["code"] == MM_ERR_INVALID and r["error"] == "mm_trace_pixel_lists: offsets[0] is not 0"
    for off in ([0, 5, 4], [0, 0, 7, 6, 9], [0, 2**40, 1]):
        r = plan(off)
        assert r["code"] == MM_ERR_INVALID and r["error"] == "mm_trace_pixel_lists: offsets decrease", off
    r = plan([0, 1], null_offsets=1)
    assert r["code"] == MM_ERR_INVALID and r["error"] == "mm_trace_pixel_lists: null offsets"
    for n in (0, 65536):
        r = plan([0, 1], n_lists=n)
        assert r["code"] == MM_ERR_INVALID and r["error"] == "mm_trace_pixel_lists: n_lists outside 1..65535"
    r = plan([0], zeros=65536)  # 65535 lists, all empty
    assert r["code"] == MM_OK and len(r["lists"]) == 65535
    assert plan([0], zeros=65537)["code"] == MM_ERR_INVALID


# ---- select_noisy_frames -------------------------------------------------------------------------------------


def _frames(seed, n=4, h=13, w=17):
    rng = np.random.default_rng(seed)
    color = rng.uniform(0.0, 2.0, size=(n, h, w, 4)).astype(np.float32)
    var = (rng.uniform(0.0, 1.5, size=(n, h, w)) ** 2).astype(np.float32)
    count = rng.integers(2, 64, size=(n, h, w)).astype(np.float32)
    return color, var, count


def test_select_noisy_frames_is_the_per_frame_lists_back_to_back():
    import torch

    from mirror_maze import MM_AOV_ID_FAILED, MM_AOV_ID_MISS, select_noisy, select_noisy_frames

    color, var, count = (torch.from_numpy(a) for a in _frames(21))
    n, h, w = var.shape
    var[2] = 0.0  # a frame that selects nothing, in the middle
    ids = torch.full((n, h, w), 7 | 0x40000000, dtype=torch.int32)
    ids[0, 2, 3] = MM_AOV_ID_MISS - (1 << 32)
    ids[3, :, 5] = MM_AOV_ID_FAILED - (1 << 32)
    for cnt, kw in ((count, {}), (8.0, {}), (count, dict(ids=ids, x0=100, y0=40)), (count, dict(floor=0.5))):
        per_frame = [select_noisy(color[f], var[f], cnt[f] if torch.is_tensor(cnt) else cnt, 0.2,
                                  **{k: (v[f] if k == "ids" else v) for k, v in kw.items()}) for f in range(n)]
        pixels, offsets = select_noisy_frames(color, var, cnt, 0.2, **kw)
        assert pixels.dtype == torch.int32 and pixels.is_contiguous() and pixels.device.type == "cpu"
        assert torch.equal(pixels, torch.cat(per_frame))
        assert isinstance(offsets, np.ndarray) and offsets.dtype == np.uint64
        assert offsets.tolist() == [0, *np.cumsum([p.shape[0] for p in per_frame]).tolist()]
        assert offsets[2] == offsets[3] and 0 < offsets[1] < offsets[-1]
    none, off = select_noisy_frames(color, var, 8, float("inf"))
    assert tuple(none.shape) == (0, 2) and none.dtype == torch.int32 and off.tolist() == [0] * (n + 1)
    with pytest.raises(ValueError):
        select_noisy_frames(color[0], var[0], 8, 0.2)


def test_symbol_exists_and_rejects_a_null_context():
    from mirror_maze import Renderer, _lib

    L = _lib.lib()
    assert "mm_trace_pixel_lists" in _lib.EXPORTS
    assert L.mm_trace_pixel_lists(None, None, None, None, None, 1, None, None, None, None, None) == _lib.MM_ERR_INVALID
    for name in ("trace_pixel_lists", "refine_frames"):
        assert callable(getattr(Renderer, name))
