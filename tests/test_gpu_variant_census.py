"""GPU side of the variant census (tests/variant_census_support.py): every row of the table uploads its scene
with its options, runs its entry point at the smallest shape that still exercises the variant -- 32 x 16 at 8
spp and 8 / 8 bounces, 64 x 32 (256 chunks: several waves park per block) where the tail rings are asked for,
two frames through the multi-frame entries, the window as a shuffled list with a duplicate and an entry outside
the view through the list entries -- and asserts zero differing bits against the oracle, the oracle's ray and
path counts where it counts, and that the launch ran the (LDS mode, internal form, ring kind) the row names."""
from __future__ import annotations

import numpy as np
import pytest

import variant_census_support as vc
from variant_census_support import CASES

pytestmark = pytest.mark.gpu


def _bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _gather(ref, x0, y0, px):
    """The list's expected entries from the window's reference: zeros for an entry outside the view."""
    out = np.zeros((len(px), 4), np.float32)
    inside = (px[:, 0] >= 0) & (px[:, 0] < vc.VIEW[0]) & (px[:, 1] >= 0) & (px[:, 1] < vc.VIEW[1])
    out[inside] = ref[px[inside, 1] - y0, px[inside, 0] - x0]
    return out, inside


def _pixel_rays(key, cam, frame, x, y):
    return vc.reference(key, cam, frame, int(x), int(y), 1, 1)[1]


@pytest.mark.parametrize("case", CASES, ids=vc.case_id)
def test_variant_bit_exact(gpu, case):
    from mirror_maze import (MM_INFO_LAST_DEFER, MM_INFO_LAST_FORM, MM_INFO_LAST_KERNEL_FORM, MM_INFO_LAST_LDS_MODE,
                             MM_INFO_LAST_RING, MM_INFO_LAST_STATIC_LDS, Renderer)

    key = case.scene
    x0, y0, w, h = win = vc.window(case)
    frames = vc.frames_of(case)
    refs = [vc.reference(key, cam, frame, *win) for cam, frame in frames]
    u, e = vc.uniform(key, 0), vc.ext()
    want_rays, want_paths = sum(r[1] for r in refs), sum(r[2] for r in refs)
    with Renderer(0) as r:
        for k, v in case.opts.items():
            r.set_option(k, v)
        r.upload_scene(vc.scene(key))
        if case.entry == "tile":
            got, st = r.trace_tile(u, e, *win, stats=case.stats)
            want = refs[0][0]
        elif case.entry == "frames":
            got, st = r.trace_tile_frames(u, e, vc.N_FRAMES, *win, stats=case.stats)
            want = np.stack([ref[0] for ref in refs])
        elif case.entry == "cameras":
            got, st = r.trace_tile_cameras(u, vc.cameras(key), e, *win, stats=case.stats)
            want = np.stack([ref[0] for ref in refs])
        else:
            lists = [vc.pixel_list(case, seed=f) for f in range(len(frames))]
            px = np.concatenate([p for p, _ in lists])
            parts = [_gather(ref[0], x0, y0, p) for ref, (p, _) in zip(refs, lists)]
            want = np.concatenate([g for g, _ in parts])
            # the duplicated pixel is traced twice; the entry outside the view traces nothing
            want_rays += sum(_pixel_rays(key, cam, frame, *p[dup]) for (cam, frame), (p, dup) in zip(frames, lists))
            want_paths = int(sum(inside.sum() for _, inside in parts)) * vc.SPP
            assert want_paths == (w * h + 1) * vc.SPP * len(frames)
            if case.entry == "pixels":
                got, st = r.trace_pixels(u, e, px, stats=case.stats)
            else:
                offsets = np.cumsum([0] + [len(p) for p, _ in lists])
                got, _, st = r.trace_pixel_lists(u, vc.cameras(key), e, px, offsets, stats=case.stats)
        r.sync()
        ran = (r.scene_info(MM_INFO_LAST_LDS_MODE), r.scene_info(MM_INFO_LAST_KERNEL_FORM),
               r.scene_info(MM_INFO_LAST_RING))
        defer, folded = r.scene_info(MM_INFO_LAST_DEFER), r.scene_info(MM_INFO_LAST_FORM)
        static_lds = r.scene_info(MM_INFO_LAST_STATIC_LDS)
    bad = int((_bits(got) != _bits(want)).sum())
    print(f"{vc.case_id(case)}: ran {ran} defer {defer} static LDS {static_lds} differing words {bad}"
          + (f" rays {st.rays} / {want_rays} paths {st.paths} / {want_paths}" if case.stats else ""))
    assert bad == 0, (vc.case_id(case), bad)
    if case.stats:
        assert (st.rays, st.paths) == (want_rays, want_paths)
    mode, form, ring = case.expect
    assert ran == (float(mode), float(form), float(ring)), (ran, case.expect)
    assert defer == (1.0 if ring != 0 else 0.0)
    assert folded == (11.0 if form >= 11 else float(form))
    if ring != 0 and mode not in vc.STATIC_GRID_MODES:  # what the table's ring kinds for dynamic LDS rest on
        assert static_lds == vc.STATIC_LDS[ring], (static_lds, ring)
