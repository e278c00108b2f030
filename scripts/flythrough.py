#!/usr/bin/env python
"""A scripted fly-through of the maze, rendered as a moving-camera sequence.

Builds an N x N maze, walks a Player along a key script (forward, with a mouse
turn every --turn-every frames; the reference's event loop, src/main.rs:738-842)
and renders the frames --batch per launch as RGBA8 through
Renderer.trace_tile_cameras (mm_trace_tile_cameras: one camera per frame, one
launch per batch), written as PNGs.

    python scripts/flythrough.py --maze 32 --frames 40 --batch 20 --out flythrough/
    python scripts/flythrough.py --maze 10 --frames 30 --no-render     # the camera path only: no GPU
    python scripts/flythrough.py --maze 32 --frames 40 --aov aov/       # + feature buffers per frame
    python scripts/flythrough.py --maze 32 --frames 40 --denoise        # + frame_NNNN_dn.png beside each frame
    python scripts/flythrough.py --maze 32 --frames 40 --denoise-var    # + frame_NNNN_dnv.png: the variance-guided filter
    python scripts/flythrough.py --maze 32 --frames 40 --accumulate     # + frame_NNNN_acc.png beside each frame
    python scripts/flythrough.py --maze 32 --frames 40 --accumulate --top-up 2:24   # + extra samples where the history is short
    python scripts/flythrough.py --maze 32 --frames 40 --accumulate-var --denoise-var   # + frame_NNNN_accv.png, and the variance-guided filter on it
    python scripts/flythrough.py --maze 32 --frames 40 --upsample 2 --denoise          # trace every 2nd pixel, rebuild from the AOVs: frame_NNNN_up.png
    python scripts/flythrough.py --maze 32 --frames 40 --panorama 2048 --map 1024       # + frame_NNNN_pano.png per frame, one map.png

--aov DIR also writes, per frame, DIR/frame_NNNN/normal.png (the outward normal of
what the pixel sees through the mirrors, as 0.5 n + 0.5), depth.npy (float32
distance along the mirror chain, 1e30 where nothing is hit) and id.npy (uint32
rect index | kind << 30) through Renderer.trace_aov (mm_trace_aov, --mirrors as
its mirror limit): the inputs a denoiser or a compositor takes beside the frame.

--denoise also writes frame_NNNN_dn.png beside each frame: the frame through
Renderer.denoise (mm_denoise_frames, its default passes and sigmas), guided by
the batch's feature buffers -- traced for it if --aov did not ask for them.  The
batch is then traced as float frames; frame_NNNN.png is their RGBA8 conversion,
the same bytes as without --denoise.

--accumulate also writes frame_NNNN_acc.png beside each frame: the frame through
Renderer.accumulate (mm_accumulate_frames, its defaults), the running mean of
the frames before it wherever they showed the same surface point through the
same mirrors; the history carries over from batch to batch.  With --denoise the
denoiser then runs on the accumulated frames (frame_NNNN_dn.png).

--top-up N[:SPP] (with --accumulate) tops every accumulated frame up to a history
of N frames: the pixels whose history length is below N -- disoccluded by a turn
or a step past a wall edge -- get SPP more samples each (default 3 x --spp)
through Renderer.top_up (mm_trace_pixels + mm_blend_pixels), drawn with RNG frame
2^20 + f.  The batch is then accumulated frame by frame, each frame's history
being the topped-up frame before it, so the extra samples stay in the history;
the share of pixels topped up is printed per frame.

--refine TOL[:SPP[:ROUNDS]] also writes frame_NNNN_ref.png beside each frame: the
frame after up to ROUNDS (default 2) rounds of Renderer.refine_frames, each
giving the pixels whose mean's standard error is above TOL times their luminance
SPP more samples (default 3 x --spp), drawn with RNG frame 2^20 + 64 f + round:
one selection, one mm_trace_pixel_lists launch and one merge per round for the
whole batch (the files are those of Renderer.refine frame by frame).  The batch
is then traced with its per-pixel sample variance through Renderer.trace_tile_var
(mm_trace_tile_var), in one launch where --accumulate-var's rule below allows
it, else frame by frame; the share of pixels each round took is printed per frame.  With
--denoise the denoiser runs on the refined frames.  Not with --accumulate: a
history of frames with unequal sample counts is not what mm_accumulate_frames
averages.

--denoise-var also writes frame_NNNN_dnv.png beside each frame: the frame through
Renderer.denoise_var (mm_denoise_frames_var, its defaults), whose luminance stop
follows each pixel's own noise.  The frames are then traced through
Renderer.trace_tile_var (one by one, unless --refine or --accumulate-var trace
the batch in one launch), and with --refine the filter runs on
the refined frames with the variance and the sample counts the rounds left.  Not
with --accumulate: mm_accumulate_frames carries no variance through the history
(--accumulate-var does).

--accumulate-var, a mode of its own (not with --accumulate), also writes
frame_NNNN_accv.png beside each frame: the frame through Renderer.accumulate_var
(mm_accumulate_frames_var, its defaults), the accumulation of --accumulate with
the variance of every accumulated pixel carried beside it.  The batch is traced
with its per-pixel sample variance, in one Renderer.trace_tile_var launch where
a multi-frame variance launch runs (2^24 .. 2^29 paths: tail deferral on, the
staged paths of a launch), else frame by frame.
It composes with --denoise (the denoiser runs on the accumulated frames), with
--denoise-var (the filter takes the accumulated variance, count 1, at sigma_l 2:
the sweep of profiles/temporal_var/quality.txt), with
--top-up N[:SPP] (through Renderer.top_up_var: mm_trace_pixels_var +
mm_blend_pixels_var, SPP at least 2, RNG frame 2^21 + f) and with --refine (every
frame is refined first and enters with weight = count / --spp per pixel and
vmean = var / count).

--upsample S[:W_MIN] (S = 2, 4 or 8; --width and --height multiples of S) traces
only the lattice of every S-th pixel -- the view (width / S, height / S) -- and
rebuilds the frames from the full-resolution feature buffers through
Renderer.trace_upsampled (mm_upsample_frames; the pixels no lattice neighbour can
stand in for are traced in one mm_trace_pixel_lists launch per batch and filled
by mm_fill_pixels).  It writes frame_NNNN_up.png instead of frame_NNNN.png and
prints the share of holes per frame.  It composes with --denoise, with
--denoise-var (the rebuilt frame's variance, count 1) and with --accumulate-var
(the rebuilt pixels' effective sample weight and variance are passed on); with
either of the last two the lattice is traced with its variance -- in one launch
where a multi-frame variance launch runs, else frame by frame.
Not with --accumulate, --refine or --top-up.

--panorama W also writes frame_NNNN_pano.png (W x W/2) beside each frame: the
360-degree equirectangular view from the frame's camera, its centre looking
where the frame looks, through Renderer.trace_rays (mm_trace_rays) over
mirror_maze.equirect_rays, with RNG frame f and --spp / --bounces / --mirrors.

--map W writes one map.png (W x W): the maze from above, orthographic
(mirror_maze.ortho_rays), the walk's camera positions marked in red.  The rays
point from the ceiling to the floor and start 5 % of the room's height BELOW
the ceiling rect: started above it they would show the ceiling and nothing
else, and the corridors are what the map is for.

The camera path is printed one frame per line (floats as %.9g, which a float32
survives): frame, center, quat -- the camera after that frame's step.
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "mirror-maze_amd"))
sys.path.insert(0, str(REPO))

ACCV_SIGMA_L = 2.0  # --accumulate-var --denoise-var: the filter's sigma_l on the accumulated variance

def key_script(n_frames: int, turn_every: int, turn_dx: float):
    """(keys, mouse_dx) per frame: W held down, a mouse move of turn_dx on every
    turn_every-th frame (walls stop the player; the turns get it moving again)."""
    from mirror_maze import Player

    return [([Player.KEY_W], [turn_dx] if turn_every and f % turn_every == turn_every - 1 else [])
            for f in range(n_frames)]


def top_down_map(r, scene, cams, width, ext):
    """The (width, width, 4) uint8 map of --map: the scene's footprint in x and z seen from above through
    Renderer.trace_rays, the cameras' positions in red.  +y is down (a camera's image-down axis): of the
    horizontal rects the ceiling is the one with the least y, the floor the one with the greatest (the walls reach
    above the ceiling), and the rays start 5 % of the room's height below the ceiling."""
    import numpy as np

    from mirror_maze import ortho_rays

    rects = scene.rects
    corners = np.concatenate([rects[:, 0:3], rects[:, 0:3] + rects[:, 3:6], rects[:, 0:3] + rects[:, 6:9],
                              rects[:, 0:3] + rects[:, 3:6] + rects[:, 6:9]])
    lo, hi = corners.min(axis=0), corners.max(axis=0)
    side = float(max(hi[0] - lo[0], hi[2] - lo[2]))
    level = rects[np.cross(rects[:, 3:6], rects[:, 6:9])[:, 1] != 0.0, 1]  # the horizontal rects' heights
    ceiling, floor = (float(level.min()), float(level.max())) if len(level) else (float(lo[1]), float(hi[1]))
    y = ceiling + 0.05 * (floor - ceiling)
    rays = ortho_rays([lo[0], y, lo[2]], [side, 0.0, 0.0], [0.0, 0.0, side], [0.0, 1.0, 0.0], width, width)
    img, _ = r.trace_rays(ext, rays, rgba8=True)
    img = img.view(width, width, 4).cpu().numpy().copy()
    for c in cams:
        i, j = int((c[0] - lo[0]) / side * width), int((c[2] - lo[2]) / side * width)
        img[max(0, j - 1):j + 2, max(0, i - 1):i + 2] = (255, 0, 0, 255)
    return img


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--maze", type=int, default=32, help="maze size N (N x N cells)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--batch", type=int, default=20, help="frames per trace_tile_cameras launch")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--mirrors", type=int, default=8)
    ap.add_argument("--turn-every", type=int, default=8, help="a mouse turn every that many frames (0: never)")
    ap.add_argument("--turn-dx", type=float, default=40.0, help="the turn's mouse deltaX")
    ap.add_argument("--out", default="flythrough", help="folder for frame_NNNN.png")
    ap.add_argument("--aov", metavar="DIR", default=None,
                    help="also write per-frame feature buffers: DIR/frame_NNNN/{normal.png,depth.npy,id.npy}")
    ap.add_argument("--denoise", action="store_true",
                    help="also write frame_NNNN_dn.png: the frame through Renderer.denoise, guided by its feature buffers")
    ap.add_argument("--denoise-var", action="store_true",
                    help="also write frame_NNNN_dnv.png: the frame through Renderer.denoise_var, its luminance stop "
                         "scaled by each pixel's sample variance (composes with --refine, not with --accumulate)")
    ap.add_argument("--accumulate", action="store_true",
                    help="also write frame_NNNN_acc.png: the frame through Renderer.accumulate (temporal accumulation); "
                         "with --denoise the denoiser runs on the accumulated frames")
    ap.add_argument("--accumulate-var", action="store_true",
                    help="also write frame_NNNN_accv.png: the frame through Renderer.accumulate_var (temporal "
                         "accumulation that carries each pixel's variance); composes with --denoise, --denoise-var, "
                         "--top-up and --refine, not with --accumulate")
    ap.add_argument("--top-up", metavar="N[:SPP]", default=None,
                    help="with --accumulate or --accumulate-var: give the pixels whose history is shorter than N frames SPP more samples "
                         "(default 3 x --spp) and blend them into the accumulated frame")
    ap.add_argument("--refine", metavar="TOL[:SPP[:ROUNDS]]", default=None,
                    help="also write frame_NNNN_ref.png: up to ROUNDS (default 2) rounds of SPP more samples (default "
                         "3 x --spp) for the pixels whose standard error is above TOL times their luminance")
    ap.add_argument("--upsample", metavar="S[:W_MIN]", default=None,
                    help="trace the lattice of every S-th pixel (S = 2, 4 or 8) and rebuild the frames from the feature "
                         "buffers (Renderer.trace_upsampled): writes frame_NNNN_up.png; composes with --denoise, "
                         "--denoise-var and --accumulate-var")
    ap.add_argument("--panorama", metavar="W", type=int, default=0,
                    help="also write frame_NNNN_pano.png: a W x W/2 equirectangular panorama from each frame's camera "
                         "(Renderer.trace_rays)")
    ap.add_argument("--map", metavar="W", type=int, default=0,
                    help="also write map.png: a W x W orthographic view of the maze from above with the walk marked; "
                         "the rays start 5 %% of the room's height below the ceiling (from above it the map would "
                         "show the ceiling rect) and point at the floor")
    ap.add_argument("--no-render", action="store_true", help="print the camera path only (needs no GPU)")
    a = ap.parse_args(argv)
    if a.frames < 1 or a.batch < 1:
        ap.error("--frames and --batch must be positive")
    if a.panorama < 0 or a.panorama % 2 or a.map < 0:
        ap.error("--panorama takes an even width, --map a width")
    if a.accumulate and a.accumulate_var:
        ap.error("--accumulate-var is a mode of its own: not with --accumulate")
    if a.denoise_var and a.accumulate:
        ap.error("--denoise-var does not go with --accumulate: no variance is carried through the accumulated history "
                 "(--accumulate-var carries it)")
    if (a.denoise_var or a.accumulate_var) and a.spp < 2:
        ap.error("--denoise-var and --accumulate-var need --spp of at least 2 (a sample variance)")
    top_up = None  # (n_min, extra spp)
    if a.top_up is not None:
        if not (a.accumulate or a.accumulate_var):
            ap.error("--top-up needs --accumulate or --accumulate-var")
        try:
            n_min, _, extra = a.top_up.partition(":")
            top_up = (float(n_min), int(extra) if extra else 3 * a.spp)
        except ValueError:
            ap.error("--top-up takes N[:SPP]")
        if not (top_up[0] > 1.0 and 1 <= top_up[1] <= 4096):
            ap.error("--top-up: N must be above 1 and SPP in 1..4096")
        if a.accumulate_var and top_up[1] < 2:
            ap.error("--top-up with --accumulate-var: SPP must be at least 2 (a sample variance)")
    refine = None  # (rel_tol, extra spp, rounds)
    if a.refine is not None:
        if a.accumulate:
            ap.error("--refine does not go with --accumulate (it goes with --accumulate-var)")
        try:
            parts = a.refine.split(":")
            if not 1 <= len(parts) <= 3:
                raise ValueError
            refine = (float(parts[0]), int(parts[1]) if len(parts) > 1 and parts[1] else 3 * a.spp,
                      int(parts[2]) if len(parts) > 2 else 2)
        except ValueError:
            ap.error("--refine takes TOL[:SPP[:ROUNDS]]")
        if not (refine[0] > 0.0 and 2 <= refine[1] <= 4096 and 1 <= refine[2] <= 64 and a.spp >= 2):
            ap.error("--refine: TOL must be positive, SPP in 2..4096, ROUNDS in 1..64, and --spp at least 2")

    upsample = None  # (scale, w_min)
    if a.upsample is not None:
        if a.accumulate or a.refine is not None or a.top_up is not None:
            ap.error("--upsample does not go with --accumulate, --refine or --top-up")
        try:
            scale, _, w_min = a.upsample.partition(":")
            upsample = (int(scale), float(w_min) if w_min else 0.25)
        except ValueError:
            ap.error("--upsample takes S[:W_MIN]")
        if upsample[0] not in (2, 4, 8) or not 0.0 < upsample[1] <= 1.0:
            ap.error("--upsample: S must be 2, 4 or 8 and W_MIN in (0, 1]")
        if a.width % upsample[0] or a.height % upsample[0]:
            ap.error("--upsample: --width and --height must be multiples of S")

    from mirror_maze import Player, Scene, walk_cameras

    scene = Scene.build(a.maze, a.seed)
    player = Player(scene, a.width, a.height)
    script = key_script(a.frames, a.turn_every, a.turn_dx)
    cams = walk_cameras(player, script)
    for f, c in enumerate(cams):
        print(f"frame {f} center {c[0]:.9g} {c[1]:.9g} {c[2]:.9g} quat {c[4]:.9g} {c[5]:.9g} {c[6]:.9g} {c[7]:.9g}")
    if a.no_render:
        return 0

    import numpy as np
    import torch

    from mirror_maze import MMError, Renderer, make_ext, mm_camera, mm_uniform
    from mirror_maze.io import quantize, write_png

    out_dir = Path(a.out)
    out_dir.mkdir(parents=True, exist_ok=True)
    u = player.uniform()  # view size and chunk width; its camera is not used
    with_var = refine is not None or a.denoise_var or a.accumulate_var  # the frames are traced with their per-pixel sample variance
    floats = a.denoise or a.accumulate or with_var or upsample is not None  # the batch is traced as float frames
    prev = None  # --accumulate: the last accumulated frame, its feature buffers and its camera (-var: and its variance)
    with Renderer(0) as r:
        r.upload_scene(scene)
        if a.map:
            write_png(out_dir / "map.png", top_down_map(r, scene, cams, a.map, make_ext(a.spp, a.bounces, a.mirrors)))
            print(f"# map: {out_dir}/map.png", flush=True)
        for f0 in range(0, a.frames, a.batch):
            batch = cams[f0:f0 + a.batch]
            e = make_ext(a.spp, a.bounces, a.mirrors, frame=f0)
            if a.panorama:
                from mirror_maze import equirect_rays

                for k in range(len(batch)):
                    rays = equirect_rays(batch[k][0:3], batch[k][4:8], a.panorama, a.panorama // 2)
                    pano, _ = r.trace_rays(make_ext(a.spp, a.bounces, a.mirrors, frame=f0 + k), rays, rgba8=True)
                    write_png(out_dir / f"frame_{f0 + k:04d}_pano.png",
                              pano.view(a.panorama // 2, a.panorama, 4).cpu().numpy())
                print(f"# frames {f0}..{f0 + len(batch) - 1}: panoramas, {out_dir}/frame_{f0:04d}_pano.png ...", flush=True)
            # one launch for the batch where a multi-frame variance call runs: at most the 2^29 paths a launch
            # stages, and the tail deferral such a launch needs (from MM_OPT_DEFER_MIN's 2^24 paths on, where the
            # plan has it; the call refuses the launch otherwise, before anything is enqueued)
            paths = len(batch) * a.width * a.height * a.spp
            one_var_launch = ((a.accumulate_var or refine is not None) and len(batch) > 1 and 2**24 <= paths <= 2**29
                              and not upsample)
            if one_var_launch:
                try:
                    img, var, _ = r.trace_tile_var(u, e, 0, 0, a.width, a.height, cameras=batch)
                    count = torch.full_like(var, float(a.spp))
                except MMError:
                    one_var_launch = False
            up_bufs = up_weight = None
            if upsample:
                # the lattice, the feature buffers, the rebuilt frames and their filled holes: one launch per stage for
                # the batch (with a variance the lattice frame by frame where a multi-frame variance launch does not run)
                img, up_bufs, up_weight, var, share = r.trace_upsampled(u, batch, e, upsample[0], 0, 0, a.width,
                                                                        a.height, w_min=upsample[1], var=with_var)
                count = 1.0  # var is already the variance of the rebuilt pixel's mean
                for k in range(len(batch)):
                    print(f"# frame {f0 + k}: upsampled x{upsample[0]}, holes {100.0 * share[k]:.2f} % "
                          f"(traced at full resolution and filled)", flush=True)
            elif one_var_launch:
                pass
            elif with_var:
                # frame by frame (a single-frame variance call runs at any size; frame k is the batch launch's)
                img = torch.empty((len(batch), a.height, a.width, 4), dtype=torch.float32, device="cuda:0")
                var = torch.empty((len(batch), a.height, a.width), dtype=torch.float32, device="cuda:0")
                count = torch.full_like(var, float(a.spp))  # the samples each pixel holds
                for k in range(len(batch)):
                    uk = mm_uniform.from_buffer_copy(u)
                    uk.cam = mm_camera.from_buffer_copy(np.ascontiguousarray(batch[k], dtype=np.float32).tobytes())
                    r.trace_tile_var(uk, make_ext(a.spp, a.bounces, a.mirrors, frame=f0 + k), 0, 0, a.width, a.height,
                                     out=img[k], var=var[k])
            else:
                img, _ = r.trace_tile_cameras(u, batch, e, 0, 0, a.width, a.height, rgba8=not floats)
            frames = (r.quantize(img) if floats else img).cpu().numpy()
            r.sync()
            tag = "_up" if upsample else ""
            for k in range(len(batch)):
                write_png(out_dir / f"frame_{f0 + k:04d}{tag}.png", frames[k])
            print(f"# frames {f0}..{f0 + len(batch) - 1}: {'one launch each' if with_var and not one_var_launch else 'one launch'}, "
                  f"{out_dir}/frame_{f0:04d}{tag}.png ...", flush=True)
            if refine:
                # the whole batch per round: one selection, one list launch (mm_trace_pixel_lists), one merge.  A
                # frame that selects nothing in a round selects nothing in the later ones either: its rounds end
                shares = [[] for _ in batch]
                for rnd in range(refine[2]):
                    n_sel = r.refine_frames(u, batch, e, img, var, count, refine[0], refine[1],
                                            [2**20 + 64 * (f0 + k) + rnd for k in range(len(batch))])
                    for k in range(len(batch)):
                        if not (shares[k] and shares[k][-1] == 0):
                            shares[k].append(n_sel[k])
                    if not any(n_sel):
                        break
                for k in range(len(batch)):
                    shares[k] = [f"{100.0 * n / (a.width * a.height):.2f} %" for n in shares[k]]
                    print(f"# frame {f0 + k}: refined with {refine[1]} spp per round, pixels per round: "
                          f"{', '.join(shares[k])}", flush=True)
                done = r.quantize(img).cpu().numpy()
                r.sync()
                for k in range(len(batch)):
                    write_png(out_dir / f"frame_{f0 + k:04d}_ref.png", done[k])
            if a.aov is None and not (a.denoise or a.denoise_var or a.accumulate or a.accumulate_var):
                continue
            bufs = up_bufs or r.trace_aov(u, batch, a.mirrors, x0=0, y0=0, w=a.width, h=a.height,
                                          want=Renderer.AOV_NAMES if floats else ("normal_depth", "id"))
            if a.accumulate and top_up:
                # frame by frame: the history of frame k is the topped-up frame k - 1
                acc_img = torch.empty_like(img)
                for k in range(len(batch)):
                    gk = {name: v[k:k + 1] for name, v in bufs.items()}
                    r.accumulate(u, batch[k:k + 1], img[k:k + 1], gk, prev=prev, out=acc_img[k:k + 1])
                    _, n_sel = r.top_up(u, batch[k], e, acc_img[k], gk, top_up[0], top_up[1], 2**20 + f0 + k)
                    print(f"# frame {f0 + k}: topped up {n_sel} pixels ({100.0 * n_sel / (a.width * a.height):.2f} %) "
                          f"with {top_up[1]} spp", flush=True)
                    prev = (acc_img[k], gk, batch[k])
                img = acc_img
            elif a.accumulate:
                img = r.accumulate(u, batch, img, bufs, prev=prev)
                prev = (img[-1], {k: v[-1:] for k, v in bufs.items()}, batch[-1])
            if a.accumulate_var:
                vmean = (var / count).contiguous()  # the variance of each frame's pixel mean
                weight = (count / float(a.spp)).contiguous() if refine else None  # refined pixels hold more samples
                if upsample:
                    weight = up_weight  # a rebuilt pixel's effective sample weight, 1 where it was traced
                if top_up:
                    # frame by frame: the history of frame k is the topped-up frame k - 1
                    acc_img, acc_var = torch.empty_like(img), torch.empty_like(var)
                    for k in range(len(batch)):
                        gk = {name: v[k:k + 1] for name, v in bufs.items()}
                        r.accumulate_var(u, batch[k:k + 1], img[k:k + 1], gk, vmean[k:k + 1],
                                         None if weight is None else weight[k:k + 1], prev=prev, out=acc_img[k:k + 1],
                                         var_out=acc_var[k:k + 1])
                        _, _, n_sel = r.top_up_var(u, batch[k], e, acc_img[k], acc_var[k], gk, top_up[1],
                                                   2**21 + f0 + k, n_min=top_up[0])
                        print(f"# frame {f0 + k}: topped up {n_sel} pixels "
                              f"({100.0 * n_sel / (a.width * a.height):.2f} %) with {top_up[1]} spp", flush=True)
                        prev = (acc_img[k], gk, batch[k], acc_var[k])
                    img = acc_img
                else:
                    img, acc_var = r.accumulate_var(u, batch, img, bufs, vmean, weight, prev=prev)
                    prev = (img[-1], {k: v[-1:] for k, v in bufs.items()}, batch[-1], acc_var[-1])
                var, count = acc_var, 1.0  # what --denoise-var filters with: already the variance of the mean
            if a.accumulate or a.accumulate_var:
                tag = "accv" if a.accumulate_var else "acc"
                acc = r.quantize(img).cpu().numpy()
                r.sync()
                for k in range(len(batch)):
                    write_png(out_dir / f"frame_{f0 + k:04d}_{tag}.png", acc[k])
                print(f"# frames {f0}..{f0 + len(batch) - 1}: accumulated, {out_dir}/frame_{f0:04d}_{tag}.png ...",
                      flush=True)
            if a.denoise:
                clean = r.denoise(img, bufs, rgba8=True).cpu().numpy()
                r.sync()
                for k in range(len(batch)):
                    write_png(out_dir / f"frame_{f0 + k:04d}_dn.png", clean[k])
                print(f"# frames {f0}..{f0 + len(batch) - 1}: denoised, {out_dir}/frame_{f0:04d}_dn.png ...", flush=True)
            if a.denoise_var:
                # on an accumulated variance the narrow stop wins (profiles/temporal_var/quality.txt: sigma_l 2 has
                # the least geometric mean over the maze and the corridor, walk and turn); else the call's default
                kw = dict(sigma_l=ACCV_SIGMA_L) if a.accumulate_var else {}
                clean = r.denoise_var(img, bufs, var, count, rgba8=True, **kw).cpu().numpy()
                r.sync()
                for k in range(len(batch)):
                    write_png(out_dir / f"frame_{f0 + k:04d}_dnv.png", clean[k])
                print(f"# frames {f0}..{f0 + len(batch) - 1}: variance-guided denoise, "
                      f"{out_dir}/frame_{f0:04d}_dnv.png ...", flush=True)
            r.sync()
            if a.aov is None:
                continue
            nd = bufs["normal_depth"].cpu().numpy()
            ids = bufs["id"].cpu().numpy().view(np.uint32)
            for k in range(len(batch)):
                d = Path(a.aov) / f"frame_{f0 + k:04d}"
                d.mkdir(parents=True, exist_ok=True)
                rgba = np.concatenate([0.5 * nd[k, ..., :3] + 0.5, np.ones_like(nd[k, ..., :1])], axis=-1)
                write_png(d / "normal.png", quantize(rgba))
                np.save(d / "depth.npy", nd[k, ..., 3])
                np.save(d / "id.npy", ids[k])
            print(f"# frames {f0}..{f0 + len(batch) - 1}: feature buffers, one launch, {a.aov}/frame_{f0:04d}/ ...",
                  flush=True)
    torch.cuda.synchronize()
    return 0


if __name__ == "__main__":
    sys.exit(main())
