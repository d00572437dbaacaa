#!/usr/bin/env python3
"""What temporal reprojection (rt_hip_reproject) costs and what it buys.
Timing: config 4 (the 38-sphere room) at 1920x1080 and 3840x2160, 4 spp, under the last two cameras of the orbit; the one launch
timed by HIP events, best of `reps`, with and without the byte output.
--sweep: the quality table of DESIGN ("`pt_reproject`"): config 4 at 320x180, 4 spp per frame, the 8-frame orbit of
scene.orbit_cameras, against 1024 spp of the last camera and another seed, over a grid of max_history, depth_tol and normal_min:
the clipped linear RMS of the accumulated last frame and its ratio to the last 4-spp frame's own; then the defaults at 160x90, the
size tests/test_gpu_reproject.py runs.
usage: python tools/reproject_bench.py [--reps=R (5)] [--sweep]"""
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "raytracer.c_amd")]
import numpy as np
import torch
from rt_amd import gpu as G, scene as S

SEED = 1666943821
SPP, FRAMES = 4, 8
opt = {a.split("=")[0]: (a.split("=") + [""])[1] for a in sys.argv[1:] if a.startswith("--")}
reps = int(opt.get("--reps") or 5)


def frame(gs, cam, seed, spp=SPP):
    """the frame's linear mean and its first-hit buffers of the same seed and samples, on the device"""
    total = G.n_tiles(gs.scene.width, gs.scene.height)
    tiles, tiles8, _ = gs.render_tiles(seed, 0, 1, total, samples=spp, chunks=gs.suggest_chunks(total, spp), camera=cam)
    image, _ = gs.untile(tiles, tiles8, 0, 1, total)
    aov = gs.untile_aov(gs.render_aov(seed, spp, 0, 1, total, camera=cam, want=G.DENOISE_AOV), 0, 1, total)
    torch.cuda.synchronize()
    return image, aov


def timing():
    for w, h in ((1920, 1080), (3840, 2160)):
        sc = S.build_scene(4, w, h, SPP)
        gs = G.GpuScene(sc)
        cams = S.orbit_cameras(4, w, h)[-2:]
        prev, prev_aov = frame(gs, cams[0], SEED)
        cur, cur_aov = frame(gs, cams[1], SEED + 1)
        hist = dict(rgb=prev, len=torch.full((h, w), 3.0, device=prev.device), aov=prev_aov, camera=cams[0])
        out = {}
        for want8 in (True, False):
            best = None
            for k in range(reps + 1):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                a.record()
                out = G.reproject(cur, cur_aov, cams[1], hist=hist, out=dict(out) if want8 else dict(out, rgb8=None))
                b.record()
                torch.cuda.synchronize()
                if k:
                    best = a.elapsed_time(b) if best is None else min(best, a.elapsed_time(b))
            took = float((out["len"] > 1).float().mean())
            # a pixel reads 36 B of its own, up to 4 x 40 B of history (neighbouring lanes share them) and writes 24 B (+ 3 B)
            print(f"{w}x{h} {'with' if want8 else 'without'} bytes: {best:.3f} ms  ({w * h / best * 1e-6:.2f} Gpixel/s; history taken "
                  f"on {took:.3f} of the frame)", flush=True)
        gs.close()
        sc.free()


def clip(a):
    return np.clip(np.nan_to_num(np.asarray(a, np.float64), nan=1.0), 0, 1)


def rms(a, b):
    return float(np.sqrt(((clip(a) - clip(b)) ** 2).mean()))


def orbit(gs, frames, cams, **params):
    """the frames accumulated in order -> (the accumulated last frame, its mean history length)"""
    hist, res = None, None
    for (image, aov), cam in zip(frames, cams):
        res = G.reproject(image, aov, cam, hist=hist, out=dict(rgb8=None), **params)
        hist = dict(rgb=res["rgb"], len=res["len"], aov=aov, camera=cam)
    torch.cuda.synchronize()
    return res["rgb"].cpu().numpy(), float(res["len"].mean())


def sweep():
    for (w, h), grid in (((320, 180), True), ((160, 90), False)):
        sc = S.build_scene(4, w, h, SPP)
        gs = G.GpuScene(sc)
        cams = S.orbit_cameras(4, w, h, FRAMES)
        frames = [frame(gs, cam, SEED + k) for k, cam in enumerate(cams)]
        ref, _, _ = gs.render_image(SEED + 100, 1024)      # the orbit ends at the scene's own camera
        ref = ref.cpu().numpy()
        l0 = rms(frames[-1][0].cpu().numpy(), ref)
        print(f"{w}x{h}: the last frame alone, {SPP} spp: clipped linear RMS {l0:.4f}")
        if not grid:
            out, n = orbit(gs, frames, cams)
            print(f"{w}x{h}: the defaults: clipped linear RMS {rms(out, ref):.4f}, ratio {rms(out, ref) / l0:.3f}, mean length {n:.2f}")
        else:
            print(" max_history  depth_tol  normal_min | linear RMS  ratio  mean length")
            for mh, dt, nm in itertools.product((4.0, 8.0, 16.0, 32.0, 64.0), (0.01, 0.02, 0.05, 0.1, 0.2), (0.5, 0.8, 0.9, 0.95, 0.99)):
                if (dt != 0.05 and nm != 0.9) or (mh != 32.0 and (dt != 0.05 or nm != 0.9)):
                    continue   # max_history at the other two's middle; depth_tol and normal_min each along its own axis at max_history 32
                out, n = orbit(gs, frames, cams, max_history=mh, depth_tol=dt, normal_min=nm)
                print(f"{mh:12.0f} {dt:10.2f} {nm:11.2f} | {rms(out, ref):10.4f} {rms(out, ref) / l0:6.3f} {n:12.2f}", flush=True)
        gs.close()
        sc.free()


if __name__ == "__main__":
    sweep() if "--sweep" in opt else timing()
