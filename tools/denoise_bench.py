#!/usr/bin/env python3
"""What the denoiser (rt_hip_denoise) costs and what it buys.
Timing: config 4 (the 38-sphere room) at 1920x1080 and 3840x2160, 16 spp, its first-hit buffers of the same samples; the whole
denoise (prepare + L filter launches) timed by HIP events, best of `reps`, next to the bytes and fp64 operations a pixel needs.
--sweep: the quality table of DESIGN ("Denoiser"): config 4 at 320x180, 16 spp, against 1024 spp of another seed, over a grid of
parameters: RMS of the tonemapped bytes and of the linear values clipped to [0, 1].
usage: python tools/denoise_bench.py [--iterations=L (5)] [--reps=R (5)] [--sweep]"""
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "raytracer.c_amd")]
import numpy as np
import torch
from rt_amd import gpu as G, scene as S

SEED = 1666943821
opt = {a.split("=")[0]: (a.split("=") + [""])[1] for a in sys.argv[1:] if a.startswith("--")}
L = int(opt.get("--iterations") or 5)
reps = int(opt.get("--reps") or 5)


def per_pixel(iterations, k=3, demodulate=True):
    """(DRAM bytes, fp64 operations) per pixel of a whole denoise: the prepare pass reads colour, albedo, normal, depth, hits and
    writes the signal (16 B), the guidance (16 B) and hits + object (8 B); a filter pass reads a pixel's 40 B once from DRAM (its 24
    neighbours' loads hit in cache) and writes 16 B; the last one writes 12 + 3 B and reads the albedo again.  A tap: the normal
    dot (5), its clamp (1), k squarings, D, Zn, dz, Zd (5), the colour distance (8), the weight (6, one division), the sums (7)."""
    alb = 12 if demodulate else 0
    prep = 12 + alb + 12 + 4 + 4 + 40
    filt = iterations * (40 + 16) + (alb + 15 - 16 if iterations else 0)
    ops = iterations * 24 * (32 + k)
    return prep + filt, ops


def frame(w, h, spp, seed=SEED):
    sc = S.build_scene(4, w, h, spp)
    gs = G.GpuScene(sc)
    image, image8, _ = gs.render_image(seed, spp)
    total = G.n_tiles(w, h)
    aov = gs.untile_aov(gs.render_aov(seed, spp, 0, 1, total, want=G.DENOISE_AOV), 0, 1, total)
    torch.cuda.synchronize()
    return sc, gs, image, image8, aov


def timing():
    for w, h in ((1920, 1080), (3840, 2160)):
        sc, gs, image, _, aov = frame(w, h, 16)
        out = torch.empty_like(image)
        best = None
        for k in range(reps + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            G.denoise(image, aov, w, h, out=out, iterations=L)
            b.record()
            torch.cuda.synchronize()
            if k:
                best = a.elapsed_time(b) if best is None else min(best, a.elapsed_time(b))
        nbytes, ops = per_pixel(L)
        px = w * h
        print(f"{w}x{h} L={L}: {best:.3f} ms  ({nbytes} B/pixel -> {nbytes * px / best * 1e-6:.0f} GB/s;  {ops} fp64 op/pixel -> "
              f"{ops * px / best * 1e-9:.2f} TFLOP/s fp64, {ops * px / best * 1e-9 / 39.3 * 100:.1f} % of 39.3)", flush=True)
        gs.close()
        sc.free()


def rms(a, b):
    return float(np.sqrt(((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2).mean()))


def clip(a):
    return np.clip(np.nan_to_num(np.asarray(a, np.float64), nan=1.0), 0, 1)


def sweep():
    w, h = 320, 180
    sc, gs, image, image8, aov = frame(w, h, 16)
    ref, ref8, _ = gs.render_image(SEED + 1, 1024)
    ref, ref8 = ref.cpu().numpy(), ref8.cpu().numpy()
    b0, l0 = rms(image8.cpu().numpy(), ref8), rms(clip(image.cpu().numpy()), clip(ref))
    print(f"noisy 16 spp: bytes RMS {b0:.2f} LSB, clipped linear RMS {l0:.4f}")
    print(" L  sigma_c  k  sigma_z  flags | bytes RMS  ratio | linear RMS  ratio")
    for it, sc_, k, sz, fl in itertools.product((3, 4, 5, 6), (0.25, 0.5, 1.0, 2.0), (1, 3, 5, 7), (0.5, 1.0, 4.0),
                                                ((True, False), (False, False), (True, True))):
        if (sz != 1.0 and (k != 3 or fl != (True, False))) or (fl != (True, False) and (k != 3 or it != 5)):
            continue   # the full grid of L, sigma_c, k at sigma_z 1 with DEMODULATE; the other axes around the default
        out, out8 = G.denoise(image, aov, w, h, iterations=it, sigma_color=sc_, normal_power_log2=k, sigma_depth=sz,
                              demodulate=fl[0], object_edges=fl[1])
        torch.cuda.synchronize()
        b1, l1 = rms(out8.cpu().numpy(), ref8), rms(clip(out.cpu().numpy()), clip(ref))
        flags = ("D" if fl[0] else "-") + ("O" if fl[1] else "-")
        print(f"{it:2d} {sc_:7.2f} {k:2d} {sz:7.2f}  {flags:5s} | {b1:8.2f} {b1 / b0:6.3f} | {l1:10.4f} {l1 / l0:6.3f}", flush=True)
    gs.close()
    sc.free()


if __name__ == "__main__":
    sweep() if "--sweep" in opt else timing()
