#!/usr/bin/env python3
"""What adaptive sampling (rt_hip_accum_run_adaptive) buys against the uniform accumulation.
For a scene (--config=4 at 1920x1080 by default; --width, --height) and a budget (--budget=256): the ground truth is a uniform
frame of 16 x the budget with another seed.  For every threshold of a decade around the starting value (--thresholds=a,b,...):
mean samples per pixel, share of the tiles at the full budget, device seconds of all passes + resolves + estimates + freezes,
and the error against the ground truth -- RMS of the tonemapped bytes and of the linear values clipped to [0, 1], the two
measures of tools/denoise_bench.py -- next to uniform accumulations at the budget and at the sample count nearest the adaptive
run's mean.  The last column is the uniform accumulation's device time at the adaptive run's error, interpolated in log-log
between the uniform rows: time to equal error.
usage: python tools/adaptive_bench.py [--config=4] [--width=1920] [--height=1080] [--budget=256] [--min-samples=16] [--dilate=1]
                                       [--thresholds=0.005,0.01,0.02,0.05,0.1] [--truth-factor=16] [--json=FILE]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "raytracer.c_amd")]
import numpy as np
import torch
from rt_amd import gpu as G, scene as S

SEED = 1666943821
opt = {a.split("=")[0]: (a.split("=") + [""])[1] for a in sys.argv[1:] if a.startswith("--")}
config = int(opt.get("--config") or 4)
w, h = int(opt.get("--width") or 1920), int(opt.get("--height") or 1080)
budget = int(opt.get("--budget") or 256)
min_samples = int(opt.get("--min-samples") or 16)
dilate = int(opt.get("--dilate") or 1)
thresholds = [float(x) for x in (opt.get("--thresholds") or "0.005,0.01,0.02,0.05,0.1").split(",")]
truth_factor = int(opt.get("--truth-factor") or 16)


def errors(img, img8, truth, truth8):
    lin = np.sqrt(np.mean((np.clip(img, 0, 1).astype(np.float64) - np.clip(truth, 0, 1)) ** 2))
    byt = np.sqrt(np.mean((img8.astype(np.float64) - truth8) ** 2))
    return float(byt), float(lin)


def uniform(gs, spp, total):
    """a uniform accumulation of spp samples in passes of at most 64 -> (image, image8, device seconds)"""
    acc = gs.accumulate(SEED, spp)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    while acc.samples < spp:
        acc.add(min(64, spp - acc.samples))
    t, t8 = acc.resolve()
    b.record()
    torch.cuda.synchronize()
    img, img8 = gs.untile(t, t8, 0, 1, total)
    torch.cuda.synchronize()
    acc.close()
    return img.cpu().numpy(), img8.cpu().numpy(), a.elapsed_time(b) * 1e-3


def main():
    sc = S.build_scene(config, w, h, budget)
    gs = G.GpuScene(sc)
    total = G.n_tiles(w, h)
    timg, timg8, _ = gs.render_image(SEED + 1, budget * truth_factor)
    truth, truth8 = timg.cpu().numpy().astype(np.float64), timg8.cpu().numpy().astype(np.float64)
    rows, uni = [], {}

    def uniform_row(spp):
        if spp not in uni:
            img, img8, secs = uniform(gs, spp, total)
            uni[spp] = (secs,) + errors(img, img8, truth, truth8)
        return uni[spp]

    for spp in sorted({budget, max(1, budget // 2), max(1, budget // 4), max(1, budget // 8)}):
        uniform_row(spp)
    for thr in thresholds:
        img, img8, counts, st, secs = gs.render_adaptive(SEED, budget, threshold=thr, min_samples=min_samples, dilate=dilate)
        mean = st["samples"] / (w * h)
        byt, lin = errors(img.cpu().numpy(), img8.cpu().numpy(), truth, truth8)
        near = max(1, int(round(mean)))
        usecs, ubyt, ulin = uniform_row(near)
        # the uniform accumulation's time at this error: log-log interpolation over the uniform rows (error falls with time)
        pts = sorted((e[2], e[0]) for e in uni.values())
        xs, ys = np.log([p[0] for p in pts]), np.log([p[1] for p in pts])
        equal = float(np.exp(np.interp(np.log(lin), xs, ys)))
        rows.append(dict(threshold=thr, mean_spp=mean, full_budget_share=float((counts >= budget).mean()), seconds=secs, byte_rms=byt,
                         linear_rms=lin, uniform_spp=near, uniform_seconds=usecs, uniform_byte_rms=ubyt, uniform_linear_rms=ulin,
                         uniform_seconds_at_equal_error=equal))
    print(f"config {config} at {w} x {h}, budget {budget}, min_samples {min_samples}, dilate {dilate}, {gs.kernel_name()}; "
          f"ground truth {budget * truth_factor} spp of another seed")
    print("uniform:   " + "  ".join(f"{spp} spp {v[0] * 1e3:.1f} ms byte {v[1]:.3f} lin {v[2]:.5f}" for spp, v in sorted(uni.items())))
    print(f"{'threshold':>9} {'mean spp':>9} {'full %':>7} {'ms':>8} {'byte rms':>9} {'lin rms':>9} | {'uni spp':>7} {'ms':>8} {'byte rms':>9} "
          f"{'lin rms':>9} | {'uniform ms at equal error':>25}")
    for r in rows:
        print(f"{r['threshold']:9g} {r['mean_spp']:9.2f} {100 * r['full_budget_share']:7.1f} {r['seconds'] * 1e3:8.2f} {r['byte_rms']:9.3f} "
              f"{r['linear_rms']:9.5f} | {r['uniform_spp']:7d} {r['uniform_seconds'] * 1e3:8.2f} {r['uniform_byte_rms']:9.3f} "
              f"{r['uniform_linear_rms']:9.5f} | {r['uniform_seconds_at_equal_error'] * 1e3:25.2f}")
    if opt.get("--json"):
        json.dump(dict(config=config, width=w, height=h, budget=budget, min_samples=min_samples, dilate=dilate,
                       uniform={str(k): v for k, v in uni.items()}, rows=rows), open(opt["--json"], "w"), indent=1)
    gs.close()
    sc.free()


if __name__ == "__main__":
    main()
