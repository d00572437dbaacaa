#!/usr/bin/env python3
"""What guided upsampling (rt_hip_upsample) costs and what it buys.
Timing: config 4 (the 38-sphere room), 4 spp: pt_upsample to 1920x1080 from 960x540 and from 640x360, with and without the byte
output, and in the same run, alternating with it, pt_reproject and the denoiser (L = 5) at 1920x1080 and at the two low sizes.
Every figure is the device time of a batch of `batch` back-to-back launches (bare C-ABI calls, arguments marshalled once) between
two HIP events divided by `batch`, after a warm-up batch; the median of `reps` such batches, with their least and largest, and the
host's time per enqueue next to it, which says whether the queue stayed full.
--sweep: the quality table of DESIGN ("`pt_upsample`"): the checkered room (config 4 with M_CHECKERED on the floor) at 192x108
from 96x54, the low frame at 16 spp, first-hit buffers of 16 samples, against 1024 spp at 192x108 of another seed, in clipped linear
RMS, over k, sigma_depth and DEMODULATE; then, per seed of three, (a) the defaults, (b) plain bilinear of the same low frame, (c) a
192x108 frame of 4 spp, and the same with the low frame denoised.
usage: python tools/upsample_bench.py [--reps=R (7)] [--batch=B (100)] [--sweep]"""
import itertools
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "raytracer.c_amd")]
import numpy as np
import torch
from rt_amd import abi, gpu as G, scene as S

SEED = 1666943821
opt = {a.split("=")[0]: (a.split("=") + [""])[1] for a in sys.argv[1:] if a.startswith("--")}
reps = int(opt.get("--reps") or 7)
batch = int(opt.get("--batch") or 100)


def frame(gs, seed, spp, aov_samples=None):
    """the frame's linear mean and its first-hit buffers of the same seed, on the device"""
    total = G.n_tiles(gs.scene.width, gs.scene.height)
    tiles, tiles8, _ = gs.render_tiles(seed, 0, 1, total, samples=spp, chunks=gs.suggest_chunks(total, spp))
    image, _ = gs.untile(tiles, tiles8, 0, 1, total)
    aov = gs.untile_aov(gs.render_aov(seed, aov_samples or spp, 0, 1, total), 0, 1, total)
    torch.cuda.synchronize()
    return image, aov


def batch_ms(fn):
    """-> (device ms per launch between two events around `batch` launches, host ms per enqueue of the same loop)"""
    import time
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    for _ in range(batch):
        fn()
    b.record()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / batch, (t1 - t0) * 1e3 / batch


def timing():
    """every entry is a bare call of the C-ABI with its arguments marshalled once (no parameter struct, tensor check or
    allocation in the timed loop), as the denoiser's"""
    import ctypes as C
    import dataclasses
    w, h = 1920, 1080
    sc = S.build_scene(4, w, h, 4)
    gs = G.GpuScene(sc)
    shim = gs.shim
    rgb, aov = frame(gs, SEED, 4)
    dev = rgb.device
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    cams = S.orbit_cameras(4, w, h)[-2:]
    keep, work, sizes = [], {}, {}
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def pack(bufs):
        a = abi.RtHipAov()
        for f, t in bufs.items():
            setattr(a, f, t.data_ptr())
        keep.append(a)
        return C.byref(a)
    up = abi.upsample_params()
    for wl, hl in ((960, 540), (640, 360)):
        lo = G.GpuScene(dataclasses.replace(sc, width=wl, height=hl))
        low_rgb, low_aov = frame(lo, SEED, 4)
        sizes[(wl, hl)] = (lo, low_rgb, low_aov)
        out = G.upsample(low_rgb, low_aov, wl, hl, aov, w, h)
        keep.append(out)
        la, a = pack(low_aov), pack(aov)
        for want8 in (True, False):
            args = (ptr(low_rgb), la, wl, hl, a, w, h, C.byref(up), ptr(out["rgb"]), ptr(out["rgb8"]) if want8 else None, ptr(out["conf"]),
                    stream)
            work[f"pt_upsample {w}x{h} from {wl}x{hl} {'with' if want8 else 'without'} bytes"] = \
                (lambda args=args: G._check(shim.rt_hip_upsample(*args), "rt_hip_upsample"), w * h)
    rp, dp = abi.reproject_params(), abi.denoise_params()
    for (ww, hh), (image, bufs) in [((w, h), (rgb, aov))] + [(k, (v[1], v[2])) for k, v in sizes.items()]:
        hist = dict(rgb=image.clone(), len=torch.full((hh, ww), 3.0, device=dev), aov={f: t.clone() for f, t in bufs.items()})
        o = G.reproject(image, bufs, cams[1], hist=dict(hist, camera=cams[0]))
        keep += [hist, o]
        args = (ptr(image), pack(bufs), C.byref(cams[1]), ptr(hist["rgb"]), ptr(hist["len"]), pack(hist["aov"]), C.byref(cams[0]), ww, hh,
                C.byref(rp), ptr(o["rgb"]), ptr(o["rgb8"]), ptr(o["len"]), ptr(o["motion"]), stream)
        work[f"pt_reproject {ww}x{hh} with bytes"] = (lambda args=args: G._check(shim.rt_hip_reproject(*args), "rt_hip_reproject"), ww * hh)
        ws = torch.empty(max(shim.rt_hip_denoise_workspace_bytes(ww, hh), 1), dtype=torch.uint8, device=dev)
        den, den8 = torch.empty_like(image), torch.empty((hh, ww, 3), dtype=torch.uint8, device=dev)
        keep += [ws, den, den8]
        args = (ptr(image), pack(bufs), ww, hh, C.byref(dp), ptr(ws), ptr(den), ptr(den8), stream)
        work[f"denoise L=5 {ww}x{hh}"] = (lambda args=args: G._check(shim.rt_hip_denoise(*args), "rt_hip_denoise"), ww * hh)
    for fn, _ in work.values():       # warm-up: every shape the timed window uses
        batch_ms(fn)
    times = {name: [] for name in work}
    for _ in range(reps):             # alternating, so that what else runs on the machine meets every kernel alike
        for name, (fn, _) in work.items():
            times[name].append(batch_ms(fn))
    print(f"# device ms per launch: the time between two HIP events around {batch} back-to-back launches / {batch}; median of {reps} such "
          "batches (least, largest).  host: ms per enqueue of the same loop -- where it is not below the device figure the queue ran "
          "empty and the figure is launch throughput, not kernel time")
    for name, (_, pixels) in work.items():
        t, host = [x[0] for x in times[name]], statistics.median(x[1] for x in times[name])
        med = statistics.median(t)
        note = "" if host < 0.8 * med else "  [host-bound: an upper bound on the kernel's time]"
        print(f"{name}: {med:.4f} ms  (least {min(t):.4f}, largest {max(t):.4f}; {pixels / med * 1e-6:.2f} Gpixel/s; host {host:.4f} ms){note}",
              flush=True)
    for lo, _, _ in sizes.values():
        lo.close()
    gs.close()
    sc.free()


def clip(a):
    return np.clip(np.nan_to_num(np.asarray(a, np.float64), nan=1.0), 0, 1)


def rms(a, b):
    return float(np.sqrt(((clip(a) - clip(b)) ** 2).mean()))


def bilinear(low_rgb, wl, hl, w, h):
    """plain bilinear at rt_hip_upsample's own tap positions: the kernel under guides that are the same everywhere (every g = 1)"""
    dev = low_rgb.device
    flat = lambda ww, hh: dict(normal=torch.zeros((hh, ww, 3), device=dev), depth=torch.zeros((hh, ww), device=dev),
                               hits=torch.zeros((hh, ww), dtype=torch.int32, device=dev))
    return G.upsample(low_rgb, flat(wl, hl), wl, hl, flat(w, h), w, h, out=dict(rgb8=None, conf=None), demodulate=False)["rgb"]


def sweep():
    w, h, wl, hl, spp = 192, 108, 96, 54, 16
    sc = S.build_scene(4, w, h, spp)
    sc.objects[0].flags |= abi.M_CHECKERED        # the floor
    gs = G.GpuScene(sc)
    ref = gs.render_image(SEED + 100, 1024)[0].cpu().numpy()
    pv = gs.preview(2)
    res = pv.frame(SEED, spp)
    low_rgb, low_aov, aov = res["low"]["rgb"], res["low"]["aov"], res["aov"]
    torch.cuda.synchronize()
    b = rms(bilinear(low_rgb, wl, hl, w, h).cpu().numpy(), ref)
    print(f"{w}x{h} from {wl}x{hl}, {spp} spp: plain bilinear: clipped linear RMS {b:.4f}")
    print("  k  sigma_depth  demodulate | linear RMS  ratio to bilinear  mean conf")
    for dm, k, sd in itertools.product((True, False), (0, 2, 3, 5), (0.01, 0.05, 0.2, 1.0)):
        r = G.upsample(low_rgb, low_aov, wl, hl, aov, w, h, sigma_depth=sd, normal_power_log2=k, demodulate=dm)
        torch.cuda.synchronize()
        a = rms(r["rgb"].cpu().numpy(), ref)
        print(f"{k:3d} {sd:12.2f} {str(dm):>11s} | {a:10.4f} {a / b:18.3f} {float(r['conf'].clamp(min=0).mean()):10.3f}", flush=True)
    print("seed | (a) guided  (b) bilinear  (c) 4 spp full  (a)/(b)  (a)/(c) | low frame denoised: (a)  (b)  (a)/(b)  (a)/(c)  conf < 0.5")
    for seed in (SEED, SEED + 1, SEED + 2):
        row = []
        c = rms(gs.render_image(seed, 4)[0].cpu().numpy(), ref)
        for den in (False, True):
            res = pv.frame(seed, spp, denoise=den)
            torch.cuda.synchronize()
            a = rms(res["rgb"].cpu().numpy(), ref)
            b = rms(bilinear(res["low"]["rgb"], wl, hl, w, h).cpu().numpy(), ref)
            row.append((a, b))
        (a, b), (ad, bd) = row
        print(f"{seed} | {a:.4f} {b:.4f} {c:.4f} {a / b:.3f} {a / c:.3f} | {ad:.4f} {bd:.4f} {ad / bd:.3f} {ad / c:.3f} "
              f"{float((res['conf'] < 0.5).float().mean()):.4f}", flush=True)
    pv.close()
    gs.close()
    sc.free()


if __name__ == "__main__":
    sweep() if "--sweep" in opt else timing()
