#!/usr/bin/env python3
"""What pixel refinement (rt_hip_select_pixels, rt_hip_trace_pixels, rt_hip_blend_pixels) costs and what it buys.
1. select: the launches of one rt_hip_select_pixels call at 1920x1080 on maps with 1 %, 10 % and 100 % of the pixels selected.
2. trace: rt_hip_trace_pixels next to rt_hip_trace_rays (CAMERA_UV, the pixels' centre rays: the only route before) on the same
   list -- every 10th pixel of the 1080p frame -- at S = 16, depth 16, on config 4's room and config 5's mesh.
3. quality: the checkered room at 192x108 from 1/2 and 1/3 of the size, 16 spp low frame, OBJECT_EDGES, against 1024 spp of
   another seed in clipped linear RMS: (i) the upsampled preview, (ii) preview + fill at S = 4 and 16, (iii) a full-size render of
   16 spp, each with the device time of everything the frame launches.
Every time is the device time between two HIP events around one call (or one frame) after a warm-up call, the median of `reps`
repeats with their least and largest.
usage: python tools/refine_bench.py [--reps=R (7)]   (writes nothing itself: redirect it to profiles/r10_refine_bench.txt)"""
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


def timed(fn):
    """-> 'median ms (least, largest)' of fn's device time over `reps` runs after one warm-up run, and the median"""
    fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        t.append(a.elapsed_time(b))
    med = statistics.median(t)
    return f"{med:.4f} ms (least {min(t):.4f}, largest {max(t):.4f})", med


def select_times():
    import ctypes as C
    w, h = 1920, 1080
    shim = abi.load_shim()
    rng = np.random.default_rng(1)
    u = torch.from_numpy(rng.uniform(0.0, 1.0, (h, w)).astype(np.float32)).cuda()
    ws = torch.empty(shim.rt_hip_select_workspace_bytes(w, h), dtype=torch.uint8, device="cuda")
    idx, count = torch.empty(w * h, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for share in (0.01, 0.10, 1.00):
        call = lambda: G._check(shim.rt_hip_select_pixels(C.c_void_p(u.data_ptr()), w, h, 0.0, share, 0, C.c_void_p(ws.data_ptr()),
                                                          C.c_void_p(idx.data_ptr()), w * h, C.c_void_p(count.data_ptr()), stream),
                                "rt_hip_select_pixels")
        text, _ = timed(call)
        print(f"select {w}x{h}, {int(count.cpu()[0])} of {w * h} selected ({share:.0%}): {text}", flush=True)


def trace_times():
    w, h, spp, depth = 1920, 1080, 16, 16
    for config in (4, 5):
        sc = S.build_scene(config, w, h, spp, depth)
        gs = G.GpuScene(sc)
        pixels = torch.arange(0, w * h, 10, dtype=torch.int32, device="cuda")
        x, y = (pixels % w).double(), (pixels // w).double()
        uv = torch.stack([(x + 0.5) / (w - 1.0), (y + 0.5) / (h - 1.0)], dim=1).contiguous()
        stats = torch.zeros(abi.NSTATS, dtype=torch.int64, device="cuda")
        a, _ = timed(lambda: gs.trace_pixels(pixels, spp, SEED, stats=stats))
        b, _ = timed(lambda: gs.trace_uv(uv, spp, SEED, stats=stats))
        print(f"config {config}, {pixels.numel()} pixels, S = {spp}, depth {depth}: {gs.pixel_kernel_name()} {a}; "
              f"{gs.trace_kernel_name()} (CAMERA_UV, centre rays) {b}", flush=True)
        gs.close()
        sc.free()


def clip_rms(a, b):
    c = lambda v: np.clip(np.nan_to_num(np.asarray(v, np.float64), nan=1.0), 0, 1)
    return float(np.sqrt(((c(a) - c(b)) ** 2).mean()))


def quality():
    w, h, spp = 192, 108, 16
    sc = S.build_scene(4, w, h, spp)
    sc.objects[0].flags |= abi.M_CHECKERED        # the floor
    gs = G.GpuScene(sc)
    ref = gs.render_image(SEED + 100, 1024)[0].cpu().numpy()
    text, _ = timed(lambda: gs.render_image(SEED, spp))
    print(f"{w}x{h}: a full-size render of {spp} spp: clipped linear RMS {clip_rms(gs.render_image(SEED, spp)[0].cpu().numpy(), ref):.4f}, {text}")
    for scale in (2, 3):
        pv = gs.preview(scale, object_edges=True)
        for fill in (None, 4, 16):
            res = pv.frame(SEED, spp, fill=fill)
            torch.cuda.synchronize()
            text, _ = timed(lambda: pv.frame(SEED, spp, fill=fill))
            print(f"{w}x{h} from {pv.low_width}x{pv.low_height}, fill {fill} ({res.get('filled', 0)} pixels): clipped linear RMS "
                  f"{clip_rms(res['rgb'].cpu().numpy(), ref):.4f}, {text}", flush=True)
        pv.close()
    gs.close()
    sc.free()


if __name__ == "__main__":
    print(f"# device ms between two HIP events around one call or frame, after a warm-up: median of {reps} (least, largest); a frame's "
          "figure includes its allocations and, with fill, the 4-byte read-back of the count")
    select_times()
    trace_times()
    quality()
