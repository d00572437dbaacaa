#!/usr/bin/env python3
"""When the workgroups of a launch begin and end, and how empty the device is while the launch drains (PT_PHASE build:
make variant NAME=phase DEFS="-DPT_PHASE"; RT_HIP_PHASE_WG_TIMES=1 makes every workgroup of the pooled kernels note both times
on the device's constant clock behind the phase sums).
usage: RT_HIP_SHIM_PATH=raytracer.c_amd/csrc/variants/librt_hip_phase.so python tools/grid_tail.py [config] [spp]
       (RT_HIP_GRID_UNIFORM=1 / RT_HIP_GRID_SPLIT=<n_whole>,<chunks>: the arm)"""
import os, sys
os.environ["RT_HIP_PHASE_WG_TIMES"] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "raytracer.c_amd"))
import numpy as np
import torch
from rt_amd import gpu as G, scene as S
cfg = int(sys.argv[1]) if len(sys.argv) > 1 else 4
spp = int(sys.argv[2]) if len(sys.argv) > 2 else 0
sc = S.build_scene(cfg, samples=spp or None)
gs = G.GpuScene(sc)
tiles = G.n_tiles(sc.width, sc.height)
# room for the arm's workgroups: the kernel writes two words per workgroup behind the phase sums and knows no bound.  The default
# arm is the rule's (at most 4 workgroups a tile); a forced split says how many it launches
MAX_WG = tiles * 4
if os.environ.get("RT_HIP_GRID_UNIFORM") != "1" and os.environ.get("RT_HIP_GRID_SPLIT"):
    try:
        n_whole, n_chunks = (int(v) for v in os.environ["RT_HIP_GRID_SPLIT"].split(","))
    except ValueError:
        sys.exit("RT_HIP_GRID_SPLIT must be <n_whole>,<chunks>")
    if n_whole < 0 or n_chunks < 0:
        sys.exit("RT_HIP_GRID_SPLIT must be <n_whole>,<chunks>, both >= 0")
    MAX_WG = max(tiles, min(n_whole, tiles) + max(tiles - n_whole, 0) * n_chunks)
stats = torch.zeros(80 + 2 * MAX_WG, dtype=torch.int64, device="cuda")
for _ in range(2):   # warm: the first launch of a process pays cold TLBs and instruction fetch
    gs.render_tiles(1666943821, 0, 1, tiles, stats=stats)
torch.cuda.synchronize()
stats.zero_()
ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
ev[0].record()
gs.render_tiles(1666943821, 0, 1, tiles, stats=stats)
ev[1].record()
torch.cuda.synchronize()
ms = ev[0].elapsed_time(ev[1])
t = stats.cpu().numpy()[80:].reshape(-1, 2)
t = t[t[:, 1] != 0]
b, e = t[:, 0].astype(np.float64), t[:, 1].astype(np.float64)
t0, t1 = b.min(), e.max()
tick_ms = ms / (t1 - t0)   # the launch by events (with the resolve, where there is one) over the kernel's span in ticks: ~1e-5 ms
b, e = (b - t0) * tick_ms, (e - t0) * tick_ms
frame = e.max()
# resident workgroups over time: +1 at a begin, -1 at an end
times = np.concatenate([b, e])
delta = np.concatenate([np.ones_like(b), -np.ones_like(e)])
order = np.argsort(times, kind="stable")
times, res = times[order], np.cumsum(delta[order])
full = res.max()
dry = b.max()                                   # the dispatcher hands out its last workgroup
seg = np.diff(np.append(times, frame))
tail = times >= dry
empty_ms = float(((full - res[tail]) * seg[tail]).sum() / full)   # workgroup slots left empty from there on, in full-device ms
print(f"kernel {gs.last_launch_kernel()}, config {cfg}, {sc.samples} spp, arm {os.environ.get('RT_HIP_GRID_SPLIT') or ('uniform' if os.environ.get('RT_HIP_GRID_UNIFORM') == '1' else 'default')}")
print(f"  launch by events {ms:.3f} ms; {len(b)} workgroups, at most {int(full)} resident; a workgroup lives {np.mean(e - b):.3f} ms (median {np.median(e - b):.3f}, max {np.max(e - b):.3f})")
print(f"  last workgroup dispatched at {dry:.3f} ms, last ends at {frame:.3f} ms: the drain lasts {frame - dry:.3f} ms = {100 * (frame - dry) / frame:.2f} % of the frame")
print(f"  empty workgroup slots during the drain: {empty_ms:.3f} full-device ms = {100 * empty_ms / frame:.2f} % of the frame")
print("  the frame's last 10 ms, 0.5 ms bins: [bin start] workgroups ending, resident at the bin's end")
for k in range(20, 0, -1):
    lo, hi = frame - 0.5 * k, frame - 0.5 * (k - 1)
    n_end = int(((e > lo) & (e <= hi)).sum())
    r = int(res[np.searchsorted(times, hi, side="right") - 1]) if hi < frame else 0
    print(f"    [{lo:8.3f}] {n_end:5d} {r:5d}")
gs.close()
