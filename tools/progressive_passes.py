#!/usr/bin/env python3
"""What progressive rendering costs: one frame (default BASELINE config 4: 1920x1080, 1024 spp, depth 16) rendered one-shot
(rt_hip_render_tiles_chunked at the suggested chunks, as bench.py does) against the same frame accumulated in passes
(rt_hip_accum_*: GpuScene.accumulate) of 256 and of 64 spp.  Device time by HIP events around the whole frame -- every pass and
the final resolve -- best of `reps`; the final frames are compared bit for bit with the one-shot frame.
usage: python tools/progressive_passes.py [scene=4] [spp=1024] [pass_spp ...=256 64] [--reps R=3]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "raytracer.c_amd")]
import torch
import bench
from rt_amd import gpu as G

args = [a for a in sys.argv[1:] if not a.startswith("--")]
reps = int(next((a.split("=")[1] for a in sys.argv[1:] if a.startswith("--reps=")), 3))
name = args[0] if args else "4"
spp = int(args[1]) if len(args) > 1 else 1024
passes = [int(a) for a in args[2:]] or [256, 64]


def timed(start, run, finish=lambda x: None):
    """best device time of reps runs (after one warm-up), ms, and the last run's result: start() outside the timed window,
    run(state) inside it, finish(state) after it"""
    best, out = None, None
    for k in range(reps + 1):
        state = start()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = run(state)
        b.record()
        torch.cuda.synchronize()
        finish(state)
        if k:
            best = a.elapsed_time(b) if best is None else min(best, a.elapsed_time(b))
    return best, out


sc = bench.make_scene(name, None, None, spp)
gs = G.GpuScene(sc)
total = G.n_tiles(sc.width, sc.height)
chunks = gs.suggest_chunks(total)
ref = torch.empty((total, 64, 3), dtype=torch.float32, device="cuda")
ref8 = torch.empty((total, 64, 3), dtype=torch.uint8, device="cuda")
one_ms, _ = timed(lambda: None, lambda _: gs.render_tiles(bench.SEED, 0, 1, total, tiles=ref, tiles8=ref8, chunks=chunks))
kernel = gs.last_launch_kernel()
print(f"scene {name}: {sc.width}x{sc.height} x {spp} spp, depth {sc.max_depth}, {kernel}: one-shot {one_ms:.2f} ms "
      f"({chunks} chunks)", flush=True)
tiles, tiles8 = torch.empty_like(ref), torch.empty_like(ref8)
for p in passes:
    def run(acc):
        member[0] = acc.kernel
        left = spp
        while left:
            acc.add(min(p, left))
            left -= min(p, left)
        return acc.resolve(tiles, tiles8)
    # creation (allocation, clearing) and destruction are outside the timed window
    member = [""]
    ms, (t, t8) = timed(lambda: gs.accumulate(bench.SEED, spp), run, lambda acc: acc.close())
    same = torch.equal(t, ref) and torch.equal(t8, ref8)
    print(f"  passes of {p:5d} spp ({(spp + p - 1) // p:3d} passes, {member[0]}): {ms:.2f} ms = "
          f"{100.0 * (ms / one_ms - 1.0):+.1f} % against one-shot; final frame bit-identical: {same}", flush=True)
    if not same:
        sys.exit(1)
gs.close()
