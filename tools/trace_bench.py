#!/usr/bin/env python3
"""Kernel time and ray-bounces/s of the radiance-query kernels (rt_hip_trace_rays) on config 4's room and config 5's mesh: the
1920 x 1080 pixel-centre camera rays (from query_uv, in 8x8-tile order) traced GIVEN at S = 16, depth 16, next to render_tiles of the
same scene at 16 spp (the pooled or parked-walk member).  Device events around `--reps` launches after `--warmup`, the median per
launch; ray-bounces are the launches' own `casts` counters.  Needs the GPU: there is no CPU path.
usage: tools/trace_bench.py [--out FILE] [--reps N] [--warmup N] [--width W --height H] [--samples S] [--depth D]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "raytracer.c_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from query_bench import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--depth", type=int, default=16)
    args = ap.parse_args()
    import numpy as np
    import torch
    from rt_amd import abi, gpu, scene
    if not torch.cuda.is_available() or abi.load_shim().rt_hip_device_count() < 1:
        sys.exit("trace_bench needs a GPU: there is no CPU path")
    w, h, S, D = args.width, args.height, args.samples, args.depth
    seed = 1666943821
    lines = [f"radiance queries, {w} x {h} rays x {S} samples at depth {D}, median of {args.reps} launches after {args.warmup} (min .. max), device events",
             f"device: {torch.cuda.get_device_name(0)}"]
    tx, ty = (w + 7) // 8, (h + 7) // 8
    t, p = np.divmod(np.arange(tx * ty * 64), 64)
    px, py = (t % tx) * 8 + (p & 7), (t // tx) * 8 + (p >> 3)
    keep = (px < w) & (py < h)
    uv = np.stack([(px[keep] + 0.5) / (w - 1), (py[keep] + 0.5) / (h - 1)], axis=1)
    dev = torch.device("cuda", 0)
    for config in (4, 5):
        sc = scene.build_scene(config, w, h, S, D)
        gs = gpu.GpuScene(sc)
        rays = gs.query_uv(torch.as_tensor(uv, device=dev), want=("ray",))["ray"]
        x, y, z = sc.camera.position.tuple()
        radius = (x * x + y * y + z * z) ** 0.5
        out = gs.trace_rays(rays, S, seed, origin_radius=radius)
        torch.cuda.synchronize()
        casts_t = int(out["stats"][1])
        total = gpu.n_tiles(w, h)
        chunks = gs.suggest_chunks(total, S, D)
        _, _, st = gs.render_tiles(seed, 0, 1, total, chunks=chunks)
        torch.cuda.synchronize()
        casts_r = int(st[1])
        mt = timed(torch, lambda: gs.trace_rays(rays, S, seed, origin_radius=radius), args.warmup, args.reps)
        mr = timed(torch, lambda: gs.render_tiles(seed, 0, 1, total, chunks=chunks), args.warmup, args.reps)
        lines.append(f"config {config}: {sc.n_objects} spheres, {sc.n_triangles} triangles; trace kernel {gs.trace_kernel_name()}, "
                     f"render kernel {gs.last_launch_kernel()} ({chunks} chunks)")
        lines.append(f"  {'trace_rays':14s} {mt[0]:9.3f} ms ({mt[1]:.3f} .. {mt[2]:.3f})  {casts_t} ray-bounces  {casts_t / mt[0] / 1e6:8.3f} G/s")
        lines.append(f"  {'render_tiles':14s} {mr[0]:9.3f} ms ({mr[1]:.3f} .. {mr[2]:.3f})  {casts_r} ray-bounces  {casts_r / mr[0] / 1e6:8.3f} G/s")
        lines.append(f"  time per ray-bounce, trace_rays / render_tiles = {(mt[0] / casts_t) / (mr[0] / casts_r):.2f}")
        gs.close()
        sc.free()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
