#!/usr/bin/env python3
"""Kernel time and rays/s of the ray-query kernels (rt_hip_query_rays) on config 4's room and config 5's mesh, 1920 x 1080 rays each:
  (a) the pixel-centre camera rays (u, v) in row-major order,
  (b) the same rays in 8x8-tile order (a wave = one tile, as the render kernels have it),
  (c) as many rays with uniformly random origins inside the scene's bounds and random unit directions;
and next to (b) the kernel time of rt_hip_render_aov_tiles at S = 1 on the same frame, which scans the same number of camera rays.
Device events around `--reps` launches after `--warmup`, the median per launch.  Needs the GPU: there is no CPU path.
usage: tools/query_bench.py [--out FILE] [--reps N] [--warmup N] [--width W --height H]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "raytracer.c_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(torch, fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    args = ap.parse_args()
    import numpy as np
    import torch
    from rt_amd import abi, gpu, scene
    import util
    if not torch.cuda.is_available() or abi.load_shim().rt_hip_device_count() < 1:
        sys.exit("query_bench needs a GPU: there is no CPU path")
    w, h = args.width, args.height
    n = w * h
    lines = [f"ray queries, {w} x {h} = {n} rays per launch, median of {args.reps} launches after {args.warmup} (min .. max), device events",
             f"device: {torch.cuda.get_device_name(0)}"]
    ys, xs = np.divmod(np.arange(n), w)
    uv_rows = np.stack([(xs + 0.5) / (w - 1), (ys + 0.5) / (h - 1)], axis=1)
    tx, ty = (w + 7) // 8, (h + 7) // 8
    t, p = np.divmod(np.arange(tx * ty * 64), 64)
    px, py = (t % tx) * 8 + (p & 7), (t // tx) * 8 + (p >> 3)
    keep = (px < w) & (py < h)
    uv_tiles = np.stack([(px[keep] + 0.5) / (w - 1), (py[keep] + 0.5) / (h - 1)], axis=1)
    for config in (4, 5):
        sc = scene.build_scene(config, w, h, 1)
        gs = gpu.GpuScene(sc)
        objs, meshes = util.scene_parts(sc)
        # the scene's bounds: the spheres of ordinary size and every vertex (a room's walls are spheres of radius >= 1000)
        lo = np.min([np.array(o["center"]) - o["radius"] for o in objs if o["radius"] < 1000] + [m["vertices"][:, :3].min(axis=0) for m in meshes], axis=0)
        hi = np.max([np.array(o["center"]) + o["radius"] for o in objs if o["radius"] < 1000] + [m["vertices"][:, :3].max(axis=0) for m in meshes], axis=0)
        rng = np.random.default_rng(config)
        d = rng.normal(size=(n, 3))
        d /= np.sqrt((d * d).sum(axis=1))[:, None]
        random_rays = np.concatenate([rng.uniform(lo, hi, (n, 3)), d], axis=1)
        radius = float(np.abs(np.stack([lo, hi])).max() * 3 ** 0.5)
        dev = torch.device("cuda", 0)
        cases = [("(a) pixel centres, row-major", lambda r=torch.as_tensor(uv_rows, device=dev): gs.query_uv(r)),
                 ("(b) pixel centres, 8x8 tiles", lambda r=torch.as_tensor(uv_tiles, device=dev): gs.query_uv(r)),
                 ("(c) random origins and directions", lambda r=torch.as_tensor(random_rays, device=dev): gs.query_rays(r, origin_radius=radius))]
        lines.append(f"config {config}: {sc.n_objects} spheres, {sc.n_triangles} triangles; query kernel {gs.query_kernel_name()}, "
                     f"AOV kernel {gs.aov_kernel_name()}")
        res = {}
        for name, fn in cases:
            out = fn()
            torch.cuda.synchronize()
            hits = int((out["status"] == 1).sum())
            med, lo_ms, hi_ms = timed(torch, fn, args.warmup, args.reps)
            res[name[:3]] = med
            lines.append(f"  {name:36s} {med:8.3f} ms ({lo_ms:.3f} .. {hi_ms:.3f})  {n / med / 1e6:8.2f} Grays/s  hits {hits}")
        total = gpu.n_tiles(w, h)
        med, lo_ms, hi_ms = timed(torch, lambda: gs.render_aov(1666943821, 1, 0, 1, total), args.warmup, args.reps)
        lines.append(f"  {'rt_hip_render_aov_tiles, S = 1':36s} {med:8.3f} ms ({lo_ms:.3f} .. {hi_ms:.3f})")
        lines.append(f"  (b) / AOV = {res['(b)'] / med:.2f}   (a) / (b) = {res['(a)'] / res['(b)']:.2f}   (c) / (b) = {res['(c)'] / res['(b)']:.2f}")
        lines.append("  (the timed window of a query holds its eight output allocations too; the AOV launch's holds its five)")
        gs.close()
        sc.free()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
