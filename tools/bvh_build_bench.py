#!/usr/bin/env python3
"""Host against device builds of the triangle hierarchy (rt_hip_scene_create_opts, RT_HIP_BVH_HOST / RT_HIP_BVH_DEVICE) on config 5's
mesh and on generated shells of 1e5 and 1e6 triangles:
  build seconds   the host builder by the host's clock around BvhBuild (the existing path, unchanged); the device builder by device
                  events around its kernels, after one warm-up build, median of 5 (rt_hip_scene_bvh_build_seconds)
  create seconds  the whole rt_hip_scene_create_opts call by the host's clock (uploads, hull facets and the rest included)
  tree_cost       both trees', by BvhBuild::tree_cost()'s formula (rt_hip_scene_bvh_info)
  frame           config 5 at 3840 x 2160 x 64 spp through each tree, alternating, kernel milliseconds by device events
usage: python tools/bvh_build_bench.py [--out FILE] [--no-frame] [--sizes 100000,1000000]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "raytracer.c_amd"))


def shell_scene(n, seed=15, size=0.004):
    import numpy as np
    from rt_amd import abi, scene as S
    rng = np.random.default_rng(seed)
    c = rng.normal(size=(n, 1, 3))
    c /= np.linalg.norm(c, axis=2, keepdims=True)
    tris = c + rng.normal(size=(n, 3, 3)) * size
    objs = [dict(flags=abi.M_DEFAULT, radius=4.0, center=(0, 18, 0), color=(1, 1, 1), emission=(8, 8, 8))]
    return S.custom_scene(objs, 64, 40, 2, 5, (0, 0, 4), (0, 0, 0), meshes=[dict(flags=abi.M_DEFAULT, color=(0.8, 0.7, 0.6), triangles=tris)])


def build(G, sc, bvh):
    t0 = time.perf_counter()
    gs = G.GpuScene(sc, bvh=bvh)
    wall = time.perf_counter() - t0
    info = gs.bvh_info()
    gs.close()
    return info, wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-frame", action="store_true")
    ap.add_argument("--sizes", default="100000,1000000")
    a = ap.parse_args()
    import torch
    from rt_amd import abi, gpu as G, scene as S
    shim = abi.load_shim()
    name = C.create_string_buffer(128)
    shim.rt_hip_device_info(0, name, 128, None)
    lines = [f"device: {name.value.decode()}", "mesh, triangles | host build s (create s) tree_cost | device build s median of 5 (create s) "
             "tree_cost | build speed-up, cost ratio device / host"]
    meshes = [("config 5", S.build_scene(5, 192, 108, 2))] + [(f"shell {n}", shell_scene(n)) for n in map(int, a.sizes.split(",")) if n]
    for label, sc in meshes:
        host, host_wall = build(G, sc, "host")
        build(G, sc, "device")   # warm-up
        runs = [build(G, sc, "device") for _ in range(5)]
        dev = runs[0][0]
        dev_s = statistics.median(r[0]["build_seconds"] for r in runs)
        dev_wall = statistics.median(r[1] for r in runs)
        lines.append(f"{label}, {sc.n_triangles} | {host['build_seconds']:.6f} ({host_wall:.4f}) {host['tree_cost']:.3f} | {dev_s:.6f} "
                     f"({dev_wall:.4f}) {dev['tree_cost']:.3f} | x{host['build_seconds'] / dev_s:.1f}, {dev['tree_cost'] / host['tree_cost']:.4f}"
                     f" | depth {host['depth']} / {dev['depth']} of {dev['max_depth']}, nodes {host['n_nodes']} / {dev['n_nodes']}")
        print(lines[-1], flush=True)
    if a.no_frame:
        lines.append("config 5 frame at 3840 x 2160 x 64 spp: unmeasured")
    else:
        sc = S.build_scene(5, 3840, 2160, 64)
        total = G.n_tiles(sc.width, sc.height)
        scenes = {b: G.GpuScene(sc, bvh=b) for b in ("host", "device")}
        ms = {b: [] for b in scenes}
        for rep in range(4):   # the first round warms up
            for b, gs in scenes.items():
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                ev[0].record()
                gs.render_tiles(1666943821, 0, 1, total, chunks=gs.suggest_chunks(total))
                ev[1].record()
                torch.cuda.synchronize()
                if rep:
                    ms[b].append(ev[0].elapsed_time(ev[1]))
        lines.append("config 5 frame at 3840 x 2160 x 64 spp, alternating, ms: " +
                     ", ".join(f"{b} tree {' '.join('%.3f' % v for v in ms[b])} (min {min(ms[b]):.3f})" for b in ms) +
                     f" | kernel {scenes['device'].last_launch_kernel()}")
        print(lines[-1], flush=True)
        for gs in scenes.values():
            gs.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
