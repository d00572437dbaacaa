#!/usr/bin/env python3
"""What moving a mesh in place costs (GpuScene.update_vertices, rt_hip_scene_update_vertices) against recreating the scene, on
config 5's mesh and on generated shells of 1e5 and 1e6 triangles:
  update seconds    the synchronous call with a device tensor of new positions, by the host's clock, after one warm-up update (which
                    makes the level array), median of 5
  recreate seconds  rt_hip_scene_create_opts with the device builder on the moved vertices (uploads, hull facets and the rest
                    included), by the host's clock, after one warm-up, median of 5, in the same session
  tree_cost         of the refitted tree against a fresh device tree of the moved mesh, after scale-and-wobble and after the mirror
  frame             config 5 at 3840 x 2160 x 64 spp through the refitted tree and through a fresh tree of the same (wobbled)
                    mesh, alternating, kernel milliseconds by device events: what a refit costs the walks
usage: python tools/scene_update_bench.py [--out FILE] [--no-frame] [--sizes 100000,1000000]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "raytracer.c_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)


def tris_of(sc):
    import numpy as np
    v = np.ctypeslib.as_array(C.cast(sc.meshes[0].mesh.vertices, C.POINTER(C.c_double)), shape=(3 * sc.n_triangles, 5))
    return v[:, :3].reshape(-1, 3, 3).copy()


def moved_scene(sc, tris):
    """`sc` again with the corners `tris`: the vertex array is written in place and the caller puts it back"""
    import numpy as np
    v = np.ctypeslib.as_array(C.cast(sc.meshes[0].mesh.vertices, C.POINTER(C.c_double)), shape=(3 * sc.n_triangles, 5))
    v[:, :3] = np.asarray(tris).reshape(-1, 3)
    return sc


def timed(call, reps=5):
    call()   # warm-up
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        res = call()
        out.append(time.perf_counter() - t0)
        if hasattr(res, "close"):
            res.close()
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-frame", action="store_true")
    ap.add_argument("--sizes", default="100000,1000000")
    a = ap.parse_args()
    import torch
    import scene_update_meshes as U
    from bvh_build_bench import shell_scene
    from rt_amd import abi, gpu as G, scene as S
    shim = abi.load_shim()
    name = C.create_string_buffer(128)
    shim.rt_hip_device_info(0, name, 128, None)
    lines = [f"device: {name.value.decode()}",
             "mesh, triangles | update s median of 5 (device pointer) | recreate s median of 5 (device builder) | recreate / update | "
             "tree_cost refit / fresh after scale-and-wobble, after mirror"]
    meshes = [("config 5", S.build_scene(5, 192, 108, 2))] + [(f"shell {n}", shell_scene(n)) for n in map(int, a.sizes.split(",")) if n]
    for label, sc in meshes:
        tris = tris_of(sc)
        wob, mir = U.scale_wobble(tris), U.mirror(tris)
        gs = G.GpuScene(sc, bvh="device")
        d_wob = torch.tensor(wob, dtype=torch.float64, device="cuda")
        d_mir = torch.tensor(mir, dtype=torch.float64, device="cuda")
        upd = timed(lambda: gs.update_vertices(d_wob))
        cost = {"wobble": [gs.bvh_info()["tree_cost"]]}
        gs.update_vertices(d_mir)
        cost["mirror"] = [gs.bvh_info()["tree_cost"]]
        gs.close()
        moved_scene(sc, wob)
        rec = timed(lambda: G.GpuScene(sc, bvh="device"))
        for key, t in (("wobble", wob), ("mirror", mir)):
            fresh = G.GpuScene(moved_scene(sc, t), bvh="device")
            cost[key].append(fresh.bvh_info()["tree_cost"])
            fresh.close()
        moved_scene(sc, tris)
        lines.append(f"{label}, {sc.n_triangles} | {upd:.6f} | {rec:.6f} | x{rec / upd:.1f} | "
                     f"{cost['wobble'][0] / cost['wobble'][1]:.4f}, {cost['mirror'][0] / cost['mirror'][1]:.4f}")
        print(lines[-1], flush=True)
    if a.no_frame:
        lines.append("config 5 frame at 3840 x 2160 x 64 spp: unmeasured")
    else:
        sc = S.build_scene(5, 3840, 2160, 64)
        tris = tris_of(sc)
        wob = U.scale_wobble(tris)
        total = G.n_tiles(sc.width, sc.height)
        refit = G.GpuScene(sc, bvh="device")
        refit.update_vertices(torch.tensor(wob, dtype=torch.float64, device="cuda"))
        scenes = {"refitted": refit, "fresh": G.GpuScene(moved_scene(sc, wob), bvh="device")}
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
        lines.append("config 5 (scaled and wobbled) frame at 3840 x 2160 x 64 spp, alternating, ms: " +
                     ", ".join(f"{b} tree {' '.join('%.3f' % v for v in ms[b])} (min {min(ms[b]):.3f})" for b in ms) +
                     f" | kernel {refit.last_launch_kernel()}")
        print(lines[-1], flush=True)
        for gs in scenes.values():
            gs.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
