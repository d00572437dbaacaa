#!/usr/bin/env python3
"""What rebuilding a scene's hierarchy in place costs and buys (GpuScene.rebuild_bvh, bvh_cost, maintain_bvh), in three blocks:
  rebuild / recreate   rt_hip_scene_rebuild_bvh against destroying the scene and creating it again with the device builder from the
                       same (scaled and wobbled) vertices: the host's clock around the synchronous calls, alternating, median of 7
                       after one warm-up each, on config 5's mesh and on generated shells of 1e5 and 1e6 triangles
  cost                 rt_hip_scene_bvh_cost (a kernel and 8 bytes back) against rt_hip_scene_bvh_info's tree_cost (every node
                       downloaded, summed on the host), same scenes, alternating in a loop of their own (right behind a destroy +
                       create the first synchronous call pays for what the frees left behind), median of 7
  ladder               config 5 at 3840 x 2160 x 64 spp under deformations of growing severity -- scale-and-wobble at several
                       amplitudes, a twist about the y axis by 45 / 90 / 180 degrees: the refitted tree's cost ratio
                       (maintain_bvh with a ratio nothing exceeds), kernel milliseconds through the refitted tree and after
                       rebuild_bvh, alternating (min of 3 after a warm-up round), and the frames after which a rebuild has paid for
                       itself: rebuild seconds / (refitted - rebuilt frame seconds)
usage: python tools/bvh_rebuild_bench.py [--out FILE] [--no-ladder] [--sizes 100000,1000000]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "raytracer.c_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
HUGE_RATIO = 1e300


def wobble(t, amp):
    """tests/scene_update_meshes.py's scale_wobble with the sine's amplitude (a fraction of the extent) as a parameter: 0.05 is its"""
    import numpy as np
    t = np.asarray(t, dtype=np.float64)
    c = np.array([0.3, -0.2, 0.1])
    flat = t.reshape(-1, 3)
    ext = float((flat.max(axis=0) - flat.min(axis=0)).max()) or 1.0
    return c + 1.3 * (t - c) + amp * ext * np.sin(2.0 * np.pi * np.roll(t, -1, axis=2) / ext)


def twist(t, degrees):
    """every vertex turned about the y axis through the mesh's centre, by an angle that grows linearly from 0 at the lowest y to
    `degrees` at the highest"""
    import numpy as np
    t = np.array(t, dtype=np.float64)
    flat = t.reshape(-1, 3)
    lo, hi = flat.min(axis=0), flat.max(axis=0)
    cx, cz = 0.5 * (lo[0] + hi[0]), 0.5 * (lo[2] + hi[2])
    a = np.radians(degrees) * (t[..., 1] - lo[1]) / ((hi[1] - lo[1]) or 1.0)
    x, z = t[..., 0] - cx, t[..., 2] - cz
    t[..., 0], t[..., 2] = cx + x * np.cos(a) - z * np.sin(a), cz + x * np.sin(a) + z * np.cos(a)
    return t


def clock(call):
    t0 = time.perf_counter()
    res = call()
    return time.perf_counter() - t0, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-ladder", action="store_true")
    ap.add_argument("--sizes", default="100000,1000000")
    a = ap.parse_args()
    import torch
    from bvh_build_bench import shell_scene
    from rt_amd import abi, gpu as G, scene as S
    from scene_update_bench import moved_scene, tris_of
    shim = abi.load_shim()
    name = C.create_string_buffer(128)
    shim.rt_hip_device_info(0, name, 128, None)
    lines = [f"device: {name.value.decode()}",
             "mesh, triangles | rebuild_bvh s | destroy + create (device builder) s | recreate / rebuild | device build s inside the "
             "rebuild | bvh_cost s | bvh_info tree_cost s | info / cost   (medians of 7, alternating)"]
    meshes = [("config 5", S.build_scene(5, 192, 108, 2))] + [(f"shell {n}", shell_scene(n)) for n in map(int, a.sizes.split(",")) if n]
    for label, sc in meshes:
        tris = tris_of(sc)
        moved_scene(sc, wobble(tris, 0.05))
        gs = G.GpuScene(sc, bvh="device")
        other = G.GpuScene(sc, bvh="device")
        reb, rec, cost, info = [], [], [], []
        for rep in range(8):           # the first round warms up
            t_reb = clock(gs.rebuild_bvh)[0]
            t_rec, other = clock(lambda: (other.close(), G.GpuScene(sc, bvh="device"))[1])
            if rep:
                reb.append(t_reb), rec.append(t_rec)
        torch.cuda.synchronize()
        for rep in range(8):           # (not in the loop above: see the docstring)
            t_cost = clock(gs.bvh_cost)[0]
            t_info = clock(gs.bvh_info)[0]
            if rep:
                cost.append(t_cost), info.append(t_info)
        m = statistics.median
        lines.append(f"{label}, {sc.n_triangles} | {m(reb):.6f} | {m(rec):.6f} | x{m(rec) / m(reb):.1f} | {gs.bvh_info()['build_seconds']:.6f} | "
                     f"{m(cost):.6f} | {m(info):.6f} | x{m(info) / m(cost):.1f}")
        print(lines[-1], flush=True)
        gs.close()
        other.close()
        moved_scene(sc, tris)
    if a.no_ladder:
        lines.append("ladder on config 5 at 3840 x 2160 x 64 spp: unmeasured")
    else:
        sc = S.build_scene(5, 3840, 2160, 64)
        tris = tris_of(sc)
        total = G.n_tiles(sc.width, sc.height)
        lines.append("config 5 at 3840 x 2160 x 64 spp | cost_ratio of the refitted tree | refitted ms (min of 3) | rebuilt ms (min of 3) | "
                     "refitted / rebuilt | rebuild s | frames until a rebuild has paid for itself | kernel")
        ladder = [("wobble 0.05", wobble(tris, 0.05)), ("wobble 0.10", wobble(tris, 0.10)), ("wobble 0.20", wobble(tris, 0.20)),
                  ("wobble 0.40", wobble(tris, 0.40)), ("twist 45", twist(tris, 45)), ("twist 90", twist(tris, 90)),
                  ("twist 180", twist(tris, 180))]
        for label, new in ladder:
            d_new = torch.tensor(new, dtype=torch.float64, device="cuda")
            scenes = {"refitted": G.GpuScene(sc, bvh="device"), "rebuilt": G.GpuScene(sc, bvh="device")}
            for gs in scenes.values():
                gs.update_vertices(d_new)
            ratio = scenes["refitted"].maintain_bvh(HUGE_RATIO)["cost_ratio"]
            scenes["rebuilt"].rebuild_bvh()
            t_reb = scenes["rebuilt"].rebuild_info()["last_seconds"]
            ms = {b: [] for b in scenes}
            for rep in range(4):       # the first round warms up
                for b, gs in scenes.items():
                    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                    ev[0].record()
                    gs.render_tiles(1666943821, 0, 1, total, chunks=gs.suggest_chunks(total))
                    ev[1].record()
                    torch.cuda.synchronize()
                    if rep:
                        ms[b].append(ev[0].elapsed_time(ev[1]))
            fit, reb = min(ms["refitted"]), min(ms["rebuilt"])
            pays = f"{t_reb / (1e-3 * (fit - reb)):.1f}" if fit > reb else "never (the refitted tree is no slower)"
            lines.append(f"{label} | {ratio:.4f} | {fit:.3f} | {reb:.3f} | {fit / reb:.4f} | {t_reb:.6f} | {pays} | "
                         f"{scenes['refitted'].last_launch_kernel()}")
            print(lines[-1], flush=True)
            for gs in scenes.values():
                gs.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
