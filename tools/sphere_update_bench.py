#!/usr/bin/env python3
"""What moving a scene's spheres in place costs (GpuScene.update_spheres, rt_hip_scene_update_spheres) against destroying the
scene and creating it again from the same spheres, at 38 (config 4), 1,000 and 100,000 spheres:
  update ms        the synchronous call with a device tensor, by the host's clock, after one warm-up, median of 7
  recreate ms      close + rt_hip_scene_create of the moved spheres, by the host's clock, after one warm-up, median of 7
  first launch ms  the first frame after each (48 x 32, 1 spp; the host's clock around launch and synchronize): the stale table
                   set is rebuilt there after an update, built for the first time after a recreate
and pt_prev_points_moved next to pt_prev_points on 1920 x 1080 entries (device events, after a warm-up, best of 20).
usage: python tools/sphere_update_bench.py [--out FILE] [--sizes 1000,100000]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "raytracer.c_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def cloud_scene(n, seed=3):
    """config 4's eight leading spheres and a cloud of n - 8 small ones in the room"""
    import numpy as np
    from rt_amd import abi, scene as S
    room = S.build_scene(4, 48, 32, 1)
    objs = [dict(flags=int(o.flags), radius=float(o.radius), center=o.center.tuple(), color=o.color.tuple(), emission=o.emission.tuple())
            for o in (room.objects[i] for i in range(8))]
    room.free()
    rng = np.random.default_rng(seed)
    r = 0.5 * (30.0 / max(n, 30)) ** (1.0 / 3.0)
    for c in rng.uniform(-18, 18, (n - 8, 3)):
        objs.append(dict(flags=abi.M_DEFAULT, radius=float(r), center=tuple(c), color=(0.8, 0.8, 0.8)))
    return S.custom_scene(objs, 48, 32, 1, 5, (0, 0, 50), (0, 0, 0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="1000,100000")
    a = ap.parse_args()
    import numpy as np
    import torch
    import sphere_update_expected as E
    from rt_amd import abi, gpu as G, scene as S
    shim = abi.load_shim()
    name = C.create_string_buffer(128)
    shim.rt_hip_device_info(0, name, 128, None)
    lines = [f"device: {name.value.decode()}",
             "spheres | update ms (device pointer) | first launch after it ms | destroy + create ms | first launch after it ms | recreate / update"]
    scenes = [S.build_scene(4, 48, 32, 1)] + [cloud_scene(n) for n in map(int, a.sizes.split(",")) if n]
    for sc in scenes:
        s0 = E.spheres_of(sc)
        moves = [torch.tensor(E.jitter(s0, seed=k), dtype=torch.float64, device="cuda") for k in range(2)]
        total = G.n_tiles(sc.width, sc.height)
        state = {"gs": G.GpuScene(sc), "k": 0}

        def launch():
            state["gs"].render_tiles(1666943821, 0, 1, total, samples=1)
            torch.cuda.synchronize()

        def update():
            state["k"] ^= 1
            state["gs"].update_spheres(moves[state["k"]])

        def recreate():
            state["gs"].close()
            state["gs"] = G.GpuScene(sc)

        launch()
        rows = {}
        for what, call in (("update", update), ("recreate", recreate)):
            ms, first = [], []
            call(), launch()   # warm-up
            for _ in range(7):
                t0 = time.perf_counter()
                call()
                t1 = time.perf_counter()
                launch()
                ms.append(1e3 * (t1 - t0))
                first.append(1e3 * (time.perf_counter() - t1))
            rows[what] = (statistics.median(ms), statistics.median(first))
        state["gs"].close()
        lines.append(f"{sc.n_objects} | {rows['update'][0]:.3f} | {rows['update'][1]:.3f} | {rows['recreate'][0]:.3f} | {rows['recreate'][1]:.3f} | "
                     f"x{rows['recreate'][0] / rows['update'][0]:.1f}")
        print(lines[-1], flush=True)
    # the previous points at 1080p: synthetic hits, half on spheres, half on triangles
    n, n_sph, n_tri = 1920 * 1080, 38, 12
    rng = np.random.default_rng(1)
    on_sphere = rng.random(n) < 0.5
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    hits = dict(status=dev(np.ones(n, np.int32)), prim=dev(np.where(on_sphere, -1, rng.integers(0, n_tri, n)).astype(np.int32)),
                object=dev(rng.integers(0, n_sph, n).astype(np.int32)), bary=dev(rng.uniform(0, 0.5, (n, 2))), point=dev(rng.uniform(-9, 9, (n, 3))))
    pos = dev(rng.uniform(-4, 4, (n_tri, 3, 3)))
    prev = dev(np.concatenate([rng.uniform(-9, 9, (n_sph, 3)), rng.uniform(1, 3, (n_sph, 1))], axis=1))
    cur = prev + 0.1
    out = torch.empty((n, 3), dtype=torch.float64, device="cuda")
    old = {f: hits[f] for f in ("status", "prim", "bary", "point")}
    for label, call in (("pt_prev_points", lambda: G.prev_points(old, pos, out=out)),
                        ("pt_prev_points_moved", lambda: G.prev_points_moved(hits, pos, prev, cur, out=out))):
        call()
        torch.cuda.synchronize()
        best = []
        for _ in range(20):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            call()
            ev[1].record()
            torch.cuda.synchronize()
            best.append(ev[0].elapsed_time(ev[1]))
        lines.append(f"{label:22s} 1920 x 1080: {min(best):.3f} ms (median {statistics.median(best):.3f})")
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
