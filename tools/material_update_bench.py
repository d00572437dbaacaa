#!/usr/bin/env python3
"""What editing a scene's materials in place costs (GpuScene.update_materials, rt_hip_scene_update_materials) against destroying
the scene and creating it again from the same data, at 38 (config 4), 1,000 and 100,000 spheres and on config 5's mesh:
  update ms        the synchronous call of the shim's entry itself -- rt_hip_scene_update_materials on a prepared (n, 6) device
                   tensor and int32 flags, rt_hip_scene_update_materials_host on numpy arrays; GpuScene.update_materials' own
                   concatenation, stream wait and clones are NOT in it --, after one warm-up, median of 9: device events on the
                   null stream around the call, and the host's clock next to them
  recreate ms      close + rt_hip_scene_create of the same scene, the same two clocks
  first launch ms  the first frame after each (48 x 32, 1 spp; the host's clock around launch and synchronize): the table sets stay
                   valid after a material update, and are built for the first time after a recreate
usage: python tools/material_update_bench.py [--out FILE] [--sizes 1000,100000] [--no-mesh]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "raytracer.c_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="1000,100000")
    ap.add_argument("--no-mesh", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch
    import material_expected as E
    from sphere_update_bench import cloud_scene
    from rt_amd import abi, gpu as G, scene as S
    shim = abi.load_shim()
    name = C.create_string_buffer(128)
    shim.rt_hip_device_info(0, name, 128, None)
    lines = [f"device: {name.value.decode()}",
             "scene | form | update ms (device events) | update ms (host clock) | first launch after it ms | destroy + create ms (device events) "
             "| (host clock) | first launch after it ms | recreate / update (host clock)"]
    scenes = [("38 spheres", S.build_scene(4, 48, 32, 1))] + [(f"{n} spheres", cloud_scene(n)) for n in map(int, a.sizes.split(",")) if n]
    if not a.no_mesh:
        scenes.append(("config 5's mesh", S.build_scene(5, 48, 32, 1)))
    for label, sc in scenes:
        c0, e0, f0 = E.materials_of(sc)
        edits = []
        for k in range(2):   # two sets of materials to alternate between: every colour and emission scaled, the flags as they are
            m = np.ascontiguousarray(np.concatenate([c0 * (0.5 + 0.25 * k), e0 * (1.0 + k)], axis=1))
            edits.append(dict(host=(m, f0), device=(torch.tensor(m, device="cuda"), torch.tensor(f0.astype(np.int32), device="cuda"))))
        n = len(c0)
        total = G.n_tiles(sc.width, sc.height)
        state = {"gs": G.GpuScene(sc), "k": 0}

        def launch():
            state["gs"].render_tiles(1666943821, 0, 1, total, samples=1)
            torch.cuda.synchronize()

        def recreate():
            state["gs"].close()
            state["gs"] = G.GpuScene(sc)

        def update(form):
            state["k"] ^= 1
            m, f = edits[state["k"]][form]
            if form == "device":
                rc = shim.rt_hip_scene_update_materials(state["gs"].handle, C.c_void_p(m.data_ptr()), C.c_void_p(f.data_ptr()), n)
            else:
                rc = shim.rt_hip_scene_update_materials_host(state["gs"].handle, m.ctypes.data, f.ctypes.data, n)
            assert rc == 0, shim.rt_hip_last_error()

        launch()
        rows = {}
        for what, call in (("device", lambda: update("device")), ("host", lambda: update("host")), ("recreate", recreate)):
            dev_ms, host_ms, first = [], [], []
            call(), launch()   # warm-up
            for _ in range(9):
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ev[0].record()
                call()
                ev[1].record()
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                launch()
                first.append(1e3 * (time.perf_counter() - t1))
                host_ms.append(1e3 * (t1 - t0))
                dev_ms.append(ev[0].elapsed_time(ev[1]))
            rows[what] = tuple(statistics.median(x) for x in (dev_ms, host_ms, first))
        state["gs"].close()
        r = rows["recreate"]
        for form in ("device", "host"):
            u = rows[form]
            lines.append(f"{label} | {form} | {u[0]:.3f} | {u[1]:.3f} | {u[2]:.3f} | {r[0]:.3f} | {r[1]:.3f} | {r[2]:.3f} | x{r[1] / u[1]:.1f}")
            print(lines[-1], flush=True)
        sc.free()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
