#!/usr/bin/env python3
"""Child process of tests/test_gpu_sphere_update.py: the n_packed=33 and n_packed=4 rooms of util.class_scene, their spheres moved
IN PLACE (GpuScene.update_spheres) by the jitter (b) and by the shrunken wall (d) of tests/sphere_update_expected.py, then one frame
each through the PT_DIAG build of the shim (RT_HIP_SHIM_PATH=.../librt_hip_diag.so, RT_HIP_DIAG_WALK_REJECTED=1), and one JSON line
per frame with the counters the conservative rules are judged by (tests/diag_child.py explains them): violations must be 0 on the
rebuilt filter tables, the matrix-pipe filter of the 32 small spheres and the pruning among the leading walls."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "raytracer.c_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def main():
    if "diag" not in os.path.basename(os.environ.get("RT_HIP_SHIM_PATH", "")):
        raise SystemExit("run with RT_HIP_SHIM_PATH=<...>/librt_hip_diag.so (the PT_DIAG build)")
    os.environ["RT_HIP_DIAG_WALK_REJECTED"] = "1"   # read by the shim at every launch
    import torch
    import sphere_update_expected as E
    from rt_amd import gpu as G
    from util import class_scene
    for n_packed in (33, 4):
        sc = class_scene(n_packed=n_packed)
        s0 = E.spheres_of(sc)
        gs = G.GpuScene(sc)
        total = G.n_tiles(sc.width, sc.height)
        gs.render_tiles(1666943821, 0, 1, total)         # a frame before: the table sets exist and are then left stale
        torch.cuda.synchronize()
        for k, move in enumerate(("jitter", "wall_shrunk")):
            gs.update_spheres(torch.tensor(E.MOVES[move](s0), dtype=torch.float64, device="cuda"))
            stats = torch.zeros(48, dtype=torch.int64, device="cuda")
            gs.render_tiles(1666943821, 0, 1, total, stats=stats, chunks=gs.suggest_chunks(total))
            torch.cuda.synchronize()
            st = stats.cpu().tolist()
            d = st[4:]
            print(json.dumps({"n_packed": n_packed, "move": move, "updates": gs.update_info()["updates"], "kernel": gs.last_launch_kernel(),
                              "n_big": gs.sphere_bounds()["n_big"], "casts": st[1], "violations": d[12], "candidates": d[3],
                              "filter_evals": d[39], "walls_pruned": d[37]}), flush=True)
        gs.close()
        sc.free()


if __name__ == "__main__":
    main()
