#!/usr/bin/env python3
"""Child process of tests/test_gpu_scene_update.py: config 5's 10,240-triangle sphere, scaled and wobbled IN PLACE
(GpuScene.update_vertices on a device-built tree), then one frame through the PT_DIAG build of the shim
(RT_HIP_SHIM_PATH=.../librt_hip_diag.so, RT_HIP_DIAG_WALK_REJECTED=1), and one JSON line with the counters the conservative rules
are judged by (tests/diag_child.py explains them): violations must be 0 on the refitted tree and the rebuilt tables."""
import ctypes as C
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
    import numpy as np
    import torch
    import scene_update_meshes as U
    from rt_amd import gpu as G
    from rt_amd import scene as S
    sc = S.build_scene(5, 192, 108, 4)
    assert sc.n_triangles == 10240 and sc.n_meshes == 1
    v = np.ctypeslib.as_array(C.cast(sc.meshes[0].mesh.vertices, C.POINTER(C.c_double)), shape=(3 * sc.n_triangles, 5))
    tris = v[:, :3].reshape(-1, 3, 3).copy()
    gs = G.GpuScene(sc, bvh="device")
    total = G.n_tiles(sc.width, sc.height)
    gs.render_tiles(1666943821, 0, 1, total)         # a frame before: the table sets exist and are then left stale
    torch.cuda.synchronize()
    gs.update_vertices(torch.tensor(U.scale_wobble(tris), dtype=torch.float64, device="cuda"))
    stats = torch.zeros(48, dtype=torch.int64, device="cuda")
    gs.render_tiles(1666943821, 0, 1, total, stats=stats)
    torch.cuda.synchronize()
    st = stats.cpu().tolist()
    d = st[4:]
    print(json.dumps({"updates": gs.update_info()["updates"], "kernel": gs.last_launch_kernel(), "casts": st[1], "violations": d[12],
                      "parked": d[17], "leaf_pretests": d[16], "walked_found_triangle": d[18]}), flush=True)
    gs.close()


if __name__ == "__main__":
    main()
