#!/usr/bin/env python3
"""What reprojection across a vertex update costs per frame (rt_hip_prev_points, rt_hip_reproject_points) next to the static form
(rt_hip_reproject), on config 5's mesh under scale-and-wobble (tests/scene_update_meshes.py), at 1920x1080 and 3840x2160, 1 spp:
  pt_reproject            with and without bytes, as tools/reproject_bench.py times it: the yardstick
  pt_reproject_points     the same call with the previous points
  pt_prev_points          the blend of the previous corners
  query                   the pixel-centre RT_HIP_RAYS_CAMERA_UV query (status, prim, bary, point)
Each by HIP events, best of `reps` after a warm-up; the timed runs alternate in one process.  The added cost of a moving frame is
query + points + (pt_reproject_points - pt_reproject).
usage: python tools/reproject_moving_bench.py [--reps=R (5)] [--out=FILE]"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "raytracer.c_amd"), os.path.join(ROOT, "tests")]
import numpy as np
import torch
import scene_update_meshes as U
from rt_amd import gpu as G, scene as S

SEED = 1666943821
opt = {a.split("=")[0]: (a.split("=") + [""])[1] for a in sys.argv[1:] if a.startswith("--")}
reps = int(opt.get("--reps") or 5)


def tris_of(sc):
    v = np.ctypeslib.as_array(C.cast(sc.meshes[0].mesh.vertices, C.POINTER(C.c_double)), shape=(3 * sc.n_triangles, 5))
    return v[:, :3].reshape(-1, 3, 3).copy()


def frame(gs, seed):
    total = G.n_tiles(gs.scene.width, gs.scene.height)
    tiles, tiles8, _ = gs.render_tiles(seed, 0, 1, total, samples=1, chunks=gs.suggest_chunks(total, 1))
    image, _ = gs.untile(tiles, tiles8, 0, 1, total)
    aov = gs.untile_aov(gs.render_aov(seed, 1, 0, 1, total, want=G.DENOISE_AOV), 0, 1, total)
    torch.cuda.synchronize()
    return image, aov


def timed(call):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    call()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    lines = []
    for w, h in ((1920, 1080), (3840, 2160)):
        sc = S.build_scene(5, w, h, 1)
        gs = G.GpuScene(sc, bvh="device")
        cam = sc.camera
        tris = tris_of(sc)
        poses = [torch.tensor(U.scale_wobble(tris, phase=0.3 * k), dtype=torch.float64, device="cuda") for k in (0, 1)]
        gs.update_vertices(poses[0])
        prev, prev_aov = frame(gs, SEED)
        gs.update_vertices(poses[1])
        cur, cur_aov = frame(gs, SEED + 1)
        hist = dict(rgb=prev, len=torch.full((h, w), 3.0, device=prev.device), aov=prev_aov, camera=cam)
        ys, xs = np.mgrid[0:h, 0:w]
        uv = torch.tensor(np.stack([(xs + 0.5) / (w - 1.0), (ys + 0.5) / (h - 1.0)], axis=-1).reshape(-1, 2), device="cuda")
        want = ("status", "prim", "bary", "point")
        hits = gs.query_uv(uv, want=want)
        pts = G.prev_points(hits, poses[0])
        out, out_p = G.reproject(cur, cur_aov, cam, hist=hist), G.reproject(cur, cur_aov, cam, hist=hist, prev_points=pts)
        runs = {
            "pt_reproject with bytes": lambda: G.reproject(cur, cur_aov, cam, hist=hist, out=out),
            "pt_reproject without bytes": lambda: G.reproject(cur, cur_aov, cam, hist=hist, out=dict(out, rgb8=None)),
            "pt_reproject_points with bytes": lambda: G.reproject(cur, cur_aov, cam, hist=hist, out=out_p, prev_points=pts),
            "pt_reproject_points without bytes": lambda: G.reproject(cur, cur_aov, cam, hist=hist, out=dict(out_p, rgb8=None), prev_points=pts),
            "pt_prev_points": lambda: G.prev_points(hits, poses[0], out=pts),
            "pixel-centre query": lambda: gs.query_uv(uv, want=want, out=hits),
        }
        best = {}
        for k in range(reps + 1):
            for name, call in runs.items():      # alternating: every round times each run once
                t = timed(call)
                if k:
                    best[name] = min(best.get(name, t), t)
        on_mesh = float((hits["prim"] != -1).float().mean())
        blend, blend_p = float((out["len"] > 1).float().mean()), float((out_p["len"] > 1).float().mean())
        lines.append(f"{w}x{h}, config 5 ({sc.n_triangles} triangles) between wobble phases 0 and 0.3; {on_mesh:.3f} of the pixels on the mesh; "
                     f"history taken on {blend:.3f} of the frame by the static form, {blend_p:.3f} with the previous points")
        for name, t in best.items():
            lines.append(f"  {name:36s} {t:7.3f} ms  ({w * h / t * 1e-6:6.2f} Gpixel/s)")
        added = best["pixel-centre query"] + best["pt_prev_points"] + best["pt_reproject_points with bytes"] - best["pt_reproject with bytes"]
        lines.append(f"  added cost of a moving frame: query + points + (points form - static form) = {added:.3f} ms")
        gs.close()
        sc.free()
    text = "\n".join(lines)
    print(text)
    if opt.get("--out"):
        open(opt["--out"], "w").write(text + "\n")


if __name__ == "__main__":
    main()
