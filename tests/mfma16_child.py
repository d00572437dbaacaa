#!/usr/bin/env python3
"""Child process of tests/test_gpu_mfma16.py: renders a fixed list of scenes with the shim that RT_HIP_SHIM_PATH names and prints one
JSON line per launch -- kernel, hashes of the float and the byte tiles, the four counters; with the PT_DIAG build (`diag`) also the
filter's violations, candidates and evaluations, the trips of the loop and those whose small spheres went through the matrix pipe.

usage: mfma16_child.py frames|diag"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "raytracer.c_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

SEED = 1666943821


def room_objects(width, height):
    """config 4's six walls and two lights, as dicts"""
    from rt_amd import scene as S
    room = S.build_scene(4, width, height, 1)
    objs = [dict(flags=int(o.flags), radius=float(o.radius), center=o.center.tuple(), color=o.color.tuple(), emission=o.emission.tuple())
            for o in (room.objects[i] for i in range(8))]
    room.free()
    assert all(o["radius"] >= 1000 for o in objs[:6]) and all(o["radius"] < 1000 for o in objs[6:])
    return objs


def tiny_grid(width, height, samples):
    """32 spheres of radius 1e-3 on a 4 x 4 x 2 grid (with the two lights: 34 small spheres)"""
    from rt_amd import abi, scene as S
    objs = room_objects(width, height)
    for k in range(32):
        c = (-15.0 + 10.0 * (k % 4), -12.0 + 8.0 * ((k // 4) % 4), -10.0 + 20.0 * (k // 16))
        objs.append(dict(flags=abi.M_DEFAULT, radius=1e-3, center=c, color=(1.0, 1.0, 1.0), emission=(0.0, 0.0, 0.0)))
    return S.custom_scene(objs, width, height, samples, 16, (0, 0, 50), (0, 0, 0))


def tangent_room(width, height, samples):
    """32 spheres each tangent to a wall (floor, ceiling, left, right, back in turn), mirrors among them"""
    from rt_amd import abi, scene as S
    objs = room_objects(width, height)
    half_w = 20.0 * width / height
    for k in range(32):
        r = 1.0 + 0.25 * (k % 5)
        u, v = -0.8 + 1.6 * ((k * 7) % 11) / 10.0, -0.8 + 1.6 * ((k * 3) % 13) / 12.0
        c = [(u * half_w, -20.0 + r, v * 25.0), (u * half_w, 20.0 - r, v * 25.0), (-half_w + r, u * 18.0, v * 25.0),
             (half_w - r, u * 18.0, v * 25.0), (u * half_w, v * 18.0, -30.0 + r)][k % 5]
        objs.append(dict(flags=abi.M_REFLECTION if k % 4 == 0 else abi.M_DEFAULT, radius=r, center=c, color=(0.9, 0.9, 0.9),
                         emission=(0.0, 0.0, 0.0)))
    return S.custom_scene(objs, width, height, samples, 16, (0, 0, 50), (0, 0, 0))


def cases(mode):
    from rt_amd import scene as S
    from util import packed_room
    if mode == "diag":   # 64 x 64 x 4 spp, depth 16
        return [("config 4", S.build_scene(4, 64, 64, 4), 0, 1, None), ("tiny grid", tiny_grid(64, 64, 4), 0, 1, None),
                ("tangent", tangent_room(64, 64, 4), 0, 1, None)] + \
               [(f"{n + 2} small", packed_room(n, 3, 64, 64, 4, 16), 0, 1, None) for n in (29, 30, 31, 36)]
    out = []
    # 29, 30, 31, 36 packed spheres + 2 lights = 31, 32, 33, 38 small spheres behind the six walls: one short of the matrix tile,
    # exactly one, one and six past it (those go through the packed loop behind the tile)
    for n in (29, 30, 31, 36):
        out.append((f"{n + 2} small 64x64", packed_room(n, 3, 64, 64, 8, 16), 0, 1, None))
        out.append((f"{n + 2} small 70x35", packed_room(n, 3, 70, 35, 8, 16), 0, 1, None))
        out.append((f"{n + 2} small 64x64 subset", packed_room(n, 3, 64, 64, 8, 16), 3, 5, 10))
    out.append(("config 4 64x64", S.build_scene(4, 64, 64, 8), 0, 1, None))
    out.append(("tiny grid", tiny_grid(64, 64, 8), 0, 1, None))
    out.append(("tangent", tangent_room(70, 35, 8), 0, 1, None))
    return out


def main():
    mode = sys.argv[1]
    import torch
    from rt_amd import gpu as G
    for name, sc, first, stride, count in cases(mode):
        gs = G.GpuScene(sc)
        count = G.n_tiles(sc.width, sc.height) if count is None else count
        stats = torch.zeros(48, dtype=torch.int64, device="cuda")
        tiles, tiles8, stats = gs.render_tiles(SEED, first, stride, count, stats=stats)
        torch.cuda.synchronize()
        st = stats.cpu().tolist()
        rec = {"scene": name, "kernel": gs.last_launch_kernel(), "n": sc.n_primitives,
               "tiles": hashlib.sha256(tiles.cpu().numpy().tobytes()).hexdigest(),
               "tiles8": hashlib.sha256(tiles8.cpu().numpy().tobytes()).hexdigest(), "counters": st[:4]}
        if mode == "diag":
            rec.update(violations=st[4 + 12], candidates=st[4 + 3], filter_evals=st[4 + 39], trips=st[4 + 0], matrix_trips=st[4 + 4])
        print(json.dumps(rec), flush=True)
        gs.close()


if __name__ == "__main__":
    main()
