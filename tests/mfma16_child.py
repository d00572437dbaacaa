#!/usr/bin/env python3
"""Child process of tests/test_gpu_mfma16.py: renders a fixed list of scenes with the shim that RT_HIP_SHIM_PATH names and prints one
JSON line per launch -- kernel, hashes of the float and the byte tiles, the four counters; with the PT_DIAG build (`diag`) also the
filter's violations, candidates and evaluations, the trips of the loop and those whose small spheres went through the matrix pipe.

The EDGE scenes (edge_scenes below) stand where the selection rule of the pooled body's prologue changes its answer -- near_R at 250,
the walls' count, the row range mf_first .. mf_first + 31, n_sph at 64 -- and away from config 4's operating point (scaled by 1/8,
the origin near a corner of the room).  Each states the n_big it means to have and, where it matters, the interval near_R must land
in; the child reads both back through the shim (rt_hip_scene_sphere_bounds, rt_hip_scene_bounds) and fails loudly when a scene misses
its edge.

usage: mfma16_child.py frames|diag"""
import hashlib
import json
import math
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


def _dicts(sc):
    return [dict(flags=int(o.flags), radius=float(o.radius), center=o.center.tuple(), color=o.color.tuple(), emission=o.emission.tuple())
            for o in (sc.objects[i] for i in range(sc.n_objects))]


def _reach(objs):
    """the scene's reach as the shim forms it (bvh_build.h, scene_sphere_reach_part): |c| (rounded up) + r over the spheres of ordinary size"""
    return max(math.sqrt(sum(x * x for x in o["center"])) * (1.0 + 1e-12) + o["radius"] for o in objs if o["radius"] < 1000)


def near_R_of(cam, objs):
    """rt_hip.h: near_R = 1.5 (|camera| + reach) + 1"""
    return 1.5 * (math.sqrt(sum(x * x for x in cam)) + _reach(objs)) + 1.0


def edge_scenes():
    """-> {name: dict(objs, cam, target, on, n_big, near_R (interval or None), kernel)}: `on` = the matrix pipe must run"""
    from rt_amd import abi
    from util import packed_room

    def room(n_packed):   # six walls, two lights, n_packed spheres
        sc = packed_room(n_packed, 3, 64, 64, 1, 16)
        objs = _dicts(sc)
        assert len(objs) == n_packed + 8 and all(o["radius"] >= 1000 for o in objs[:6]) and all(o["radius"] < 1000 for o in objs[6:])
        return objs

    def moved(objs, f=1.0, t=(0.0, 0.0, 0.0)):
        return [dict(o, radius=o["radius"] * f, center=tuple(x * f + y for x, y in zip(o["center"], t))) for o in objs]

    r32 = room(30)
    walls, small = r32[:6], r32[6:]
    cam, zero = (0.0, 0.0, 50.0), (0.0, 0.0, 0.0)
    out = {}

    def add(name, objs, on, n_big, cam=cam, target=zero, near_R=None, kernel="pt_render_tiles"):
        out[name] = dict(objs=objs, cam=cam, target=target, on=on, n_big=n_big, near_R=near_R, kernel=kernel)

    # 1 / 8 is the smallest power of two that leaves the walls (radius 1e4) wall-sized: at 1 / 16 they fall under 1000
    assert min(o["radius"] for o in walls) / 8 >= 1000 > max(o["radius"] for o in walls) / 16
    add("scaled 1/8", moved(r32, 1.0 / 8), True, 6, cam=(0.0, 0.0, 50.0 / 8))
    reach = _reach(r32)
    add("near_R under 250", r32, True, 6, cam=(0.0, 0.0, (248.75 - 1.0) / 1.5 - reach), near_R=(247.5, 250.0))
    add("near_R over 250", r32, False, 6, cam=(0.0, 0.0, (251.25 - 1.0) / 1.5 - reach), near_R=(250.0 + 1e-9, 252.5))
    # the origin one unit inside the room's left bottom back corner; the camera as far out on the room's axis as near_R = 249 allows
    half_w = 20.0 * 16 / 9
    t = (half_w - 1.0, 19.0, 29.0)
    corner = moved(r32, 1.0, t)
    far = (249.0 - 1.0) / 1.5 - _reach(corner)
    assert far > math.hypot(t[0], t[1]) + 5.0, "the translated room's reach leaves the camera no place within near_R <= 250"
    add("corner", corner, True, 6, cam=(t[0], t[1], min(t[2] + 50.0, math.sqrt(far * far - t[0] * t[0] - t[1] * t[1]))), target=t, near_R=(100.0, 250.0))
    add("no walls 32", small, True, 0)
    add("no walls 64", room(62)[6:], True, 0)
    add("no walls 31", room(29)[6:], False, 0)
    add("floor and ceiling", [w for w in walls if abs(w["center"][1]) > 1000] + small, True, 2)
    add("wall behind the rows", walls[:4] + small + walls[4:], True, 4)      # walls 4 and 5 at 36 and 37 = mf_first + 32, + 33
    add("64 spheres", room(56), True, 6)
    add("65 spheres", room(57), False, 6, kernel=None)
    add("five walls", walls[:5] + small, False, 4)                           # n_big counts whole pairs: the fifth wall is row 0
    big = dict(flags=abi.M_DEFAULT, radius=2000.0, center=(0.0, -2025.0, 0.0), color=(0.5, 0.5, 0.5), emission=(0.0, 0.0, 0.0))   # under the floor
    add("wall amid the rows", walls + small[:16] + [big] + small[16:], False, 6)
    # the 30 packed spheres replaced: the origin, the axes, signed zeros, a concentric pair, two identical spheres
    twins = [((0.0, 0.0, 0.0), 2.0), ((0.0, 0.0, 0.0), 1.0), ((12.0, 0.0, -0.0), 2.0), ((-12.0, -0.0, 0.0), 2.0), ((0.0, 10.0, 0.0), 1.5),
             ((-0.0, -10.0, 0.0), 1.5), ((0.0, 0.0, 20.0), 2.0), ((0.0, -0.0, -20.0), 2.0), ((20.0, 8.0, 5.0), 3.0), ((20.0, 8.0, 5.0), 3.0),
             ((-20.0, 8.0, 5.0), 3.0), ((-20.0, 8.0, 5.0), 1.0), ((2.0 ** -15, 15.0, 10.0), 1.0), ((25.0, 2.0 ** -20, -10.0), 2.0)]
    twins += [((-28.0 + 8.0 * (k % 8), -14.0 + 9.0 * (k // 8), -25.0 + 6.0 * (k % 5)), 1.0 + 0.25 * (k % 4)) for k in range(16)]
    add("axes and twins", walls + small[:2] + [dict(flags=abi.M_REFLECTION if k % 5 == 0 else abi.M_DEFAULT, radius=r, center=c, color=(0.9, 0.8, 0.7),
                                                    emission=(0.0, 0.0, 0.0)) for k, (c, r) in enumerate(twins)], True, 6)
    # the family's other member with MFMA_FILT (pt_kernel.hip, PT_FAMILY: SWAP && FILT_LDS && GEOM_LDS && !TRIS && !REFR holds for
    # pt_render_tiles and pt_render_tiles_chk alone): one packed sphere checkered
    add("32 small chk", [dict(o, flags=o["flags"] | (abi.M_CHECKERED if i == 9 else 0)) for i, o in enumerate(r32)], True, 6, kernel="pt_render_tiles_chk")
    return out


def edge_scene(name, samples):
    from rt_amd import scene as S
    e = edge_scenes()[name]
    return S.custom_scene(e["objs"], 64, 64, samples, 16, e["cam"], e["target"]), e


def check_edge(gs, e):
    """the scene stands on the edge it was built for: n_big and near_R read back through the shim"""
    nb, reach = gs.sphere_bounds()["n_big"], gs.bounds()["reach"]
    assert nb == e["n_big"], (nb, e["n_big"])
    assert abs(reach - _reach(e["objs"])) <= 1e-9 * reach, (reach, _reach(e["objs"]))
    near_R = 1.5 * (math.sqrt(sum(x * x for x in e["cam"])) + reach) + 1.0
    if e["near_R"]:
        assert e["near_R"][0] <= near_R <= e["near_R"][1], (near_R, e["near_R"])
    else:
        assert near_R <= 250.0
    return near_R


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
    edges = [(name, *edge_scene(name, 4 if mode == "diag" else 8)) for name in edge_scenes()]
    for name, sc, first, stride, count, e in [(*c, None) for c in cases(mode)] + [(name, sc, 0, 1, None, e) for name, sc, e in edges]:
        gs = G.GpuScene(sc)
        count = G.n_tiles(sc.width, sc.height) if count is None else count
        stats = torch.zeros(48, dtype=torch.int64, device="cuda")
        tiles, tiles8, stats = gs.render_tiles(SEED, first, stride, count, stats=stats)
        torch.cuda.synchronize()
        st = stats.cpu().tolist()
        rec = {"scene": name, "kernel": gs.last_launch_kernel(), "n": sc.n_primitives,
               "tiles": hashlib.sha256(tiles.cpu().numpy().tobytes()).hexdigest(),
               "tiles8": hashlib.sha256(tiles8.cpu().numpy().tobytes()).hexdigest(), "counters": st[:4]}
        if e is not None:
            rec.update(near_R=check_edge(gs, e), n_big=e["n_big"])
            assert e["kernel"] is None or rec["kernel"] == e["kernel"], rec
        if mode == "diag":
            rec.update(violations=st[4 + 12], candidates=st[4 + 3], filter_evals=st[4 + 39], trips=st[4 + 0], matrix_trips=st[4 + 4])
        print(json.dumps(rec), flush=True)
        gs.close()


if __name__ == "__main__":
    main()
