"""The scenes of tests/test_gpu_dir_park.py, in a plain module: its child process (tests/dir_park_child.py) builds them too,
without pytest."""


def room_tile():
    """config 4's scene, one full tile, 16 spp, depth 16"""
    from rt_amd import scene as S
    sc = S.build_scene(4, 8, 8, 16)
    assert sc.max_depth == 16
    return sc


def room_ragged():
    """config 4's scene at 13 x 9: tiles of 8 x 8, 5 x 8, 8 x 1 and 5 x 1 pixels"""
    from rt_amd import scene as S
    return S.build_scene(4, 13, 9, 32)


def _diffuse_objs():
    """the ten spheres of the all-diffuse room: six walls, three balls, the light"""
    from rt_amd import abi
    R, d = 1e4, 12.0
    white = (0.99, 0.97, 0.95)
    objs = [dict(flags=abi.M_DEFAULT, radius=R, center=c, color=white) for c in
            ((0, -(R + d), 0), (0, R + d, 0), (-(R + d), 0, 0), (R + d, 0, 0), (0, 0, -(R + d)), (0, 0, R + 40.0))]
    objs += [dict(flags=abi.M_DEFAULT, radius=3.0, center=(-4, -9, -3), color=(0.99, 0.6, 0.5)),
             dict(flags=abi.M_DEFAULT, radius=2.0, center=(5, -10, 2), color=(0.5, 0.7, 0.99)),
             dict(flags=abi.M_DEFAULT, radius=4.0, center=(1, -8, -7), color=white),
             dict(flags=abi.M_DEFAULT, radius=1.0, center=(0, 10.5, 0), color=(1, 1, 1), emission=(12, 12, 12))]
    return objs


def diffuse_room():
    """every surface diffuse with a roulette probability (the albedo's largest channel) of 0.99: a closed room of six wall-sized
    spheres and three balls, lit by a small ball under the ceiling; an 8 x 8 tile at 64 spp, depth 16.  Nearly every lane wants a
    direction in every trip."""
    from rt_amd import scene as S
    return S.custom_scene(_diffuse_objs(), 8, 8, 64, 16, (0, 0, 30), (0, -3, 0))


def _box(lo, hi):
    """the twelve triangles of an axis-aligned box, texture coordinates from the face's own two axes"""
    tris = []
    for ax in range(3):
        u, v = (ax + 1) % 3, (ax + 2) % 3
        for side in (lo, hi):
            def p(a, b):
                q = [0.0, 0.0, 0.0]
                q[ax], q[u], q[v] = side[ax], (lo[u], hi[u])[a], (lo[v], hi[v])[b]
                return tuple(q) + (float(a), float(b))
            tris += [[p(0, 0), p(1, 0), p(1, 1)], [p(0, 0), p(1, 1), p(0, 1)]]
    return tris


def park_room(chk=False, wide=False, small=0, mesh=None, glass_ball=False, width=8, height=8, samples=64, max_depth=16):
    """diffuse_room() plus what moves it to another row of the kernel pick table, and nothing else:
    chk: M_CHECKERED on the floor wall and on the first ball; wide: a diffuse floor sphere of radius 1e19 (in fp64 its centre
    is (0, -1e19, 0) whatever is added to it, so its top lies at y = 0, through the middle of the room: 12 above the room's own
    floor); small: that many diffuse spheres of radius 0.45 on a grid in the room's upper half, clear of the balls and the light;
    mesh: "diffuse", "checkered" or "glass": a floating box of twelve triangles; glass_ball: the largest ball M_REFRACTION"""
    from rt_amd import abi, scene as S
    objs = _diffuse_objs()
    if chk:
        objs[0]["flags"] |= abi.M_CHECKERED
        objs[6]["flags"] |= abi.M_CHECKERED
    if glass_ball:
        objs[8]["flags"] = abi.M_REFRACTION
        objs[8]["color"] = (0.95, 0.95, 0.95)
    if small:
        nx, ny, nz = {120: (6, 4, 5), 300: (10, 5, 6)}[small]
        for i in range(nx):
            for j in range(ny):
                for k in range(nz):
                    c = (-10.5 + 21.0 * i / (nx - 1), -2.0 + 10.0 * j / (ny - 1), -10.0 + 20.0 * k / (nz - 1))
                    objs.append(dict(flags=abi.M_DEFAULT, radius=0.45, center=c, color=(0.99, 0.99, 0.99)))
    if wide:
        objs.append(dict(flags=abi.M_DEFAULT, radius=1e19, center=(0.0, -1e19, 0.0), color=(0.99, 0.98, 0.9)))
    meshes = []
    if mesh:
        flags = {"diffuse": abi.M_DEFAULT, "checkered": abi.M_DEFAULT | abi.M_CHECKERED, "glass": abi.M_REFRACTION}[mesh]
        meshes = [dict(flags=flags, color=(0.95, 0.95, 0.95) if mesh == "glass" else (0.99, 0.9, 0.7),
                       triangles=_box((4.0, -6.0, 1.0), (8.0, -2.0, 5.0)))]
    return S.custom_scene(objs, width, height, samples, max_depth, (0, 0, 30), (0, -3, 0), meshes=meshes)


# one deep-path, all-diffuse (but for the glass the row asks for) scene per swapping pooled kernel: (scene name, kernel, what
# park_room adds).  One 8 x 8 tile at 64 spp and depth 16 is 4,096 jobs for four waves: every wave swaps with live paths on its
# list, and nearly every lane wants a direction in every trip.
PARK_ROWS = [
    ("diffuse_room", "pt_render_tiles", dict()),
    ("dr_chk", "pt_render_tiles_chk", dict(chk=True)),
    ("dr_big", "pt_render_tiles_big", dict(wide=True)),
    ("dr_big_chk", "pt_render_tiles_big_chk", dict(wide=True, chk=True)),
    ("dr_tri", "pt_render_tiles_tri", dict(mesh="diffuse")),
    ("dr_tri_chk", "pt_render_tiles_tri_chk", dict(mesh="checkered", chk=True)),
    ("dr_mem_s", "pt_render_tiles_pool_mem_s", dict(small=120)),
    ("dr_mem_s_chk", "pt_render_tiles_pool_mem_s_chk", dict(small=120, chk=True)),
    ("dr_mem", "pt_render_tiles_pool_mem", dict(small=300, wide=True)),
    ("dr_mem_chk", "pt_render_tiles_pool_mem_chk", dict(small=300, wide=True, chk=True)),
    ("dr_refr", "pt_render_tiles_refr_pool", dict(glass_ball=True)),
    ("dr_refr_mem", "pt_render_tiles_refr_pool_mem", dict(glass_ball=True, small=120)),
    ("dr_tri_refr", "pt_render_tiles_tri_refr_pool", dict(mesh="glass")),
]
PARK_SCENES = [r[0] for r in PARK_ROWS]
REFR_SCENES = [r[0] for r in PARK_ROWS if "refr" in r[1]]
# the all-diffuse room of the same row without its glass (the glass scenes' ray count is held against it)
NO_GLASS = {"dr_refr": "diffuse_room", "dr_refr_mem": "dr_mem_s", "dr_tri_refr": "dr_tri"}
# the M_REFRACTION entry's depth field past bit 3: the glass room at 32 spp and the largest max_depth <= 28 at which the launch
# stays on pt_render_tiles_refr_pool and a sample chunk (GpuScene.suggest_chunks) keeps 8 samples, two batches a wave -- taken
# from the shim's answers on the MI355X (tests/test_gpu_dir_park.py asserts them)
DEEP_GLASS_DEPTH = 26


def deep_glass_room(max_depth=DEEP_GLASS_DEPTH):
    return park_room(glass_ball=True, samples=32, max_depth=max_depth)


def ragged_chk():
    """the checkered room at 13 x 9: tiles of 8 x 8, 5 x 8, 8 x 1 and 5 x 1 pixels"""
    return park_room(chk=True, width=13, height=9)


def ragged_refr():
    return park_room(glass_ball=True, width=13, height=9)


def passes_refr():
    return park_room(glass_ball=True, samples=16)


def passes_mem_s():
    return park_room(small=120, samples=16)


def config2_small():
    from rt_amd import scene as S
    return S.build_scene(2, 16, 16, 8)


def config3_small():
    from rt_amd import scene as S
    return S.build_scene(3, 16, 16, 8)


def checkered_balls():
    """diffuse checkered spheres over a checkered floor, a mirror, a light: no glass"""
    from rt_amd import abi, scene as S
    objs = [dict(flags=abi.M_DEFAULT | abi.M_CHECKERED, radius=10000.0, center=(0, -10005.0, 0), color=(0.8, 0.8, 0.8)),
            dict(flags=abi.M_DEFAULT | abi.M_CHECKERED, radius=4.0, center=(-6, -1, 0), color=(0.9, 0.5, 0.3)),
            dict(flags=abi.M_DEFAULT, radius=3.0, center=(4, -2, 3), color=(0.4, 0.8, 0.9)),
            dict(flags=abi.M_REFLECTION, radius=3.0, center=(9, -2, -6), color=(1, 1, 1)),
            dict(flags=abi.M_DEFAULT, radius=6.0, center=(-2, 18, 4), color=(1, 1, 1), emission=(5, 5, 5))]
    return S.custom_scene(objs, 16, 16, 16, 8, (0, 5, 32), (0, 0, 0))


def glass_small():
    from util import glass_scene
    return glass_scene(16, 16, 12)


SCENES = {"room_tile": room_tile, "room_ragged": room_ragged, "diffuse_room": diffuse_room, "config2": config2_small,
          "config3": config3_small, "checkered": checkered_balls, "glass": glass_small, "deep_glass": deep_glass_room,
          "ragged_chk": ragged_chk, "ragged_refr": ragged_refr, "passes_refr": passes_refr, "passes_mem_s": passes_mem_s}
SCENES.update({name: (lambda kw=kw: park_room(**kw)) for name, _, kw in PARK_ROWS[1:]})
# the swapping pooled kernel each of them is there for
KERNELS = {"room_tile": "pt_render_tiles", "room_ragged": "pt_render_tiles", "diffuse_room": "pt_render_tiles",
           "config2": "pt_render_tiles", "config3": "pt_render_tiles_tri", "checkered": "pt_render_tiles_chk",
           "glass": "pt_render_tiles_refr_pool", "deep_glass": "pt_render_tiles_refr_pool", "ragged_chk": "pt_render_tiles_chk",
           "ragged_refr": "pt_render_tiles_refr_pool", "passes_refr": "pt_render_tiles_refr_pool",
           "passes_mem_s": "pt_render_tiles_pool_mem_s"}
KERNELS.update({name: kernel for name, kernel, _ in PARK_ROWS})
