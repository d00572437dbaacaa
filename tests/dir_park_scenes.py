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


def diffuse_room():
    """every surface diffuse with a roulette probability (the albedo's largest channel) of 0.99: a closed room of six wall-sized
    spheres and three balls, lit by a small ball under the ceiling; an 8 x 8 tile at 64 spp, depth 16.  Nearly every lane wants a
    direction in every trip."""
    from rt_amd import abi, scene as S
    R, d = 1e4, 12.0
    white = (0.99, 0.97, 0.95)
    objs = [dict(flags=abi.M_DEFAULT, radius=R, center=c, color=white) for c in
            ((0, -(R + d), 0), (0, R + d, 0), (-(R + d), 0, 0), (R + d, 0, 0), (0, 0, -(R + d)), (0, 0, R + 40.0))]
    objs += [dict(flags=abi.M_DEFAULT, radius=3.0, center=(-4, -9, -3), color=(0.99, 0.6, 0.5)),
             dict(flags=abi.M_DEFAULT, radius=2.0, center=(5, -10, 2), color=(0.5, 0.7, 0.99)),
             dict(flags=abi.M_DEFAULT, radius=4.0, center=(1, -8, -7), color=white),
             dict(flags=abi.M_DEFAULT, radius=1.0, center=(0, 10.5, 0), color=(1, 1, 1), emission=(12, 12, 12))]
    return S.custom_scene(objs, 8, 8, 64, 16, (0, 0, 30), (0, -3, 0))


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
          "config3": config3_small, "checkered": checkered_balls, "glass": glass_small}
# the swapping pooled kernel each of them is there for
KERNELS = {"room_tile": "pt_render_tiles", "room_ragged": "pt_render_tiles", "diffuse_room": "pt_render_tiles",
           "config2": "pt_render_tiles", "config3": "pt_render_tiles_tri", "checkered": "pt_render_tiles_chk",
           "glass": "pt_render_tiles_refr_pool"}
