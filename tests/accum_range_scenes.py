"""The scenes at the edges of what the library accepts (rt_hip_shim.hip: material_ok -- colours in [0, 1e100], |emission| <=
1e100), shared by tests/test_gpu_sum_range.py (one-shot launches), tests/test_gpu_accum_range.py (accumulations) and
tests/test_gpu_trace_range.py (radiance queries and pixel refinement); tests/test_accum_range_cpu.py shows without a GPU that
they reach what they claim.  Importable without a GPU: scenes, the restated sum rules of pt_device.h, ray and pixel lists.
"""
import math

import numpy as np

from util import acc_scale_exp, class_scene

SHELL_C = (-12.0, 8.0, -10.0)  # a diffuse shell in the room's upper left, away from the camera (0, 0, 50)
VISIBLE_C, VISIBLE_R = (6.0, -4.0, 10.0), 1.5   # the small emitter in view


def _parts(sc):
    """the objects and meshes of a scene as custom_scene() takes them"""
    objs = [dict(flags=int(o.flags), radius=float(o.radius), center=o.center.tuple(), color=o.color.tuple(),
                 emission=o.emission.tuple()) for o in (sc.objects[i] for i in range(sc.n_objects))]
    meshes = []
    for i in range(sc.n_meshes):
        m = sc.meshes[i]
        v = m.mesh.vertices
        tris = [[(v[3 * t + k].pos.x, v[3 * t + k].pos.y, v[3 * t + k].pos.z, v[3 * t + k].tex.x, v[3 * t + k].tex.y)
                 for k in range(3)] for t in range(m.mesh.num_triangles)]
        meshes.append(dict(flags=int(m.flags), color=m.color.tuple(), emission=m.emission.tuple(), triangles=tris))
    return objs, meshes


def _custom(objs, meshes, width, height, samples, max_depth):
    from rt_amd import scene as S
    return S.custom_scene(objs, width, height, samples, max_depth, (0, 0, 50), (0, 0, 0), meshes=meshes)


def hidden_emitter_scene(E, width=40, height=24, samples=4, max_depth=5, **cls):
    """class_scene(**cls) plus an emitter of E sealed inside a closed diffuse shell: no ray can reach it"""
    objs, meshes = _parts(class_scene(width=width, height=height, samples=samples, depth=max_depth, **cls))
    from rt_amd import abi
    objs.append(dict(flags=abi.M_DEFAULT, radius=3.0, center=SHELL_C, color=(0.6, 0.6, 0.6)))
    objs.append(dict(flags=abi.M_DEFAULT, radius=1.0, center=SHELL_C, color=(1.0, 1.0, 1.0), emission=(E, E, E)))
    return _custom(objs, meshes, width, height, samples, max_depth)


def without_last_emitter(sc):
    """the scene with its last object's emission switched off (the hidden emitter of hidden_emitter_scene: the premise check)"""
    objs, meshes = _parts(sc)
    objs[-1]["emission"] = (0.0, 0.0, 0.0)
    return _custom(objs, meshes, sc.width, sc.height, sc.samples, sc.max_depth)


def visible_emitter_object(E):
    from rt_amd import abi
    return dict(flags=abi.M_DEFAULT, radius=VISIBLE_R, center=VISIBLE_C, color=(1.0, 1.0, 1.0), emission=(E, 0.3 * E, 1.0))


def visible_emitter_scene(E, width=40, height=24, samples=4, max_depth=5, **cls):
    """a small emitter of (E, 0.3 E, 1) in view beside the dim room"""
    objs, meshes = _parts(class_scene(width=width, height=height, samples=samples, depth=max_depth, **cls))
    objs.append(visible_emitter_object(E))
    return _custom(objs, meshes, width, height, samples, max_depth)


def negative_objects():
    from rt_amd import abi
    return [dict(flags=abi.M_DEFAULT, radius=2.5, center=(-5.0, 3.0, 12.0), color=(0.8, 0.9, 0.7), emission=(-2.0, 0.5, -0.1)),
            dict(flags=abi.M_REFLECTION, radius=2.0, center=(5.0, -2.0, 12.0), color=(0.9, 0.9, 0.9), emission=(-0.3, -0.3, 0.2))]


def negative_emission_scene(width=40, height=24, samples=4, max_depth=5, **cls):
    objs, meshes = _parts(class_scene(width=width, height=height, samples=samples, depth=max_depth, **cls))
    return _custom(objs + negative_objects(), meshes, width, height, samples, max_depth)


def colour_objects():
    """colours at the edges: all three channels 0 (prob = 0: the normalised albedo is 0 x inf = NaN, never read -- the
    roulette ends every path there), one channel 0, and above 1 (normalised by prob = 3); diffuse, M_REFLECTION and
    M_CHECKERED objects"""
    from rt_amd import abi
    D, R, K = abi.M_DEFAULT, abi.M_REFLECTION, abi.M_CHECKERED
    return [dict(flags=D, radius=2.5, center=(-8.0, -3.0, 10.0), color=(0.0, 0.0, 0.0)),
            dict(flags=R, radius=2.0, center=(-3.0, 4.0, 12.0), color=(0.0, 0.0, 0.0)),
            dict(flags=D | K, radius=2.5, center=(2.0, -5.0, 8.0), color=(0.0, 0.0, 0.0)),
            dict(flags=D, radius=2.0, center=(7.0, 3.0, 10.0), color=(0.7, 0.0, 0.4)),
            dict(flags=R | K, radius=2.2, center=(-9.0, 6.0, 4.0), color=(3.0, 1.5, 0.2)),
            dict(flags=D, radius=2.4, center=(9.0, -4.0, 6.0), color=(3.0, 1.5, 0.2)),
            dict(flags=R, radius=1.8, center=(0.0, 7.0, 14.0), color=(0.0, 2.0, 0.0), emission=(0.5, 0.5, 0.5))]


def colour_scene(refr=False, chk=False, tris=0):
    objs, meshes = _parts(class_scene(width=40, height=24, samples=4, depth=5, refr=refr, chk=chk, tris=tris))
    return _custom(objs + colour_objects(), meshes, 40, 24, 4, 5)


def _fixed_point_fits(sc, E):
    """pt_fixed_sums_fit restated: (max_depth + 2) x 2^-s / 2 <= 2^-30 with the launch's scale 2^s (pt_acc_scale_exp)"""
    per = (sc.max_depth + 2) * max(10 / 255, E) * 1.01
    s = min(math.frexp(2.0 ** 62 / (per * sc.samples))[1], math.frexp(2.0 ** 51 / per)[1]) - 1
    return (sc.max_depth + 2) * 2.0 ** (-s - 1) <= 2.0 ** -30


def max_emission(sc):
    """max |emission component| over all materials: what the shim hands pt_acc_scale_exp"""
    return max([abs(c) for i in range(sc.n_objects) for c in sc.objects[i].emission.tuple()] +
               [abs(c) for i in range(sc.n_meshes) for c in sc.meshes[i].emission.tuple()] + [0.0])


def fixed_sums_fit(sc, samples):
    """pt_fixed_sums_fit(max |emission|, samples, max_depth) restated for a launch or a budget of `samples`"""
    return (sc.max_depth + 2) * 2.0 ** (-acc_scale_exp(sc, samples) - 1) <= 2.0 ** -30


def window_terms_fit(sc):
    """pt_window_terms_fit restated: no term of a sample can reach 2^128"""
    return (sc.max_depth + 2.0) * max(10.0 / 255.0, max_emission(sc)) * 1.01 < 2.0 ** 128


def budget_that_flips(sc):
    """the smallest power-of-two budget at which pt_fixed_sums_fit(max_emission, budget, max_depth) is false, for a scene whose
    4-spp launch fits: an accumulation of that budget sums without a bound while each of its passes alone would take fixed point"""
    assert fixed_sums_fit(sc, 4), "the scene's own launches must fit"
    budget = 8
    while fixed_sums_fit(sc, budget):
        budget *= 2
        assert budget < 2 ** 31, "no budget of an int32 flips this scene"
    return budget


# ---- radiance queries and pixel refinement: each form's class scene with every planted object -----------------------------------
TRACE_W, TRACE_H, TRACE_DEPTH, TRACE_S = 40, 24, 5, 5
TRACE_E = (1e9, 1e30)
TRACE_SEED = 20260505
TRACE_EMITTER_C, TRACE_EMITTER_R = (-2.0, -7.0, 16.0), 2.0   # in view from the camera, clear of the other planted objects
# name -> (pt_trace_rays form, pt_trace_pixels form, class, glass): as trace_expected.SCENES / test_gpu_refine.SCENES reach them
TRACE_FORMS = {
    "plain": ("pt_trace_rays", "pt_trace_pixels", dict(n_packed=4), False),
    "big": ("pt_trace_rays_big", "pt_trace_pixels_big", dict(n_packed=4, wide=True), False),
    "tri": ("pt_trace_rays_tri", "pt_trace_pixels_tri", dict(n_packed=4, tris=40), False),
    "mem": ("pt_trace_rays_mem", "pt_trace_pixels_mem", dict(n_packed=249, tris=60), False),
    "glass": ("pt_trace_rays", "pt_trace_pixels", dict(n_packed=4, refr=True), True),
}
# the planted objects in the order trace_range_scene appends them, by what the tests ask of them
PLANTED = ("bright", "negative", "negative", "zero", "zero", "zero", "one_zero", "above_one", "above_one", "above_one")


def trace_range_scene(name, E, absolute=False):
    """-> (scene, index of the first planted object): the form's class scene at TRACE_W x TRACE_H and TRACE_DEPTH plus the visible
    emitter of (E, 0.3 E, 1), the two negative emitters and the seven edge-colour objects.  absolute: every emission component of
    the scene replaced by its magnitude -- the same paths, and a sample is the sum of |T e| (the magnitude its rounding scales with)"""
    objs, meshes = _parts(class_scene(width=TRACE_W, height=TRACE_H, samples=1, depth=TRACE_DEPTH, **TRACE_FORMS[name][2]))
    first = len(objs)
    bright = dict(visible_emitter_object(E), center=TRACE_EMITTER_C, radius=TRACE_EMITTER_R)
    objs = objs + [bright] + negative_objects() + colour_objects()
    assert len(objs) - first == len(PLANTED)
    if absolute:
        for m in objs + meshes:
            m["emission"] = tuple(abs(c) for c in m.get("emission", (0.0, 0.0, 0.0)))
    return _custom(objs, meshes, TRACE_W, TRACE_H, 1, TRACE_DEPTH), first


def trace_ray_list(sc, first):
    """(origins, targets) of 40 rays: four at each planted object, from free points a little outside it on four sides (so that
    the object is the first thing ahead unless a neighbour overlaps that side), as trace_expected.reference_samples takes them"""
    import util
    objs, _ = util.scene_parts(sc)
    sides = np.array([[0.0, 0.0, 1.0], [0.6, 0.0, 0.8], [-0.6, 0.0, 0.8], [0.0, 0.6, 0.8]])
    origins, targets = [], []
    for k in range(len(PLANTED)):
        c, r = np.array(objs[first + k]["center"]), objs[first + k]["radius"]
        for j, side in enumerate(sides):
            o = c + side * (r + 1.5)
            aim = c + 0.3 * r * np.array([0.5 - 0.25 * j, 0.2 * j - 0.3, 0.0])   # off the centre: no ray runs along a normal
            origins.append(o)
            targets.append(o - (aim - o) / np.linalg.norm(aim - o))
    return np.array(origins), np.array(targets)


def trace_pixel_list(sc, first):
    """40 pixel indices of the scene's own frame: for each planted object the four pixels whose centre rays pass nearest its
    centre (the object's own sphere alone decides; what stands in front is tests/test_accum_range_cpu.py's business)"""
    import util
    objs, _ = util.scene_parts(sc)
    pos, H, V, llc = util.camera_arrays(sc.camera)
    w, h = sc.width, sc.height
    p = np.arange(w * h)
    u, v = (p % w + 0.5) / (w - 1.0), (p // w + 0.5) / (h - 1.0)
    d = pos - (llc + u[:, None] * H + v[:, None] * V)          # get_camera_ray: the direction is eye - frame point
    d /= np.sqrt((d * d).sum(axis=1))[:, None]
    out = []
    for k in range(len(PLANTED)):
        c = np.array(objs[first + k]["center"]) - pos
        miss = np.sqrt(np.maximum((c * c).sum() - (d @ c) ** 2, 0.0))   # the centre's distance from each pixel's ray
        out += np.argsort(miss, kind="stable")[:4].tolist()
    return np.array(out, dtype=np.uint32)


# the planted objects that the packed spheres of the "mem" room hide from the scene's own camera (no pixel's sample meets them
# first); the ray list of the same scene reaches them from close by
MEM_HIDDEN_FROM_CAMERA = (1, 4, 7)


# ---- accumulations: one row per sum form an accumulation can hold (tests/test_gpu_accum_range.py, test_accum_range_cpu.py) ------
SAMPLES_LIMIT = 1 << 26   # rt_hip_shim.hip, check_params: samples (a launch's, and so a budget's) must be in [1, 2^26]


def flip_room(width=40, height=24, samples=4, max_depth=5):
    """config 4's own room (ceiling light 9.4): an ordinary room whose budget_that_flips lies within SAMPLES_LIMIT.  class_scene()'s
    room is dimmer (its brightest emitter is below 1), and its fixed-point sums fit every budget the shim accepts"""
    from rt_amd import scene as S
    return S.build_scene(4, width, height, samples, max_depth)


def nan_scene(E=None, budget=9):
    """the NaN-sample scene of tests/test_gpu_edges.py (the camera at the centre of a sphere so small that the hit point rounds onto
    the centre: the normal is NaN), optionally with the hidden emitter of E sealed in its shell"""
    from rt_amd import abi, scene as S
    c = (1.0e9, 1.0e9, 1.0e9)
    objs = [dict(flags=abi.M_DEFAULT, radius=2.0e-8, center=c, color=(0.5, 0.4, 0.3), emission=(0.3, 0.2, 0.1)),
            dict(flags=abi.M_DEFAULT, radius=5.0, center=(0, 0, 0), color=(0.7, 0.7, 0.7))]
    if E is not None:
        objs.append(dict(flags=abi.M_DEFAULT, radius=3.0, center=SHELL_C, color=(0.6, 0.6, 0.6)))
        objs.append(dict(flags=abi.M_DEFAULT, radius=1.0, center=SHELL_C, color=(1.0, 1.0, 1.0), emission=(E, E, E)))
    return S.custom_scene(objs, 24, 16, budget, 4, c, (0, 0, 0))


# id -> dict(scene: () -> Scene at 4 spp, budget: Scene -> int, kernel: the member the accumulation must name, and what the row
# claims: flip (the budget's kernel differs from a 4-sample pass's), sum_bound (the budget's scale is coarser than a pass's),
# hidden (an emitter no ray reaches), hdr (the bar of assert_parity follows the brightest pixel), subset (also read over a tile subset)
ACCUM_ROWS = {
    "coarse fixed point": dict(scene=lambda: hidden_emitter_scene(1e3), budget=lambda sc: 1 << 16, kernel="pt_render_tiles",
                               sum_bound=True, hidden=True, subset=True),
    "flip by budget": dict(scene=flip_room, budget=budget_that_flips, kernel="pt_render_tiles_refr_pool", flip=True, sum_bound=True),
    "bright windowed": dict(scene=lambda: hidden_emitter_scene(1e9), budget=lambda sc: 16, kernel="pt_render_tiles_refr_pool",
                            hidden=True, subset=True),
    "fp64 slices": dict(scene=lambda: hidden_emitter_scene(1e38), budget=lambda sc: 16, kernel="pt_render_tiles_refr", hidden=True),
    "negative fixed": dict(scene=negative_emission_scene, budget=lambda sc: 16, kernel="pt_render_tiles"),
    "negative windowed": dict(scene=lambda: negative_emission_scene(refr=True), budget=lambda sc: 16, kernel="pt_render_tiles_refr_pool"),
    "visible HDR": dict(scene=lambda: visible_emitter_scene(1e9), budget=lambda sc: 16, kernel="pt_render_tiles_refr_pool", hdr=True),
    "parked walks": dict(scene=lambda: hidden_emitter_scene(1e9, tris=600), budget=lambda sc: 16,
                         kernel="pt_render_tiles_tri_queued_refr", hidden=True),
}
SMALL_ROWS = tuple(k for k, r in ACCUM_ROWS.items() if not r.get("sum_bound"))   # the rows of budget 16: cheap to render to the end
# the "largest budget" row: the plain room at the largest budget the shim accepts, found by walking down from 2^31 - 1 by powers of
# two (tests/test_gpu_accum_range.py); the kernel is what the table says at that budget (tests/test_accum_range_cpu.py asks it)
LARGEST = dict(scene=lambda: class_scene(width=40, height=24, samples=4, depth=5), first_try=2 ** 31 - 1, at_least=1 << 24,
               kernel="pt_render_tiles")


def largest_candidates():
    """2^31 - 1, then the powers of two below it"""
    return [LARGEST["first_try"]] + [1 << k for k in range(30, 0, -1)]
