"""The CPU expectation of a radiance query (include/rt_hip.h, rt_hip_trace_rays), from the compiled reference with nothing new under
oracle/: a camera with horizontal = vertical = 0, position = o and lower_left_corner = q makes every jittered camera ray exactly
(o, vec3_normalize(o - q)), whatever the two jitter draws were, so the reference's own trace_sample -- render()'s per-sample body --
traces a GIVEN ray under the stream (seed, pixel, s) with its first two draws spent on the jitter: the contract's sample.  Also the
numpy statement of the contract's slice reduction, and the scenes and ray sets the GPU tests trace.
"""
import copy

import numpy as np

import query_expected as Q
import util

SLICES = 4
REL_BAR = 2.0 ** -40   # the issue's bar on a sample's value (derivation: tests/test_gpu_trace.py)


def ray_camera(o, q):
    """the zero-extent camera whose every ray is (o, vec3_normalize(o - q))"""
    from rt_amd import abi
    cam = abi.Camera()
    cam.position = abi.Vec3(*[float(x) for x in o])
    cam.lower_left_corner = abi.Vec3(*[float(x) for x in q])
    cam.horizontal = abi.Vec3(0.0, 0.0, 0.0)
    cam.vertical = abi.Vec3(0.0, 0.0, 0.0)
    return cam


def _with_camera(sc, cam, width):
    out = copy.copy(sc)   # shallow: the objects and meshes are shared, never changed
    out.camera, out.width, out.height = cam, width, 2
    return out


def reference_samples(oracle, sc, origins, targets, S, seed, index_first=0, casts_oracle=None):
    """oracle: RefOracle / RefMeshOracle (at the scene's depth) or PtOracle.  -> dict: rays [n, 6] (to be fed to the device as
    GIVEN), samples [n, S, 3], paths [n], casts [n] (from casts_oracle, a PtOracle, whose ray counter must agree; else tests / primitives).
    The pixel word is y * width + x with y = 0: the ray's stream index x = index_first + i itself (the width only has to differ
    from 1, where u = (x + r) / (w - 1) would be 0 * inf; it is index_first + n where an int holds that)."""
    origins, targets = np.asarray(origins, dtype=np.float64).reshape(-1, 3), np.asarray(targets, dtype=np.float64).reshape(-1, 3)
    n = len(origins)
    width = int(min(max(index_first + n, 2), 2 ** 31 - 1))
    rays, samples = np.zeros((n, 6)), np.zeros((n, S, 3))
    paths, casts = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    for i in range(n):
        cam = ray_camera(origins[i], targets[i])
        one = _with_camera(sc, cam, width)
        rays[i, :3], rays[i, 3:] = origins[i], oracle.camera_ray(cam, 0.0, 0.0)[3:]
        for s in range(S):
            rgb, st = oracle.trace_sample(one, index_first + i, 0, s, seed)
            samples[i, s] = rgb
            paths[i] += st["rays"]
            if casts_oracle is not None:
                rgb2, st2 = casts_oracle.trace_sample(one, index_first + i, 0, s, seed, max_depth=sc.max_depth)
                assert st2["rays"] == st["rays"] and st2["tests"] == st["tests"]
                casts[i] += st2["casts"]
            else:
                casts[i] += st["casts"] if "casts" in st else st["tests"] // sc.n_primitives
    return dict(rays=rays, samples=samples, paths=paths, casts=casts)


def reduce_samples(samples):
    """the contract's mean of samples [n, S, 3]: S_k = the ascending sum, from +0.0, of the samples with s = k (mod 4);
    (S_0 + S_1) + (S_2 + S_3); times 1.0 / S"""
    samples = np.asarray(samples, dtype=np.float64)
    n, S, _ = samples.shape
    part = np.zeros((SLICES, n, 3))
    for s in range(S):
        part[s % SLICES] = part[s % SLICES] + samples[:, s]
    return ((part[0] + part[1]) + (part[2] + part[3])) * (1.0 / float(S))


def reduce_samples_scalar(samples):
    """the same, one double at a time"""
    samples = np.asarray(samples, dtype=np.float64)
    n, S, _ = samples.shape
    out = np.zeros((n, 3))
    for i in range(n):
        for c in range(3):
            part = [0.0] * SLICES
            for s in range(S):
                part[s % SLICES] = part[s % SLICES] + float(samples[i, s, c])
            out[i, c] = ((part[0] + part[1]) + (part[2] + part[3])) * (1.0 / float(S))
    return out


def value_bar(ref_samples, glass):
    """per-sample, per-channel bound on |got - ref|: 2^-40 |ref|; on scenes with M_REFRACTION 2^-40 (|ref| + the largest |ref| among
    that ray's samples)"""
    a = np.abs(ref_samples)
    return REL_BAR * (a + a.max(axis=(1, 2), keepdims=True)) if glass else REL_BAR * a


BACKGROUND = 10 / 255.0


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def depth0_expected(ref, pt, sc, rays, S, seed, index_first=0):
    """What the contract gives at max_depth = 0 for rays AS GIVEN (no camera: a direction in the band stays as it is), from the
    reference's own scan of the ray (intersect_mesh_scene) and the stream's draws (random_doubles), trace_path (raytracer.c:482-554)
    written out for MAX_DEPTH = 0, where the second call returns BACKGROUND without a scan: a miss is BACKGROUND (1 call, 1 scan);
    a hit whose roulette draw -- the stream's third -- is not below MAX(color) is the emission (1 call); otherwise 2 calls and
    e + albedo (.) BACKGROUND for a mirror, e + albedo (.) (BACKGROUND cos) for a diffuse surface, cos from random_on_hemisphere
    (:231-253) of the following draws and the hit's normal.  Scenes without M_REFRACTION and M_CHECKERED.
    -> dict: samples [n, S, 3], exact [n, S] (the value involves no rounding: compare bit for bit), paths [n], casts [n], hit [n]"""
    from rt_amd import abi
    rays = np.asarray(rays, dtype=np.float64).reshape(-1, 6)
    n = len(rays)
    samples, exact = np.zeros((n, S, 3)), np.zeros((n, S), bool)
    paths, casts, hits = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros(n, bool)
    for i in range(n):
        h = ref.intersect_mesh_scene(rays[i], sc)
        hits[i] = h["hit"]
        for s in range(S):
            casts[i] += 1
            if not h["hit"]:
                samples[i, s], exact[i, s] = BACKGROUND, True
                paths[i] += 1
                continue
            m = sc.objects[h["id"]] if h["id"] < sc.n_objects else sc.meshes[h["id"] - sc.n_objects]
            flags, color, e = int(m.flags), np.array(m.color.tuple()), np.array(m.emission.tuple())
            assert not flags & (abi.M_REFRACTION | abi.M_CHECKERED)
            prob = max(color[0], max(color[1], color[2]))
            r = pt.random_doubles(seed, index_first + i, s, 2 + 1 + 3 * 100)
            if not r[2] < prob:
                samples[i, s], exact[i, s] = e, True
                paths[i] += 1
                continue
            paths[i] += 2
            albedo = color * (1 / prob)
            if flags & abi.M_REFLECTION:
                samples[i, s] = e + albedo * np.full(3, BACKGROUND)
                continue
            k = 3
            while True:
                q = r[k:k + 3] * (1.0 - -1.0) + -1.0
                k += 3
                length = np.sqrt(_dot(q, q))
                if not length > 1:
                    break
            d = q * (1.0 / length)
            nrm = h["normal"]
            if _dot(d, nrm) < 0:
                d = d * -1.0
            samples[i, s] = e + albedo * (np.full(3, BACKGROUND) * _dot(d, nrm))
    return dict(samples=samples, exact=exact, paths=paths, casts=casts, hit=hits)


# ---- the scenes and ray sets of tests/test_gpu_trace.py ----------------------------------------------------------------------
# the scenes with which tests/test_gpu_query.py reaches its five forms (pt_trace_pick picks as pt_query_pick does), config 3's cube and
# config 5's mesh, and a glass and a checker room, so that REFRACT and CHECKER code runs.  name -> (form, depth -> scene, glass)
SCENES = {
    "rays": ("pt_trace_rays", lambda d: util.class_scene(n_packed=4, depth=d), False),
    "big": ("pt_trace_rays_big", lambda d: util.class_scene(n_packed=4, wide=True, depth=d), False),
    "tri": ("pt_trace_rays_tri", lambda d: util.class_scene(n_packed=4, tris=40, depth=d), False),
    "tri_big": ("pt_trace_rays_tri_big", lambda d: util.class_scene(n_packed=4, tris=400, open_back=True, depth=d), False),
    "mem": ("pt_trace_rays_mem", lambda d: util.class_scene(n_packed=249, tris=60, depth=d), False),
    "glass": ("pt_trace_rays", lambda d: util.class_scene(n_packed=4, refr=True, depth=d), True),
    "chk": ("pt_trace_rays", lambda d: util.class_scene(n_packed=4, chk=True, depth=d), False),
    "cube": ("pt_trace_rays_tri", lambda d: _config(3, d), False),
    "mesh": ("pt_trace_rays_tri_big", lambda d: _config(5, d), False),
}
N_RAYS = 257
SEED = 20260303


def _config(config, depth):
    from rt_amd import scene as S
    return S.build_scene(config, 32, 24, 1, depth)


def ray_set(sc, n=N_RAYS, open_back=False):
    """(origins, targets) of n rays for scene `sc`: query_expected's ray set (origins at free points, half the directions aimed at
    primitives), the target a unit step back along the direction: vec3_normalize(o - q) is the direction to rounding.  open_back
    (a room without its back wall): the last 16 rays look about -z, out of the room, so that first rays miss too"""
    rays = Q.ray_set(sc, n, seed=20260202)
    if open_back:
        d = rays[n - 16:, 3:]
        rays[n - 16:, 3:] = Q.normalize(np.array([0.0, 0.0, -1.0]) + 0.05 * (d - d.mean(axis=0)))
    return rays[:, :3].copy(), rays[:, :3] - rays[:, 3:]


OPEN_BACK = ("tri_big",)


def flags_met(sc, rays, ref):
    """the material flags of the objects the first rays hit (a cheap witness; paths meet more)"""
    objs, meshes = util.scene_parts(sc)
    exp = Q.expected(ref, sc, rays=rays)
    ids = set(exp["object"][exp["status"] == 1].tolist())
    flags = [int(sc.objects[i].flags) if i < sc.n_objects else int(sc.meshes[i - sc.n_objects].flags) for i in ids]
    return set(flags), exp
