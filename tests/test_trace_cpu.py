"""Radiance queries (include/rt_hip.h, rt_hip_trace_*) without a GPU: the symbols and structs are what the header says, the arguments
are checked before the device is looked for, the oracle construction of tests/trace_expected.py holds on the compiled reference, the
ray sets of tests/test_gpu_trace.py are non-trivial on the reference's answers alone, and the numpy reduction equals a scalar loop."""
import ctypes as C
import math

import numpy as np
import pytest

import trace_expected as T

EINVAL, ENODEV = -2, -1


def _host_call(shim, n=1, samples=1, integrator=0, index_first=0, origin_radius=0.0, outputs=True, max_depth=5, device=0):
    from rt_amd import abi, scene as S
    sc = S.build_scene(1, 16, 16, 1)
    p = abi.RtHipTraceParams()
    shim.rt_hip_trace_defaults(C.byref(p))
    p.samples, p.integrator, p.index_first, p.origin_radius, p.max_depth = samples, integrator, index_first, origin_radius, max_depth
    rays = np.zeros((4, 6))
    rays[:, 5] = 1.0
    status = np.zeros(4, np.uint32)
    out = abi.RtHipRadiance()
    if outputs:
        out.status = status.ctypes.data
    rc = shim.rt_hip_trace_rays_host(sc.objects, sc.n_objects, None, 0, rays.ctypes.data, n, C.byref(p), device, C.byref(out), None)
    sc.free()
    return rc


def test_symbols_and_struct_sizes():
    from rt_amd import abi
    shim = abi.load_shim()
    for name in ("rt_hip_trace_defaults", "rt_hip_trace_rays", "rt_hip_trace_rays_host", "rt_hip_trace_kernel_name",
                 "rt_hip_trace_kernel_count", "rt_hip_trace_kernel_launches"):
        assert getattr(shim, name) is not None
    assert abi.load_host().trace_rays is not None
    P, R = abi.RtHipTraceParams, abi.RtHipRadiance
    assert C.sizeof(P) == 48 and (P.camera.offset, P.origin_radius.offset, P.samples.offset, P.max_depth.offset, P.seed.offset,
                                  P.index_first.offset, P.integrator.offset) == (8, 16, 24, 28, 32, 40, 44)
    assert C.sizeof(R) == 48 and [f for f, _ in R._fields_] == list(abi.RADIANCE_FIELDS)
    p = P()
    p.source, p.flags, p.samples, p.integrator, p.index_first, p.origin_radius = 7, 7, 0, 1, 9, -3.0
    shim.rt_hip_trace_defaults(C.byref(p))
    assert (p.source, p.flags, p.samples, p.max_depth, p.seed, p.index_first, p.integrator, p.origin_radius) == (0, 0, 1, 5, 0, 0, 0, 0.0)
    assert not p.camera
    n = shim.rt_hip_trace_kernel_count()
    names = [shim.rt_hip_trace_kernel_launches(k, None).decode() for k in range(n)]
    assert names == ["pt_trace_rays", "pt_trace_rays_big", "pt_trace_rays_tri", "pt_trace_rays_tri_big", "pt_trace_rays_mem"]
    assert shim.rt_hip_trace_kernel_launches(n, None) is None and shim.rt_hip_trace_kernel_launches(-1, None) is None
    assert {form for form, _, _ in T.SCENES.values()} == set(names)      # the GPU module reaches every form
    family = [shim.rt_hip_kernel_launches(k, None).decode() for k in range(shim.rt_hip_kernel_count())]
    assert not set(names) & set(family)                                   # a list of their own


def test_arguments_are_checked_before_the_device_is_looked_for():
    from rt_amd import abi
    shim = abi.load_shim()
    assert _host_call(shim, outputs=False) == EINVAL                       # all outputs NULL
    assert _host_call(shim, samples=0) == EINVAL                           # S = 0
    assert _host_call(shim, integrator=1) == EINVAL                        # cast_ray is out of scope
    assert _host_call(shim, n=2, index_first=2 ** 32 - 1) == EINVAL        # index_first + n > 2^32
    assert _host_call(shim, n=2 ** 32) == EINVAL
    assert _host_call(shim, origin_radius=math.nan) == EINVAL
    assert _host_call(shim, origin_radius=-1.0) == EINVAL
    assert _host_call(shim, max_depth=-1) == EINVAL
    # the device form: misaligned rays (checked before the missing scene), then no scene
    out = abi.RtHipRadiance()
    out.status = 16
    p = abi.trace_params(1, 0)
    assert shim.rt_hip_trace_rays(None, 24, 1, C.byref(p), C.byref(out), None, None) == EINVAL
    assert b"aligned" in shim.rt_hip_last_error()
    assert shim.rt_hip_trace_rays(None, 16, 1, C.byref(p), C.byref(out), None, None) == EINVAL
    # n = 0 is RT_HIP_OK and needs no device; with good arguments and rays the answer depends on the device alone
    assert _host_call(shim, n=0) == 0
    assert _host_call(shim, n=1, index_first=2 ** 32 - 1) == (ENODEV if shim.rt_hip_device_count() == 0 else 0)
    assert _host_call(shim) == (ENODEV if shim.rt_hip_device_count() == 0 else 0)
    # the order of the host form's steps: the arguments, then nothing to do for no ray, then the device
    assert _host_call(shim, outputs=False, device=99) == EINVAL
    assert _host_call(shim, n=0, device=99) == 0
    assert _host_call(shim, device=99) == ENODEV


def test_the_reduction_equals_a_scalar_loop():
    rng = np.random.default_rng(3)
    for S in (1, 3, 4, 5, 9):
        x = rng.uniform(0, 1, (17, S, 3)) * 10.0 ** rng.integers(-8, 8, (17, S, 3))
        assert (T.reduce_samples(x).view(np.uint64) == T.reduce_samples_scalar(x).view(np.uint64)).all()
    assert (T.reduce_samples(np.full((1, 4, 3), 0.1)) == ((0.1 + 0.1) + (0.1 + 0.1)) * 0.25).all()


def test_the_direction_does_not_depend_on_the_jitter(ref_mesh, pt):
    sc = T.SCENES["rays"][1](4)
    o, q = T.ray_set(sc, 96)
    for orc in (ref_mesh(4), pt):
        for i in range(96):
            cam = T.ray_camera(o[i], q[i])
            a, b = orc.camera_ray(cam, 0.0, 0.0), orc.camera_ray(cam, 0.37, 5.1)
            assert (a.view(np.uint64) == b.view(np.uint64)).all() and (a[:3] == o[i]).all()
            assert abs(((a[3] * a[3] + a[4] * a[4]) + a[5] * a[5]) - 1.0) <= 2.0 ** -50
    sc.free()


def test_the_depth_0_closed_form_is_the_oracle_s(ref_mesh, pt):
    """trace_expected.depth0_expected (what the GPU test of band rays compares with) equals trace_sample at MAX_DEPTH = 0 bit for
    bit, values and counters, on unit rays, where both exist"""
    for name in ("rays", "tri", "tri_big"):
        sc = T.SCENES[name][1](0)
        o, q = T.ray_set(sc, 64, open_back=name in T.OPEN_BACK)
        res = T.reference_samples(pt, sc, o, q, 3, T.SEED, 7)
        exp = T.depth0_expected(ref_mesh(4), pt, sc, res["rays"], 3, T.SEED, 7)
        assert (res["samples"].view(np.uint64) == exp["samples"].view(np.uint64)).all(), name
        assert (res["paths"] == exp["paths"]).all() and (res["casts"] == exp["casts"]).all(), name
        sc.free()


# what the reference alone gives for the first 96 rays x 4 samples of each ray set at depth 4, pinned (a ray set that changes shows here):
# first rays that hit / miss / hit a triangle; samples of 1 trace_path call (stopped at once), of >= 3 (bounced), of 6 (ended by depth:
# calls at depth 0 .. 5, the last past MAX_DEPTH = 4); the most calls of a sample; the calls and the scans in all
PINNED = {
    "rays": (96, 0, 0, 39, 258, 109, 6, 1436, 1327),
    "tri": (96, 0, 29, 43, 258, 115, 6, 1437, 1322),
    "tri_big": (86, 10, 32, 76, 249, 115, 6, 1394, 1279),
    "glass": (96, 0, 0, 39, 261, 103, 10, 1522, 1400),
    "chk": (96, 0, 0, 39, 258, 109, 6, 1436, 1327),
}


@pytest.mark.parametrize("name", sorted(PINNED))
def test_ray_sets_are_not_trivial_and_the_restatement_agrees(ref_mesh, pt, name):
    form, make, glass = T.SCENES[name]
    sc = make(4)
    o, q = T.ray_set(sc, 96, open_back=name in T.OPEN_BACK)
    ref = T.reference_samples(ref_mesh(4), sc, o, q, 4, T.SEED, casts_oracle=pt)       # asserts equal ray and test counters
    res = T.reference_samples(pt, sc, o, q, 4, T.SEED)
    assert (ref["samples"].view(np.uint64) == res["samples"].view(np.uint64)).all()     # the compiled reference equals the restatement
    assert (ref["paths"] == res["paths"]).all() and (ref["casts"] == res["casts"]).all()
    flags, first = T.flags_met(sc, ref["rays"], ref_mesh(4))
    hit = first["status"] == 1
    assert (first["status"] != 2).all()
    per_sample = np.zeros((96, 4), np.int64)
    one = T._with_camera(sc, None, 2 ** 20)
    for i in range(96):
        one.camera = T.ray_camera(o[i], q[i])
        for s in range(4):
            per_sample[i, s] = pt.trace_sample(one, i, 0, s, T.SEED, max_depth=4)[1]["rays"]
    counts = (int(hit.sum()), int((first["status"] == 0).sum()), int((first["prim"][hit] != 0xFFFFFFFF).sum()), int((per_sample == 1).sum()),
              int((per_sample >= 3).sum()), int((per_sample == 6).sum()), int(per_sample.max()), int(ref["paths"].sum()), int(ref["casts"].sum()))
    assert counts == PINNED[name], counts
    # ... and what makes them non-trivial: hits; misses where the room is open; samples that stop at once, bounce, end by depth
    assert counts[0] >= 24 and counts[3] >= 8 and counts[4] >= 32 and counts[5] >= 1
    assert (counts[1] >= 4) == (name in T.OPEN_BACK)
    assert counts[6] > 6 if glass else counts[6] == 6                                   # two children per refractive hit
    # every material flag of the scene is met by a path (already by a first hit: half the rays are aimed at primitives)
    import util
    objs, meshes = util.scene_parts(sc)
    assert flags == {ob["flags"] for ob in objs} | {m["flags"] for m in meshes}, flags
    assert (ref["samples"] != 0).any(axis=2).mean() >= 0.25   # a dark room: a path that never meets the light carries 0
    sc.free()
