"""Ray queries (include/rt_hip.h, rt_hip_query_*) without a GPU: the arguments are checked before the device is looked for, the
structs are what abi.py says, the host library exports intersect_rays, and the ray sets of tests/test_gpu_query.py are
non-trivial on the compiled reference's answers alone."""
import ctypes as C
import math

import numpy as np
import pytest

import query_expected as Q

EINVAL, ENODEV = -2, -1


def _host_call(shim, n=1, source=0, flags=0, camera=None, origin_radius=0.0, outputs=True, params=True, device=0):
    from rt_amd import abi, scene as S
    sc = S.build_scene(1, 16, 16, 1)
    p = abi.RtHipQueryParams()
    shim.rt_hip_query_defaults(C.byref(p))
    p.source, p.flags, p.origin_radius = source, flags, origin_radius
    if camera is not None:
        p.camera = C.pointer(camera)
    rays = np.zeros((max(min(n, 4), 1), 6))
    rays[:, 5] = 1.0
    status = np.zeros(4, np.uint32)
    hits = abi.RtHipHits()
    if outputs:
        hits.status = status.ctypes.data
    rc = shim.rt_hip_query_rays_host(sc.objects, sc.n_objects, None, 0, rays.ctypes.data, None, n, C.byref(p) if params else None, device,
                                     C.byref(hits))
    sc.free()
    return rc


def test_arguments_are_checked_before_the_device_is_looked_for():
    from rt_amd import abi
    shim = abi.load_shim()
    cam = abi.Camera()
    assert _host_call(shim, outputs=False) == EINVAL                       # all-NULL outputs
    assert _host_call(shim, n=2 ** 32) == EINVAL                           # n >= 2^32
    assert _host_call(shim, n=2 ** 40) == EINVAL
    assert _host_call(shim, source=2) == EINVAL                            # a bad source
    assert _host_call(shim, flags=2) == EINVAL                             # an unknown flag
    assert _host_call(shim, origin_radius=-1.0) == EINVAL
    assert _host_call(shim, origin_radius=math.nan) == EINVAL
    assert _host_call(shim, origin_radius=math.inf) == EINVAL
    assert _host_call(shim, source=abi.RAYS_CAMERA_UV) == EINVAL           # CAMERA_UV without a camera
    assert _host_call(shim, params=False) == EINVAL
    assert b"camera" in shim.rt_hip_last_error() or b"params" in shim.rt_hip_last_error()
    # the device form: no scene, and a misaligned ray pointer
    hits = abi.RtHipHits()
    hits.status = 16
    p = abi.query_params()
    assert shim.rt_hip_query_rays(None, 16, None, 1, C.byref(p), C.byref(hits), None) == EINVAL
    # with good arguments the answer depends on the device alone: none here means RT_HIP_ENODEV, never a CPU result
    good = [_host_call(shim), _host_call(shim, source=abi.RAYS_CAMERA_UV, camera=cam), _host_call(shim, n=0)]
    if shim.rt_hip_device_count() == 0:
        assert good == [ENODEV, ENODEV, ENODEV]
    else:
        assert good == [0, 0, 0]
    # the order of the host form's steps: the arguments, then the device -- for no ray too --, then nothing to do
    assert _host_call(shim, outputs=False, device=99) == EINVAL
    assert _host_call(shim, device=99) == ENODEV
    assert _host_call(shim, n=0, device=99) == ENODEV


def test_struct_sizes_and_names():
    from rt_amd import abi
    assert C.sizeof(abi.RtHipQueryParams) == 24 and abi.RtHipQueryParams.camera.offset == 8
    assert abi.RtHipQueryParams.origin_radius.offset == 16
    assert C.sizeof(abi.RtHipHits) == 64 and [f for f, _ in abi.RtHipHits._fields_] == list(abi.HIT_FIELDS)
    assert C.sizeof(abi.Ray) == 48 and C.sizeof(abi.Hit) == 80
    shim = abi.load_shim()
    p = abi.RtHipQueryParams()
    p.source, p.flags, p.origin_radius = 7, 7, -3.0
    shim.rt_hip_query_defaults(C.byref(p))
    assert (p.source, p.flags, p.origin_radius) == (abi.RAYS_GIVEN, 0, 0.0) and not p.camera
    n = shim.rt_hip_query_kernel_count()
    names = [shim.rt_hip_query_kernel_launches(k, None).decode() for k in range(n)]
    assert names == ["pt_query_rays", "pt_query_rays_tri", "pt_query_rays_big", "pt_query_rays_tri_big", "pt_query_rays_mem"]
    assert shim.rt_hip_query_kernel_launches(n, None) is None and shim.rt_hip_query_kernel_launches(-1, None) is None
    assert {form for form, _ in Q.SCENES.values() if form} == set(names)   # the GPU module reaches every form
    import query_edge_rays as E
    assert {Q.SCENES[name][0] for name in E.FORM_SCENES} == set(names)     # ... and so does tests/test_gpu_query_edges.py


def test_host_library_exports_intersect_rays():
    from rt_amd import abi
    host = abi.load_host()
    assert host.intersect_rays is not None
    hits = (abi.Hit * 1)()
    assert host.intersect_rays(None, 0, None, None, 0, None, 0, hits, None) == 0      # no rays: nothing to do, no device
    assert host.intersect_rays(None, 1, None, None, 0, None, 0, hits, None) == EINVAL


def test_normalisation_and_validity_rule():
    d = np.array([[3.0, 4.0, 0.0], [0.0, 0.0, 0.0], [2.0 ** 600, 0.0, 0.0], [2.0 ** -300, 2.0 ** -300, 0.0], [2.0 ** 300, 0.0, 2.0 ** 300]])
    u = Q.normalize(d)
    assert (u[0] == [3.0 * (1.0 / 5.0), 4.0 * (1.0 / 5.0), 0.0]).all()
    assert np.isnan(u[1]).all() and (u[2] == 0.0).all()            # zero: 0 * inf; an overflowing dot: x * (1 / inf)
    rays = np.concatenate([np.zeros((5, 3)), u], axis=1)
    assert Q.valid_mask(rays, np.full(5, 1.0)).tolist() == [True, False, False, True, True]
    edge = np.zeros((4, 6))
    edge[:, 3] = [math.sqrt(1.0 + 0.99 * Q.BAND), math.sqrt(1.0 + 1.01 * Q.BAND), math.sqrt(1.0 - 0.99 * Q.BAND), math.sqrt(1.0 - 1.01 * Q.BAND)]
    assert Q.valid_mask(edge, np.zeros(4)).tolist() == [True, False, True, False]
    assert Q.valid_mask(edge[:1], np.array([math.nan])).tolist() == [False]
    assert Q.valid_mask(edge[:1], np.array([-math.inf])).tolist() == [True]


@pytest.mark.parametrize("name", sorted(Q.SCENES))
def test_ray_sets_are_not_trivial(ref_mesh, name):
    """on the reference's answers alone: hits, misses over the open scenes, triangle and sphere winners"""
    sc = Q.SCENES[name][1]()
    rays = Q.ray_set(sc, 512)
    exp = Q.expected(ref_mesh(5), sc, rays=rays)
    valid = exp["status"] != 2
    assert valid.all()
    hit = exp["status"] == 1
    assert hit.sum() >= 0.25 * valid.sum(), f"{name}: {hit.sum()} hits of {valid.sum()}"
    if name in Q.OPEN_SCENES:
        assert (exp["status"] == 0).sum() >= 0.1 * valid.sum(), f"{name}: {(exp['status'] == 0).sum()} misses"
    if sc.n_meshes:
        tri = hit & (exp["prim"] != Q.NO_HIT)
        assert tri.sum() >= 8 and (hit & ~tri).sum() >= 8, f"{name}: {tri.sum()} triangle winners, {(hit & ~tri).sum()} sphere winners"
        assert (exp["object"][tri] >= sc.n_objects).all() and ((exp["bary"][tri] >= 0) & (exp["bary"][tri] <= 1)).all()
    assert (exp["object"][hit & (exp["prim"] == Q.NO_HIT)] < sc.n_objects).all()
    assert np.isinf(exp["t"][~hit]).all() and (exp["point"][~hit] == 0).all()
    sc.free()
