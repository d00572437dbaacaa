"""Reprojection across vertex updates on the GPU: rt_hip_prev_points and rt_hip_reproject_points equal the numpy restatements of
their contracts (tests/reproject_points_expected.py) BIT FOR BIT, in every call form; Temporal.frame(prev_positions=...) equals the
restatement chained step by step on a deforming mesh; and it does what it is for: the accumulated frame of a moving mesh is closer
to the converged image than the frame's own samples."""
import ctypes as C

import numpy as np
import pytest

import reproject_expected as RE
import reproject_points_expected as PE
from test_gpu_reproject import _check, _clip_rms, _dev, _dev_aov, _dev_hist, _render

pytestmark = pytest.mark.gpu

SEED = 1666943821


@pytest.fixture
def gpu():
    import torch
    from rt_amd import abi, gpu as G
    assert abi.load_shim().rt_hip_device_count() >= 1, "no HIP device: the GPU tests must run on the GPU box"
    assert torch.cuda.is_available()
    return G


def _cube():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    verts, tris = [], []
    for line in open(os.path.join(root, "tests", "golden", "c3_cube.obj")):      # config 3's cube: 12 triangles
        part = line.split()
        if part and part[0] == "v":
            verts.append([float(t) for t in part[1:4]])
        elif part and part[0] == "f":
            idx = [int(t.split("/")[0]) - 1 for t in part[1:]]
            tris += [[verts[idx[0]], verts[idx[k]], verts[idx[k + 1]]] for k in range(1, len(idx) - 1)]
    tris = np.array(tris, np.float64)
    assert tris.shape == (12, 3, 3)
    return tris


def _dev_hits(status, prim, bary, point):
    return dict(status=_dev(status), prim=_dev(prim), bary=_dev(bary), point=_dev(point))


def _points(G, status, prim, bary, point, tris, out=None):
    import torch
    hits = _dev_hits(status, prim, bary, point)
    pos = None if tris is None else torch.from_numpy(np.ascontiguousarray(tris)).cuda()
    got = G.prev_points(hits, pos, out=hits["point"] if out == "in place" else None)
    torch.cuda.synchronize()
    return got, hits


@pytest.mark.parametrize("mesh", ["cube", "one", "none"])
def test_prev_points_equal_the_restatement(gpu, mesh):
    tris = {"cube": _cube, "one": lambda: _cube()[5:6], "none": lambda: None}[mesh]()
    n_tri = 0 if tris is None else len(tris)
    pos = None if tris is None else PE.edge_positions(tris, seed=n_tri)
    for n in (0, 1, 63, 64, 65, 257, 1920 * 1080):
        status, prim, bary, point = PE.edge_hits(min(n, 4096), n_tri, seed=31 * n_tri + n % 4099)
        if n > 4096:      # the full-HD count: the 4096 edge entries tiled, with a ragged end
            rep = -(-n // 4096)
            status, prim, bary, point = [np.ascontiguousarray(np.concatenate([a] * rep)[:n]) for a in (status, prim, bary, point)]
        exp = PE.prev_points(status, prim, bary, point, pos)
        got, _ = _points(gpu, status, prim, bary, point, pos)
        assert PE.same_points(got.cpu().numpy(), exp, status, prim, n_tri), f"{mesh}, n = {n}"
        got, hits = _points(gpu, status, prim, bary, point, pos, out="in place")
        assert got.data_ptr() == hits["point"].data_ptr() and PE.same_points(got.cpu().numpy(), exp, status, prim, n_tri), f"{mesh}, n = {n}, in place"


def test_prev_points_call_forms(gpu):
    import torch
    from rt_amd import abi
    shim = abi.load_shim()
    tris = PE.edge_positions(_cube(), seed=12)
    n = 1000
    status, prim, bary, point = PE.edge_hits(n, 12, seed=77)
    exp = PE.prev_points(status, prim, bary, point, tris)
    same = lambda got, want=exp, nt=12: PE.same_points(got, want, status, prim, nt)
    hits, pos = _dev_hits(status, prim, bary, point), torch.from_numpy(tris).cuda()
    # a second stream
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        got = gpu.prev_points(hits, pos)
    s.synchronize()
    assert same(got.cpu().numpy())
    # the host form, on the device and on a logical device of a (0, 0, 0) map
    host = dict(status=status, prim=prim, bary=bary, point=point)
    assert same(gpu.prev_points_host(host, tris))
    assert same(gpu.prev_points_host(host, None), PE.prev_points(status, prim, bary, point, None), 0)
    assert gpu.prev_points_host({f: a[:0] for f, a in host.items()}, tris).shape == (0, 3)
    m = (C.c_int * 3)(0, 0, 0)
    assert shim.rt_hip_set_device_map(m, 3) == 0
    try:
        assert same(gpu.prev_points_host(host, tris, device=2))
        with pytest.raises(gpu.ShimError):
            gpu.prev_points_host(host, tris, device=3)
    finally:
        assert shim.rt_hip_set_device_map(None, 0) == 0
    # every RT_HIP_EINVAL
    out = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
    h = abi.RtHipHits()
    for f in ("status", "prim", "bary", "point"):
        setattr(h, f, hits[f].data_ptr())
    call = lambda hh, nn, p, nt, o: shim.rt_hip_prev_points(C.byref(hh) if hh is not None else None, nn, p, nt, o, None)
    assert call(h, n, pos.data_ptr(), 12, out.data_ptr()) == 0
    assert call(None, n, pos.data_ptr(), 12, out.data_ptr()) == abi.EINVAL
    assert call(h, 2 ** 32, pos.data_ptr(), 12, out.data_ptr()) == abi.EINVAL
    assert call(h, n, None, 12, out.data_ptr()) == abi.EINVAL
    assert call(h, n, pos.data_ptr(), 12, None) == abi.EINVAL
    assert call(h, n, pos.data_ptr(), 2 ** 62, out.data_ptr()) == abi.EINVAL
    for f in ("status", "prim", "bary", "point"):
        miss = abi.RtHipHits()
        for g in ("status", "prim", "bary", "point"):
            setattr(miss, g, None if g == f else hits[g].data_ptr())
        assert call(miss, n, pos.data_ptr(), 12, out.data_ptr()) == abi.EINVAL, f
    for f, nn in (("status", n), ("prim", n), ("bary", n), ("point", n - 1)):     # the output over an input; point shifted by an entry
        at = hits[f].data_ptr() + (24 if f == "point" else 0)
        assert call(h, nn, pos.data_ptr(), 12, at) == abi.EINVAL, f
    assert call(h, 3, pos.data_ptr(), 12, pos.data_ptr()) == abi.EINVAL
    assert call(h, n, pos.data_ptr(), 12, point.ctypes.data) == abi.EINVAL          # a host pointer is refused, not launched on
    assert call(h, 0, None, 0, None) == abi.EINVAL and call(h, 0, None, 0, out.data_ptr()) == 0
    torch.cuda.synchronize()
    assert same(out.cpu().numpy())


def _run(G, rgb, aov, cam, hist, pts, **p):
    import torch
    res = G.reproject(_dev(rgb), _dev_aov(aov), RE.to_camera(RE.cam_array(cam)), hist=_dev_hist(hist),
                      prev_points=None if pts is None else _dev(pts), **p)
    torch.cuda.synchronize()
    return res


@pytest.mark.parametrize("size", RE.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_reproject_points_edge_inputs_equal_the_restatement(gpu, size):
    w, h = size
    for kind, k in RE.CASES:
        rgb, aov, cam, hist, pts, _ = PE.planted_points(w, h, kind, RE.case_seed(w, h, kind))
        p = RE.params(k)
        _check(_run(gpu, rgb, aov, cam, hist, pts, **p), PE.reproject(rgb, aov, cam, hist, prev_points=pts, **p), f"{w}x{h} {kind} {p}")


def test_reproject_points_call_forms(gpu):
    import torch
    from rt_amd import abi
    shim = abi.load_shim()
    w, h = 45, 30
    rgb, aov, cam, hist, pts, _ = PE.planted_points(w, h, "small", seed=4530)
    p = RE.params(0)
    exp = PE.reproject(rgb, aov, cam, hist, prev_points=pts, **p)
    first = RE.reproject(rgb, aov, cam, None, **p)
    assert RE.mismatch(exp, RE.reproject(rgb, aov, cam, hist, **p))                  # (the points make a difference here)
    _check(_run(gpu, rgb, aov, cam, None, pts, **p), first, "first frame")
    _check(_run(gpu, rgb, aov, cam, RE.zero_history(w, h), pts, **p), first, "zero-filled history")
    # no previous points: gpu.reproject of today; step 3's own point: the same on every pixel that reaches step 3
    old = _run(gpu, rgb, aov, cam, hist, None, **p)
    _check(old, RE.reproject(rgb, aov, cam, hist, **p), "prev_points=None")
    info = {}
    RE.reproject(rgb, aov, cam, hist, info=info, **p)
    own = _run(gpu, rgb, aov, cam, hist, PE.step3_points(aov, cam, w, h), **p)
    at = info["candidate"]
    for f in ("rgb", "len", "motion", "rgb8"):
        a, b = own[f].cpu().numpy()[at], old[f].cpu().numpy()[at]
        assert np.array_equal(a, b) if f == "rgb8" else RE.same_bits(a, b), f
    # in place
    d_rgb, d_aov, d_hist, c, d_pts = _dev(rgb), _dev_aov(aov), _dev_hist(hist), RE.to_camera(cam), _dev(pts)
    res = gpu.reproject(d_rgb, d_aov, c, hist=d_hist, out=dict(rgb=d_rgb), prev_points=d_pts, **p)
    torch.cuda.synchronize()
    assert res["rgb"].data_ptr() == d_rgb.data_ptr()
    _check(res, exp, "in place")
    # each optional output NULL, through the C-ABI
    d_rgb = _dev(rgb)
    a, ha = gpu._reproject_aov(d_aov, w * h, d_rgb.device, "frame"), gpu._reproject_aov(d_hist["aov"], w * h, d_rgb.device, "history")
    pp = abi.reproject_params(**p)
    for drop in ("rgb8", "motion"):
        o = dict(rgb=torch.full((h, w, 3), 7.0, device="cuda"), len=torch.full((h, w), 7.0, device="cuda"),
                 motion=torch.full((h, w, 2), 7.0, device="cuda"), rgb8=torch.full((h, w, 3), 7, dtype=torch.uint8, device="cuda"))
        ptr = lambda f: None if f == drop else C.c_void_p(o[f].data_ptr())
        assert shim.rt_hip_reproject_points(d_rgb.data_ptr(), C.byref(a), C.byref(c), d_hist["rgb"].data_ptr(), d_hist["len"].data_ptr(),
                                            C.byref(ha), C.byref(d_hist["camera"]), w, h, C.byref(pp), d_pts.data_ptr(), ptr("rgb"),
                                            ptr("rgb8"), ptr("len"), ptr("motion"), None) == 0
        torch.cuda.synchronize()
        assert (o[drop] == 7).all()
        _check({f: t for f, t in o.items() if f != drop}, exp, f"without {drop}")
    # a second stream
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        res = gpu.reproject(d_rgb, d_aov, c, hist=d_hist, prev_points=d_pts, **p)
    s.synchronize()
    _check(res, exp, "second stream")
    # the previous points over an output are refused; so is what rt_hip_reproject refuses
    for f, dtype in (("rgb", torch.float32), ("len", torch.float32), ("motion", torch.float32), ("rgb8", torch.uint8)):
        big = torch.zeros(w * h * 24, dtype=torch.uint8, device="cuda")
        shape = dict(rgb=(h, w, 3), len=(h, w), motion=(h, w, 2), rgb8=(h, w, 3))[f]
        numel = int(np.prod(shape))
        over = big.view(dtype)[:numel].view(shape)
        with pytest.raises(gpu.ShimError):
            gpu.reproject(d_rgb, d_aov, c, hist=d_hist, out={f: over}, prev_points=big.view(torch.float64), **p)
    with pytest.raises(gpu.ShimError):
        gpu.reproject(d_rgb, d_aov, c, hist=d_hist, out=dict(len=d_hist["len"]), prev_points=d_pts, **p)
    # the host-array form
    hc = dict(hist, camera=RE.to_camera(RE.cam_array(hist["camera"])))
    _check(gpu.reproject_image_host(rgb, aov, c, hist=hc, prev_points=pts, **p), exp, "image form")
    _check(gpu.reproject_image_host(rgb, aov, c, prev_points=pts, **p), first, "image form, first frame")
    _check(gpu.reproject_image_host(rgb, aov, c, hist=hc, **p), RE.reproject(rgb, aov, cam, hist, **p), "image form, no points")


def _host_hits(hits):
    out = {f: t.cpu().numpy() for f, t in hits.items()}
    for f in ("status", "prim"):
        out[f] = out[f].view(np.uint32)
    return out


def _chained(G, gs, poses, cam, w, h, spp, info_last=None):
    """the restatement chained step by step over the poses: the scene is at poses[0] on entry; query, prev_points, reproject"""
    import torch
    uv = PE.pixel_centre_uv(w, h)
    hist, exp = None, None
    for k, pose in enumerate(poses):
        if k:
            gs.update_vertices(torch.tensor(pose, dtype=torch.float64, device="cuda"))
        rgb, aov = _render(gs, cam, SEED + k, spp)
        pts = None
        if k:
            hits = gs.query_uv(uv, camera=cam, want=("status", "prim", "bary", "point"))
            torch.cuda.synchronize()
            hh = _host_hits(hits)
            pts = PE.prev_points(hh["status"], hh["prim"], hh["bary"], hh["point"], poses[k - 1])
        info = info_last if k == len(poses) - 1 and info_last is not None else None
        exp = PE.reproject(rgb, aov, cam, hist, prev_points=pts, info=info, **RE.DEFAULTS)
        hist = dict(rgb=exp["rgb"], len=exp["len"], aov=aov, camera=cam)
    return exp, aov


def test_temporal_follows_a_deforming_mesh(gpu):
    """three poses at 96 x 54, 4 spp: Temporal.frame(prev_positions=...) equals the restatement chained step by step, and most of
    the mesh's pixels blend"""
    import torch
    w, h, spp = 96, 54, 4
    poses = [PE.wobble_pose(k) for k in range(3)]
    sc = PE.mesh_scene(poses[0], w, h, spp)
    gs = gpu.GpuScene(sc, bvh="device")
    t = gs.temporal()
    prev = None
    for k, pose in enumerate(poses):
        cur = torch.tensor(pose, dtype=torch.float64, device="cuda")
        if k:
            gs.update_vertices(cur)
        res = t.frame(sc.camera, SEED + k, spp, prev_positions=prev)
        prev = cur
    torch.cuda.synchronize()
    got = {f: res[f].cpu().numpy() for f in ("rgb", "len", "motion", "rgb8")}
    gs.update_vertices(torch.tensor(poses[0], dtype=torch.float64, device="cuda"))
    info = {}
    exp, aov = _chained(gpu, gs, poses, sc.camera, w, h, spp, info)
    _check(got, exp, "three poses of Temporal")
    on_mesh = (aov["hits"] > 0) & (aov["object"] == sc.n_objects)
    share = float((exp["len"][on_mesh] > 1).mean())
    print(f"\ndeforming mesh: {int(on_mesh.sum())} mesh pixels, {share:.3f} of them blend")
    assert on_mesh.sum() > 200 and share > 0.5
    gs.close()
    sc.free()


# profiles/r18_reproject_moving.txt: the measured (b) / (a); the bar is that ratio plus 15 % for box-to-box and seed spread, as
# ORBIT_RATIO's (tests/test_gpu_reproject.py).
MOVING_RATIO = 0.293


def test_temporal_moving_mesh_is_closer_to_the_converged_frame(gpu):
    """8 wobble poses at 160 x 90, 4 spp, a static camera: the clipped linear RMS against 1,024 spp of the last pose (another seed)
    of (a) the last 4-spp frame alone, which is what a reset gives; (b) Temporal with prev_positions; (c) Temporal without them and
    without a reset, the stale lookup"""
    import torch
    w, h, spp, K = 160, 90, 4, 8
    poses = [PE.wobble_pose(k) for k in range(K)]
    dev = lambda a: torch.tensor(a, dtype=torch.float64, device="cuda")
    sc = PE.mesh_scene(poses[0], w, h, spp)
    gs = gpu.GpuScene(sc, bvh="device")
    out = {}
    for name in ("b", "c"):
        gs.update_vertices(dev(poses[0]))
        t = gs.temporal()
        for k in range(K):
            if k:
                gs.update_vertices(dev(poses[k]))
            res = t.frame(sc.camera, SEED + k, spp, prev_positions=dev(poses[k - 1]) if k and name == "b" else None)
        torch.cuda.synchronize()
        out[name] = res["rgb"].cpu().numpy()
    single, _ = _render(gs, sc.camera, SEED + K - 1, spp)
    ref = gs.render_image(SEED + 100, 1024)[0].cpu().numpy()
    ra, rb, rc = _clip_rms(single, ref), _clip_rms(out["b"], ref), _clip_rms(out["c"], ref)
    print(f"\nmoving mesh: clipped linear RMS (a) {ra:.4f} 4 spp alone, (b) {rb:.4f} with prev_positions, ratio {rb / ra:.3f}; "
          f"(c) {rc:.4f} stale lookup, ratio {rc / ra:.3f}")
    assert rb / ra < 1.0
    if MOVING_RATIO is not None:
        assert rb / ra <= MOVING_RATIO * 1.15
    gs.close()
    sc.free()
