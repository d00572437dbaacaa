"""Reprojection across sphere updates on the GPU: rt_hip_prev_points_moved (pt_prev_points_moved, image_ops.hip) equals the numpy
restatement of its contract (tests/prev_points_moved_expected.py) BIT FOR BIT -- on real hits of a 12-sphere + cube scene before
and after a move, in the NULL / 0 form, which must be rt_hip_prev_points itself, and on planted entries no query returns --, in the
device and the host form; and Temporal.frame(prev_spheres=...) does what it is for: the accumulated frame of a ball moving through
config 4's room is closer to the converged image than the frame's own samples, and than the stale lookup."""
import numpy as np
import pytest

import prev_points_moved_expected as P
import sphere_update_expected as E
from test_gpu_reproject import _clip_rms, _render
from test_gpu_reproject_points import _cube

pytestmark = pytest.mark.gpu
SEED = 1666943821
FIELDS = ("status", "prim", "object", "bary", "point")


@pytest.fixture
def gpu():
    import torch
    from rt_amd import abi, gpu as G
    assert abi.load_shim().rt_hip_device_count() >= 1, "no HIP device: the GPU tests must run on the GPU box"
    assert torch.cuda.is_available()
    return G


def _scene(w=96, h=64):
    """12 spheres -- a floor, a light and ten small ones around config 3's cube -- and the cube's 12 triangles"""
    from rt_amd import abi, scene as S
    rng = np.random.default_rng(12)
    objs = [dict(flags=abi.M_DEFAULT, radius=1e4, center=(0, -10003.0, 0), color=(0.7, 0.7, 0.7)),
            dict(flags=abi.M_DEFAULT, radius=3.0, center=(0, 14, 2), color=(1, 1, 1), emission=(6, 6, 6))]
    for k in range(10):
        a = 2.0 * np.pi * k / 10
        objs.append(dict(flags=abi.M_REFLECTION if k % 4 == 3 else abi.M_DEFAULT, radius=float(rng.uniform(0.6, 1.3)),
                         center=(4.5 * np.cos(a), float(rng.uniform(-1.5, 1.5)), 4.5 * np.sin(a)), color=tuple(rng.uniform(0.3, 0.9, 3))))
    tris = _cube()
    sc = S.custom_scene(objs, w, h, 3, 5, (0, 4, 16), (0, 0, 0), meshes=[dict(flags=abi.M_DEFAULT, color=(0.8, 0.6, 0.4), triangles=tris)])
    return sc, tris


def _uv(w, h):
    ys, xs = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    return np.stack([(xs + 0.5) / (w - 1.0), (ys + 0.5) / (h - 1.0)], axis=-1).reshape(-1, 2)


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def _both_forms(G, hits, pos, prev, cur, what):
    """the device form (also in place) and the host form against the restatement"""
    import torch
    exp = P.prev_points_moved(hits, pos, prev, cur)
    d = {f: _dev(hits[f]) for f in FIELDS}
    dp = None if pos is None else _dev(pos)
    ds, dc = (None, None) if prev is None else (_dev(prev), _dev(cur))
    got = G.prev_points_moved(d, dp, ds, dc)
    torch.cuda.synchronize()
    assert P.same(got.cpu().numpy(), exp), f"{what}: the device form"
    got = G.prev_points_moved(d, dp, ds, dc, out=d["point"])
    torch.cuda.synchronize()
    assert got.data_ptr() == d["point"].data_ptr() and P.same(got.cpu().numpy(), exp), f"{what}: in place"
    assert P.same(G.prev_points_moved_host(hits, pos, prev, cur), exp), f"{what}: the host form"
    return exp


def test_real_hits_before_and_after_a_move(gpu):
    import torch
    sc, tris = _scene()
    s0 = E.spheres_of(sc)
    s1 = E.jitter(s0)
    gs = gpu.GpuScene(sc)
    uv = _uv(sc.width, sc.height)
    pos = np.ascontiguousarray(tris + 0.25)          # the cube was a quarter unit away a frame ago
    for step, (prev, cur) in (("before", (s0, s0)), ("after", (s0, s1))):
        if step == "after":
            gs.update_spheres(torch.tensor(s1, dtype=torch.float64, device="cuda"))
        q = gs.query_uv(torch.from_numpy(uv).cuda(), want=FIELDS)
        torch.cuda.synchronize()
        hits = {f: q[f].cpu().numpy().view(np.uint32) if q[f].dtype == torch.int32 else q[f].cpu().numpy() for f in FIELDS}
        on_sphere = (hits["status"] == 1) & (hits["prim"] == P.NO_PRIM)
        on_cube = (hits["status"] == 1) & (hits["prim"] != P.NO_PRIM)
        assert on_sphere.sum() > 100 and on_cube.sum() > 20 and len(set(hits["object"][on_sphere].tolist())) >= 6, step
        exp = _both_forms(gpu, hits, pos, prev, cur, step)
        # a hit point lies on its current sphere, so its previous point lies on the previous one
        k = hits["object"][on_sphere].astype(int)
        dist = np.sqrt(((exp[on_sphere] - prev[k, :3]) ** 2).sum(axis=1))
        assert (np.abs(dist - prev[k, 3]) <= 1e-9 * prev[k, 3]).all(), step      # (fp64: a few ulps of the radius, the floor's 1e4 included)
        if step == "before":
            assert np.abs(exp[on_sphere] - hits["point"][on_sphere]).max() < 1e-8, "nothing moved: the point, to rounding"
        # the NULL / 0 form is rt_hip_prev_points itself: the same bits on the same hits
        d = {f: _dev(hits[f]) for f in FIELDS}
        a = gpu.prev_points_moved(d, _dev(pos), None, None)
        b = gpu.prev_points({f: d[f] for f in ("status", "prim", "bary", "point")}, _dev(pos))
        torch.cuda.synchronize()
        assert np.array_equal(a.cpu().numpy().view(np.uint64), b.cpu().numpy().view(np.uint64)), f"{step}: the NULL / 0 form"
        _both_forms(gpu, hits, pos, None, None, step + ", no spheres")
        _both_forms(gpu, hits, None, prev, cur, step + ", no positions")
        _both_forms(gpu, hits, pos, prev[:5], cur[:5], step + ", five spheres given")
    gs.close()
    sc.free()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000])
def test_planted_entries(gpu, n):
    hits, prev, cur = P.planted(6, 12)
    rep = -(-n // len(hits["status"]))
    hits = {f: np.ascontiguousarray(np.concatenate([a] * rep)[:n]) for f, a in hits.items()}
    pos = np.random.default_rng(n).uniform(-4, 4, (12, 3, 3))
    exp = _both_forms(gpu, hits, pos, prev, cur, f"planted, n = {n}")
    if n >= 10:
        bits = exp.view(np.uint64)
        assert (bits[[0, 1, 2, 3, 6, 9]] == P.QNAN).all() and np.isinf(exp[5]).all() and np.isfinite(exp[[4, 7, 8]]).all()
    _both_forms(gpu, hits, pos, None, None, f"planted, no spheres, n = {n}")
    _both_forms(gpu, hits, pos, prev[:0], cur[:0], f"planted, an empty pair, n = {n}")


def test_n_zero_launches_nothing(gpu):
    import torch
    hits = {f: torch.zeros((0, 3) if f == "point" else ((0, 2) if f == "bary" else (0,)), dtype=torch.float64 if f in ("point", "bary") else torch.int32,
                           device="cuda") for f in FIELDS}
    assert gpu.prev_points_moved(hits, None, None, None).shape == (0, 3)


def test_temporal_moving_ball_is_closer_to_the_converged_frame(gpu):
    """a ball moved through config 4's room in 8 poses at 64 x 40, 4 spp, a static camera: the clipped linear RMS against 1,024
    spp of the last pose (another seed) of (a) the last 4-spp frame alone, which is what a reset every frame gives; (b) Temporal
    with prev_spheres; (c) Temporal without them and without a reset, the stale lookup.  (b) must beat both.
    Measured on the MI355X: see profiles/r20_sphere_update.txt."""
    import torch
    from rt_amd import scene as S
    from rt_amd import abi
    w, h, spp, K = 64, 40, 4, 8
    sc = S.build_scene(4, w, h, spp)
    s0 = E.spheres_of(sc)
    # the ball: the first packed sphere that is plainly diffuse (an emitter looks the same wherever it is looked up)
    ball = next(i for i in range(8, sc.n_objects) if sc.objects[i].flags == abi.M_DEFAULT and max(sc.objects[i].emission.tuple()) == 0.0)
    assert s0[ball, 3] < 1000

    def pose(k):
        s = s0.copy()
        s[ball] = (-9.0 + 2.5 * k, -2.0 + 0.5 * k, 22.0, 5.0)
        return s
    dev = lambda a: torch.tensor(a, dtype=torch.float64, device="cuda")
    gs = gpu.GpuScene(sc)
    out = {}
    for name in ("b", "c"):
        gs.update_spheres(dev(pose(0)))
        t = gs.temporal()
        for k in range(K):
            if k:
                gs.update_spheres(dev(pose(k)))
            res = t.frame(sc.camera, SEED + k, spp, prev_spheres=dev(pose(k - 1)) if k and name == "b" else None)
        torch.cuda.synchronize()
        out[name] = res["rgb"].cpu().numpy()
    single, _ = _render(gs, sc.camera, SEED + K - 1, spp)
    ref = gs.render_image(SEED + 100, 1024)[0].cpu().numpy()
    ra, rb, rc = _clip_rms(single, ref), _clip_rms(out["b"], ref), _clip_rms(out["c"], ref)
    print(f"\nmoving ball: clipped linear RMS (a) {ra:.4f} 4 spp alone, (b) {rb:.4f} with prev_spheres, (c) {rc:.4f} stale lookup; "
          f"(b)/(a) {rb / ra:.3f}, (b)/(c) {rb / rc:.3f}")
    assert rb < ra, "the history must help"
    assert rb < rc, "following the ball must beat the stale lookup"
    gs.close()
    sc.free()
