"""Probe updates on the GPU (include/rt_hip.h, "probe updates"): the blends equal their restatement (tests/probe_update_expected.py)
bit for bit on crafted sums; a round equals the composition of the public calls pushed through the restated blends; a round on a
fresh state is the grid bake; no bit depends on the slices; a rotation of phases touches every probe once; an invalid probe stays
alone and heals; a state follows a moved light; refusals leave the state untouched; and the Python state object is the C calls."""
import ctypes as C
import os

import numpy as np
import pytest

import probe_expected as P
import probe_grid_expected as PG
import probe_update_expected as PU
import probe_vis_expected as PV

pytestmark = pytest.mark.gpu

DEPTH = 4
W, H = 33, 17
S, R = 8, 4
SEED = P.SEED
GRIDS = {18: PG.Grid(origin=(-15.0, 0.0, -12.0), step=(15.0, 8.0, 16.0), count=(3, 3, 2)),
         65: PG.Grid(origin=(-16.0, 2.0, -14.0), step=(8.0, 1.5, 1.0), count=(5, 13, 1))}   # 65: a wave boundary inside the probes
_CACHE = {}


@pytest.fixture
def gpu():
    import torch
    from rt_amd import abi, gpu as G
    assert abi.load_shim().rt_hip_device_count() >= 1, "no HIP device: the GPU tests must run on the GPU box"
    assert torch.cuda.is_available()
    return G


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32, 1: np.uint8}[a.dtype.itemsize])


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _same(a, b):
    """bit-equal, a NaN matching any NaN"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and ((_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))).all()


def _dev(a, dtype=None):
    import torch
    a = np.ascontiguousarray(a)
    return torch.as_tensor(a if dtype is None else a.astype(dtype), device="cuda:0").clone()


def _cube_scene():
    """config 1's spheres and the cube of tests/golden/c3_cube.obj, as tests/test_gpu_probe_vis.py sets it up"""
    from rt_amd import abi, scene as Sc
    host = abi.load_host()
    mesh = abi.TriangleMesh()
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "c3_cube.obj")
    assert host.load_obj(gold.encode(), C.byref(mesh))
    host.rt_mesh_flip_winding(C.byref(mesh))
    for k in range(36):
        v = mesh.vertices[k]
        v.pos = abi.Vec3(v.pos.x * 4, v.pos.y * 4 - 1, v.pos.z * 4)
    sc = Sc.build_scene(1, W, H, 1, DEPTH)
    meshes = (abi.MeshObject * 1)()
    meshes[0].flags = abi.M_REFLECTION
    meshes[0].color = abi.Vec3(0.9, 0.8, 0.7)
    meshes[0].emission = abi.Vec3(0, 0, 0)
    meshes[0].mesh = mesh
    sc.meshes, sc.n_meshes, sc.n_triangles = meshes, 1, 12
    return sc


def _scene(gpu, name):
    if name not in _CACHE:
        from rt_amd import scene as Sc
        sc = {"spheres": lambda: Sc.build_scene(2, W, H, 1, DEPTH), "mesh": _cube_scene}[name]()
        _CACHE[name] = (sc, gpu.GpuScene(sc))
    return _CACHE[name]


def _vis(grid, res=R):
    return PV.Vis(step=grid.step, res=res)


class State:
    """a grid's state as numpy arrays, and its copy on the device"""

    def __init__(self, age, coeff, moments, change, status=None):
        self.age, self.coeff, self.moments, self.change = (np.array(x) for x in (age, coeff, moments, change))
        with np.errstate(all="ignore"):
            self.coeff_f = self.coeff.astype(np.float32)
        self.status = np.full(len(self.age), 7, dtype=np.uint32) if status is None else np.array(status)

    @classmethod
    def crafted(cls, n, texels, seed=3):
        with np.errstate(all="ignore"):
            return cls(*PU.crafted_state(n, texels, seed))

    @classmethod
    def fresh(cls, n, texels):
        """every age 0 over a state of NaN: nothing of it may be read"""
        return cls(np.zeros(n, dtype=np.uint32), np.full((n, 9, 3), np.nan), np.full((n, texels, 2), np.nan), np.zeros(n))

    def device(self):
        return dict(age=_dev(self.age.view(np.int32)), coeff=_dev(self.coeff), moments=_dev(self.moments), change=_dev(self.change),
                    coeff_f=_dev(self.coeff_f), status=_dev(self.status.view(np.int32)))

    @classmethod
    def of(cls, d):
        out = cls(_host(d["age"]).view(np.uint32), _host(d["coeff"]), _host(d["moments"]), _host(d["change"]), _host(d["status"]).view(np.uint32))
        out.coeff_f = _host(d["coeff_f"])
        return out

    def equals(self, o):
        return {f: bool(_same(getattr(self, f), getattr(o, f))) for f in ("age", "coeff", "coeff_f", "moments", "change", "status")}


def _round_on_device(gs, grid, vis, upd, state, samples=S, seed=SEED, slice_rays=None):
    d = state.device()
    gs.probe_grid_update(grid.abi(), upd.abi(), samples, seed, d["coeff"], d["age"], vis.abi(grid.abi()), d["moments"], d["coeff_f"],
                         d["change"], d["status"], max_depth=DEPTH, slice_rays=slice_rays)
    return State.of(d)


def _fresh_sums(gpu, gs, grid, vis, upd, samples=S, seed=SEED):
    """the round's fresh sums from the public calls: rt_hip_bake_probes' d_sum at the round's positions under the round's seed, and
    the restated depth fold of rt_hip_probe_rays' rays and rt_hip_query_rays' answers -> (total, depth sums, status, probes)"""
    idx = PU.probes(grid.n, upd.stride, upd.phase)
    pos = PG.positions(grid)[idx]
    seed_u = PU.round_seed(seed, upd.round)
    bake = gs.bake_probes(pos, samples, seed_u, max_depth=DEPTH, details=True)
    rays = gpu.probe_rays(pos, samples, seed_u)
    hits = gs.query_rays(rays, want=("status", "t"))
    sums, _ = PV.fold(_host(rays), _host(hits["status"]).view(np.uint32), _host(hits["t"]), samples, vis)
    return _host(bake["sum"]), sums, _host(bake["status"]).view(np.uint32), idx


def _composed(gpu, gs, grid, vis, upd, state, samples=S, seed=SEED):
    """the round as the header states it: the public calls' sums pushed through the restated blends"""
    total, sums, status, idx = _fresh_sums(gpu, gs, grid, vis, upd, samples, seed)
    with np.errstate(all="ignore"):
        coeff, coeff_f, change = PU.blend_coeff(total, samples, upd, state.age, state.coeff, state.change)
        moments = PU.blend_moments(sums, vis.d_max, upd, state.age, state.moments)
    out = State(PU.age_step(state.age, upd), coeff, moments, change, state.status)
    out.coeff_f = state.coeff_f.copy()
    out.coeff_f[idx] = coeff_f[idx]
    out.status[idx] = status
    return out


# ---- 1. the blends equal the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", [0.0, 0.9])
@pytest.mark.parametrize("n,stride,phase", [(18, 1, 0), (18, 19, 18), (18, 18, 17), (65, 1, 0), (65, 2, 1), (65, 70, 3)])
def test_blends_equal_the_restatement(gpu, h, n, stride, phase):
    """M is 18, 0, 1, 65, 32 and 1: none, one, and counts that are no multiple of 64; probes outside the round keep their bytes"""
    grid = GRIDS[n]
    m = PU.count(n, stride, phase)
    for res, (change, fast) in ((2, (0.0, 0.0)), (32, (0.25, 0.5)), (R, (1e-3, 0.0))):
        vis, upd = _vis(grid, res), PU.Update(stride, phase, 0, h, change, fast)
        st = State.crafted(n, res * res, seed=3 + res)
        total = PU.crafted_sums(m, S, seed=40 + res)
        sums = PU.crafted_depth_sums(m, res * res, seed=50 + res)
        with np.errstate(all="ignore"):
            want_c, want_f, want_change = PU.blend_coeff(total, S, upd, st.age, st.coeff, st.change)
            want_m = PU.blend_moments(sums, vis.d_max, upd, st.age, st.moments)
        d = st.device()
        gpu.probe_blend_coeff(total, S, grid.abi(), upd.abi(), d["age"], d["coeff"], d["coeff_f"], d["change"])
        gpu.probe_blend_moments(sums, grid.abi(), vis.abi(grid.abi()), upd.abi(), d["age"], d["moments"])
        gpu.probe_age_step(grid.abi(), upd.abi(), d["age"])
        got = State.of(d)
        idx = PU.probes(n, stride, phase)
        assert _same(got.coeff, want_c), np.argwhere(_bits(got.coeff) != _bits(want_c))[:4]
        assert _same(got.moments, want_m), np.argwhere(_bits(got.moments) != _bits(want_m))[:4]
        assert _same(got.change, want_change) and (got.age == PU.age_step(st.age, upd)).all()
        want_ff = st.coeff_f.copy()
        want_ff[idx] = want_f[idx]
        assert _same(got.coeff_f, want_ff)
        rest = np.setdiff1d(np.arange(n), idx)   # as bytes: a NaN of the old state keeps its payload
        for f in ("coeff", "coeff_f", "moments", "change", "age", "status"):
            assert (_bits(getattr(got, f)[rest]) == _bits(getattr(st, f)[rest])).all(), f
        fresh = st.age[idx] == 0   # the NaN the old state holds where the age is 0 does not leak
        if m:
            assert (np.isnan(got.coeff[idx][fresh]) == np.isnan(total[fresh])).all()
            assert (np.isnan(got.moments[idx][fresh][..., 0]) == np.isnan(sums[fresh][..., 0])).all()


def test_the_fast_rule_on_its_threshold(gpu):
    """c == change * m and one ulp either side, one probe each: the kernel's comparison is the restatement's strict >"""
    grid = PG.Grid(count=(3, 1, 1))
    upd = PU.Update(1, 0, 0, 0.9, 0.25, 0.5)
    cases = PU.threshold_case(upd.change, S)
    old, total = np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases])
    age = np.full(3, 10, dtype=np.uint32)
    want, _, want_change = PU.blend_coeff(total, S, upd, age, old)
    plain, _, _ = PU.blend_coeff(total, S, PU.Update(1, 0, 0, 0.9), age, old)
    assert [bool(_same(want[k], plain[k])) for k in range(3)] == [True, True, False]
    d_coeff, d_change = _dev(old), _dev(np.zeros(3))
    gpu.probe_blend_coeff(total, S, grid.abi(), upd.abi(), _dev(age.view(np.int32)), d_coeff, None, d_change)
    assert _same(_host(d_coeff), want) and _same(_host(d_change), want_change)


# ---- 2. a round equals its composition ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["spheres", "mesh"])
@pytest.mark.parametrize("n,stride,phase,round", [(18, 1, 0, 0), (18, 4, 1, 5), (65, 2, 1, 0xFFFFFFFF)])
def test_a_round_equals_its_composition(gpu, name, n, stride, phase, round):
    sc, gs = _scene(gpu, name)
    grid, vis = GRIDS[n], _vis(GRIDS[n])
    for h, change, fast in ((0.9, 0.0, 0.0), (0.5, 0.25, 0.5)):
        upd = PU.Update(stride, phase, round, h, change, fast)
        st = State.crafted(n, R * R)
        got, want = _round_on_device(gs, grid, vis, upd, st), _composed(gpu, gs, grid, vis, upd, st)
        same = got.equals(want)
        assert all(same.values()), same
        idx = PU.probes(n, stride, phase)
        assert (got.status[idx] == 1).all() and np.isfinite(got.coeff[idx]).all()
        rest = np.setdiff1d(np.arange(n), idx)   # the round's status words land on the round's probes and on no other
        assert (got.status[rest] == 7).all() and (st.status == 7).all()


# ---- 3. the anchor -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["spheres", "mesh"])
def test_a_round_on_a_fresh_state_is_the_grid_bake(gpu, name):
    sc, gs = _scene(gpu, name)
    grid, vis = GRIDS[18], _vis(GRIDS[18])
    st = State.fresh(18, R * R)
    kept = 0
    for u in range(3):
        upd = PU.Update(1, 0, u, 0.0)
        bake = gs.bake_probe_grid(grid.abi(), S, PU.round_seed(SEED, u), max_depth=DEPTH, details=True, vis=vis.abi(grid.abi()))
        got = _round_on_device(gs, grid, vis, upd, st)
        assert _same(got.coeff, _host(bake["coeff"])) and _same(got.coeff_f, _host(bake["coeff_f"]))
        assert (got.status == _host(bake["status"]).view(np.uint32)).all() and (got.age == u + 1).all() and (u > 0 or (got.change == 1.0).all())
        baked = _host(bake["moments"])
        if u == 0:
            assert _same(got.moments, baked)
        else:   # a texel the round's rays say nothing about (W == 0) keeps the old bits; every other one is the bake's
            _, sums, _, _ = _fresh_sums(gpu, gs, grid, vis, upd)
            silent = sums[..., 0] == 0.0
            assert _same(got.moments[~silent], baked[~silent]) and _same(got.moments[silent], st.moments[silent])
            assert (baked[silent] == (vis.d_max, vis.d_max * vis.d_max)).all()
            kept += int(silent.sum())
        st = got
    print(f"{name}: {kept} texels of 2 x {18 * R * R} kept their old moments under h = 0")


# ---- 4. no bit depends on slice_rays -------------------------------------------------------------------------------------------------------
def test_slices_change_no_bit(gpu):
    sc, gs = _scene(gpu, "mesh")
    grid, vis = GRIDS[18], _vis(GRIDS[18])
    upd = PU.Update(2, 1, 3, 0.9, 0.25, 0.5)
    m = PU.count(18, 2, 1)
    st = State.crafted(18, R * R)
    outs = [_round_on_device(gs, grid, vis, upd, st, slice_rays=k) for k in (1, 7, S, m * S, m * S + 100)]   # 7 cuts a probe's rays
    for o in outs[1:]:
        same = o.equals(outs[0])
        assert all(same.values()), same


# ---- 5. rotation ---------------------------------------------------------------------------------------------------------------------------
def test_a_rotation_touches_every_probe_once(gpu):
    sc, gs = _scene(gpu, "spheres")
    grid, vis = GRIDS[18], _vis(GRIDS[18])
    got = want = State.fresh(18, R * R)
    for u in range(4):
        upd = PU.Update(4, u, u, 0.9)
        got, want = _round_on_device(gs, grid, vis, upd, got), _composed(gpu, gs, grid, vis, upd, want)
    assert (got.age == 1).all() and np.isfinite(got.coeff).all() and np.isfinite(got.moments).all()
    same = got.equals(want)
    assert all(same.values()), same
    for upd in (PU.Update(19, 18, 0), PU.Update(1 << 20, 18, 7), PU.Update(1000, 999, 1)):   # a stride above n, phases >= n: M == 0
        assert PU.count(18, upd.stride, upd.phase) == 0
        after = _round_on_device(gs, grid, vis, upd, got)
        for f in ("coeff", "coeff_f", "moments", "change", "age", "status"):
            assert (_bits(getattr(after, f)) == _bits(getattr(got, f))).all(), f


# ---- 6. invalid probes -----------------------------------------------------------------------------------------------------------------------
def test_an_invalid_probe_stays_alone_and_heals(gpu):
    """A checked grid has no position that is not finite, so the invalid probe enters where the contract lets any bytes in: the
    round's sums of one probe are what the folds leave for a probe with an invalid ray -- NaN throughout."""
    sc, gs = _scene(gpu, "spheres")
    grid, vis = GRIDS[18], _vis(GRIDS[18])
    upd = PU.Update(1, 0, 0, 0.9)
    total, sums, _, _ = _fresh_sums(gpu, gs, grid, vis, upd)
    st = State.crafted(18, R * R)
    bad = 7
    assert st.age[bad] != 0

    def blended(total, sums, state):
        d = state.device()
        gpu.probe_blend_coeff(total, S, grid.abi(), upd.abi(), d["age"], d["coeff"], d["coeff_f"], d["change"])
        gpu.probe_blend_moments(sums, grid.abi(), vis.abi(grid.abi()), upd.abi(), d["age"], d["moments"])
        gpu.probe_age_step(grid.abi(), upd.abi(), d["age"])
        return State.of(d)

    clean = blended(total, sums, st)
    total_bad, sums_bad = total.copy(), sums.copy()
    total_bad[bad], sums_bad[bad] = np.nan, np.nan
    hurt = blended(total_bad, sums_bad, st)
    assert np.isnan(hurt.coeff[bad]).all() and np.isnan(hurt.coeff_f[bad]).all() and np.isnan(hurt.moments[bad]).all()
    others = np.arange(18) != bad
    for f in ("coeff", "coeff_f", "moments", "change", "age"):
        assert (_bits(getattr(hurt, f)[others]) == _bits(getattr(clean, f)[others])).all(), f
    stuck = blended(total, sums, hurt)   # a NaN state does not leave by blending ...
    assert np.isnan(stuck.coeff[bad]).all()
    hurt.age[bad] = 0                     # ... it leaves when the probe starts over
    healed = blended(total, sums, hurt)
    fresh = (total[bad] * (1.0 / S)) * P.K[P.SPHERE]
    assert _same(healed.coeff[bad], fresh) and np.isfinite(healed.moments[bad]).all() and healed.age[bad] == 1


# ---- 7. it follows a move --------------------------------------------------------------------------------------------------------------------
def _l0_distance(a, b):
    return float(np.sqrt(((a[:, 0, :] - b[:, 0, :]) ** 2).sum()))


def test_the_state_follows_a_moved_light(gpu):
    """Bake at placement A, move the emitter to B, run 40 rounds of 8 rays at h = 0.9: the state ends nearer to a 4,096-ray bake at
    B than it was before the move, and nearer than one fresh 8-ray bake at B.  Comparisons under fixed seeds, not thresholds.
    The state is WARMED first, which the protocol leaves open: every age is set to 4096 / 8 = 512, as if the bake had been that many
    rounds, so that the first round after the move already blends at 1 - h and not at 1 / (age + 1).  The second comparison is
    narrow (2.2376 against 2.29934) and depends on that choice."""
    import torch
    from rt_amd import scene as Sc
    sc = Sc.build_scene(2, W, H, 1, DEPTH)
    gs = gpu.GpuScene(sc)
    try:
        grid = GRIDS[18]
        lights = [i for i in range(sc.n_objects) if max(sc.objects[i].emission.tuple()) > 0]
        a = _host(gs.spheres()).copy()
        b = a.copy()
        b[lights[0], :3] = (-a[lights[0], 0], a[lights[0], 1] + 10.0, -a[lights[0], 2])

        def run(change, fast):
            gs.update_spheres(a)
            state = gs.probe_grid_state(grid.abi(), S, SEED, hysteresis=0.9, change=change, fast=fast)
            state.coeff.copy_(gs.bake_probe_grid(grid.abi(), 4096, SEED + 1, max_depth=DEPTH))
            state.age.fill_(4096 // S)   # (warm: the bake stands for that many rounds)
            before = _host(state.coeff).copy()
            gs.update_spheres(b)
            trail = []
            for _ in range(40):
                state.update()
                trail.append(_host(state.coeff).copy())
            return before, trail

        before, trail = run(0.0, 0.0)
        truth = _host(gs.bake_probe_grid(grid.abi(), 4096, SEED + 2, max_depth=DEPTH))
        once = _host(gs.bake_probe_grid(grid.abi(), S, SEED + 3, max_depth=DEPTH))
        d_before, d_after, d_once = _l0_distance(before, truth), _l0_distance(trail[-1], truth), _l0_distance(once, truth)
        print(f"L0 distance to a 4096-ray bake at B: before the move {d_before:.6g}, after 40 rounds {d_after:.6g}, one 8-ray bake {d_once:.6g}")
        _, quick = run(0.25, 0.5)
        halved = [next((k + 1 for k, c in enumerate(t) if _l0_distance(c, truth) <= 0.5 * d_before), None) for t in (trail, quick)]
        print(f"rounds to halve the distance: plain {halved[0]}, with change = 0.25, fast = 0.5: {halved[1]}")
        assert d_after < d_before and d_after < d_once, (d_before, d_after, d_once)
    finally:
        gs.close()


# ---- 8. refusals leave the state untouched ---------------------------------------------------------------------------------------------------
def test_refusals_leave_the_state_untouched(gpu):
    from rt_amd import abi
    sc, gs = _scene(gpu, "spheres")
    grid, vis = GRIDS[18], _vis(GRIDS[18])
    st = State.crafted(18, R * R)
    bad = [PU.Update(0, 0), PU.Update(2, 2), PU.Update(1, 0, 0, 1.0), PU.Update(1, 0, 0, float("nan")), PU.Update(1, 0, 0, 0.9, -1.0),
           PU.Update(1, 0, 0, 0.9, float("inf")), PU.Update(1, 0, 0, 0.9, 0.0, 1.0), PU.Update(1, 0, 0, 0.9, 0.0, -0.5)]
    for upd in bad:
        d = st.device()
        with pytest.raises(gpu.ShimError):
            gs.probe_grid_update(grid.abi(), upd.abi(), S, SEED, d["coeff"], d["age"], vis.abi(grid.abi()), d["moments"], d["coeff_f"],
                                 d["change"], d["status"], max_depth=DEPTH)
        assert all(State.of(d).equals(st).values())
        h = State(st.age, st.coeff, st.moments, st.change, st.status)
        with pytest.raises(gpu.ShimError):
            gpu.probe_update_host(sc, grid.abi(), upd.abi(), S, SEED, h.coeff, h.age, vis.abi(grid.abi()), h.moments, h.coeff_f, h.change,
                                  h.status, max_depth=DEPTH)
        assert all(h.equals(st).values())
    good = PU.Update(1, 0, 0, 0.9).abi()
    h = State(st.age, st.coeff, st.moments, st.change, st.status)
    for kw in (dict(vis=None, moments=h.moments), dict(vis=vis.abi(grid.abi()), moments=None)):   # vis and moments go together
        with pytest.raises(gpu.ShimError):
            gpu.probe_update_host(sc, grid.abi(), good, S, SEED, h.coeff, h.age, coeff_f=h.coeff_f, change=h.change, status=h.status,
                                  max_depth=DEPTH, **kw)
    with pytest.raises(gpu.ShimError):   # what the bake refuses: no samples
        gpu.probe_update_host(sc, grid.abi(), good, 0, SEED, h.coeff, h.age, vis.abi(grid.abi()), h.moments, max_depth=DEPTH)
    assert all(h.equals(st).values())


# ---- 9. Python -----------------------------------------------------------------------------------------------------------------------------
def test_the_host_form_is_the_device_form(gpu):
    sc, gs = _scene(gpu, "mesh")
    grid, vis = GRIDS[18], _vis(GRIDS[18])
    upd = PU.Update(2, 0, 9, 0.9, 0.25, 0.5)
    st = State.crafted(18, R * R)
    want = _round_on_device(gs, grid, vis, upd, st)
    h = State(st.age, st.coeff, st.moments, st.change, st.status)
    stats = gpu.probe_update_host(sc, grid.abi(), upd.abi(), S, SEED, h.coeff, h.age, vis.abi(grid.abi()), h.moments, h.coeff_f, h.change,
                                  h.status, max_depth=DEPTH)
    same = h.equals(want)
    assert all(same.values()), same
    assert stats["samples"] == PU.count(18, 2, 0) * S


def test_the_state_object_is_the_c_calls_and_survives_scene_updates(gpu):
    from rt_amd import abi, scene as Sc
    sc = Sc.build_scene(2, W, H, 1, DEPTH)
    gs = gpu.GpuScene(sc)
    try:
        grid, vis = GRIDS[18], _vis(GRIDS[18])
        moved = _host(gs.spheres()).copy()
        moved[3, :3] += (1.0, 0.5, -2.0)
        state = gs.probe_grid_state(grid.abi(), S, SEED, vis=vis.abi(grid.abi()), hysteresis=0.8, stride=2, change=0.25, fast=0.5)
        state.update()
        gs.update_spheres(moved)
        state.update(2)
        assert state.round == 3
        got = State.of(dict(age=state.age, coeff=state.coeff, moments=state.moments, change=state.change, status=state.status,
                            coeff_f=state.coeff_f))
        gs.update_spheres(_host(torch_spheres(sc)))
        d = State(np.zeros(18, dtype=np.uint32), np.zeros((18, 9, 3)), np.zeros((18, R * R, 2)), np.zeros(18), np.ones(18, dtype=np.uint32)).device()
        for u in range(3):
            if u == 1:
                gs.update_spheres(moved)
            upd = abi.probe_update(2, u % 2, u, 0.8, 0.25, 0.5)
            p = abi.probe_params(abi.PROBE_SPHERE, S, SEED, DEPTH, 0.0, 100.0)
            ws = gpu._workspace(gs.shim.rt_hip_probe_update_workspace_bytes(C.byref(grid.abi()), C.byref(vis.abi(grid.abi())), C.byref(upd), 9 * S),
                                gs.dev)
            rc = gs.shim.rt_hip_probe_grid_update(gs.handle, C.byref(grid.abi()), C.byref(vis.abi(grid.abi())), C.byref(p), C.byref(upd), 9 * S,
                                                  gpu._ptr(ws), gpu._ptr(d["coeff"]), gpu._ptr(d["coeff_f"]), gpu._ptr(d["moments"]),
                                                  gpu._ptr(d["age"]), gpu._ptr(d["change"]), gpu._ptr(d["status"]), None, None)
            assert rc == 0
            _host(d["age"])   # (the workspace lives until the round is done)
        same = got.equals(State.of(d))
        assert all(same.values()), same
        assert sorted(got.age) == [1] * 9 + [2] * 9
        rgb, rgb8 = state.preview()
        want = gs.probe_preview(grid.abi(), state.coeff, seed=SEED, vis=vis.abi(grid.abi()), moments=state.moments)
        assert (_bits(_host(rgb)) == _bits(_host(want[0]))).all() and (_host(rgb8) == _host(want[1])).all()
        state.reset()
        assert (_host(state.age) == 0).all()
    finally:
        gs.close()


def test_the_state_survives_vertex_updates_and_rebuilds(gpu):
    """a mesh scene: update_vertices and rebuild_bvh between rounds; the state equals the rounds composed on a scene that took the
    same steps"""
    grid, vis = GRIDS[18], _vis(GRIDS[18])

    def steps(gs, sc):
        pos = np.array([[sc.meshes[0].mesh.vertices[3 * t + c].pos.tuple() for c in range(3)] for t in range(12)], dtype=np.float64)
        yield 0
        gs.update_vertices(pos * 1.25 + (0.5, 0.0, -0.25))
        yield 1
        gs.rebuild_bvh()
        yield 2

    sc = _cube_scene()
    gs = gpu.GpuScene(sc)
    try:
        state = gs.probe_grid_state(grid.abi(), S, SEED, vis=vis.abi(grid.abi()), hysteresis=0.8)
        for _ in steps(gs, sc):
            state.update()
        got = State.of(dict(age=state.age, coeff=state.coeff, moments=state.moments, change=state.change, status=state.status,
                            coeff_f=state.coeff_f))
        assert gs.rebuild_info()["rebuilds"] == 1 and gs.update_info()["updates"] == 1
    finally:
        gs.close()
    sc = _cube_scene()
    gs = gpu.GpuScene(sc)
    try:
        want = State(np.zeros(18, dtype=np.uint32), np.zeros((18, 9, 3)), np.zeros((18, R * R, 2)), np.zeros(18), np.ones(18, dtype=np.uint32))
        for u in steps(gs, sc):
            want = _composed(gpu, gs, grid, vis, PU.Update(1, 0, u, 0.8), want)
    finally:
        gs.close()
    same = got.equals(want)
    assert all(same.values()) and (got.age == 3).all(), same


def torch_spheres(sc):
    """the spheres a scene was created from, as update_spheres takes them"""
    import torch
    a = np.array([[o.center.x, o.center.y, o.center.z, o.radius] for o in sc.objects[:sc.n_objects]], dtype=np.float64).reshape(-1, 4)
    return torch.from_numpy(a).to("cuda:0")
