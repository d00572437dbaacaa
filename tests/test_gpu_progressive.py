"""Progressive rendering on the GPU (rt_hip_accum_*, GpuScene.accumulate, render_progressive, the CLI's -p): a frame added
to in passes of any sizes is, after the whole budget, the one-shot frame BIT FOR BIT -- on every row of the pick table --
and in between it is the oracle's frame of the samples done."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import SEED
from test_gpu_parity import PICK_ROWS, _WP
from util import acc_scale_exp, assert_parity, fixed_point_floor

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    from rt_amd import abi, gpu as G
    assert abi.load_shim().rt_hip_device_count() >= 1, "no HIP device: the GPU tests must run on the GPU box"
    assert torch.cuda.is_available()
    return G


def _one_shot(gs, seed, total, integrator="path"):
    """render_tiles_chunked for the whole budget at the suggested chunks: what an accumulation must end at"""
    import torch
    chunks = gs.suggest_chunks(total)
    t, t8, st = gs.render_tiles(seed, 0, 1, total, chunks=chunks, integrator=integrator)
    torch.cuda.synchronize()
    return t.clone(), t8.clone(), st.clone(), gs.last_launch_kernel()


def _accumulate(gs, seed, passes, integrator="path", budget=None):
    """an accumulation of sum(passes) (or budget) samples, added in `passes` -> (accumulation, tiles, tiles8, stats)"""
    import torch
    acc = gs.accumulate(seed, budget or sum(passes), integrator=integrator)
    stats = torch.zeros(4, dtype=torch.int64, device=torch.device("cuda", gs.device))
    for n in passes:
        acc.add(n, stats)
    t, t8 = acc.resolve()
    torch.cuda.synchronize()
    return acc, t, t8, stats


@pytest.mark.parametrize("cls,integrator,faults,kernel", PICK_ROWS,
                         ids=[f"{k}:{i}:{'+'.join(f'{a}={b}' for a, b in c.items())}{':fault%d' % f if f else ''}" for c, i, f, k in PICK_ROWS])
def test_passes_end_at_the_one_shot_frame_on_every_row_of_the_pick_table(gpu, cls, integrator, faults, kernel):
    from rt_amd import abi
    from util import class_scene
    shim = abi.load_shim()
    sc = class_scene(**dict(cls, samples=4))
    total = gpu.n_tiles(sc.width, sc.height)
    if faults & _WP:
        shim.rt_hip_release_cache()      # no pending-ray pool yet: the launch has to ask for the wide one
    shim.rt_hip_selftest_fail_alloc(faults)
    try:
        gs = gpu.GpuScene(sc)
        t, t8, st, one_shot_kernel = _one_shot(gs, SEED, total, integrator)
        acc, at, at8, ast = _accumulate(gs, SEED, [1, 2, 1], integrator)
    finally:
        shim.rt_hip_selftest_fail_alloc(0)
    assert one_shot_kernel == kernel
    assert acc.kernel == kernel and acc.samples == 4
    assert np.array_equal(at.cpu().numpy(), t.cpu().numpy()), kernel
    assert np.array_equal(at8.cpu().numpy(), t8.cpu().numpy()), kernel
    assert ast.tolist() == st.tolist(), (kernel, ast.tolist(), st.tolist())
    gs.launch_status()
    acc.close()
    gs.close()
    sc.free()


def _scenes():
    from rt_amd import scene as S
    from util import glass_scene, whitted_scene
    return {"room": (lambda spp: S.build_scene(4, 96, 64, spp), "path"),
            "glass": (lambda spp: glass_scene(72, 48, spp), "path"),
            "whitted": (lambda spp: whitted_scene(72, 48, spp), "whitted")}


@pytest.mark.parametrize("kind", ["room", "glass", "whitted"])
def test_intermediate_frames_are_the_oracle_s_frames_of_the_samples_done(gpu, pt, kind):
    """after k < budget samples, resolve() is the mean of k samples: the oracle's frame of k samples, within the budget's
    fixed-point resolution"""
    make, integrator = _scenes()[kind]
    budget = 24
    sc = make(budget)
    gs = gpu.GpuScene(sc)
    total = gpu.n_tiles(sc.width, sc.height)
    import torch
    acc = gs.accumulate(SEED, budget, integrator=integrator)
    stats = torch.zeros(4, dtype=torch.int64, device=torch.device("cuda", 0))
    floor = max(fixed_point_floor(sc), (sc.max_depth + 2) * 2.0 ** -acc_scale_exp(sc, budget) / 2)
    for n in (3, 4):
        acc.add(n, stats)
        k = acc.samples
        t, t8 = acc.resolve()
        img, img8 = gs.untile(t, t8, 0, 1, total)
        torch.cuda.synchronize()
        mean, rgb8, ost = pt.render_pixels(sc, SEED, spp=k, integrator=integrator)
        st = dict(zip(("rays", "casts", "tests", "samples"), stats.cpu().tolist()))
        assert st["samples"] == sc.width * sc.height * k
        assert_parity(img.cpu().numpy(), img8.cpu().numpy(), st, mean, rgb8, ost, what=f"{kind} after {k} of {budget}",
                      abs_floor=floor)
    gs.launch_status()
    acc.close()
    gs.close()
    sc.free()


@pytest.mark.parametrize("kind", ["room", "glass", "whitted"])
def test_schedules_agree_at_every_common_count(gpu, kind):
    import torch
    make, integrator = _scenes()[kind]
    sc = make(12)
    gs = gpu.GpuScene(sc)
    frames = []
    for passes in ([1, 2, 3, 6], [3, 3, 3, 3], [5, 7]):
        acc = gs.accumulate(SEED, 12, integrator=integrator)
        seen = {}
        for n in passes:
            acc.add(n)
            t, t8 = acc.resolve()
            seen[acc.samples] = (t.clone(), t8.clone())
        torch.cuda.synchronize()
        frames.append(seen)
        acc.close()
    common = 0
    for a in frames:
        for b in frames:
            for k in set(a) & set(b):
                assert torch.equal(a[k][0], b[k][0]) and torch.equal(a[k][1], b[k][1]), (kind, k)
                common += 1
    assert common > 6
    gs.launch_status()
    gs.close()
    sc.free()


def test_bad_passes_change_nothing(gpu):
    from rt_amd import abi, gpu as G
    from util import glass_scene
    shim = abi.load_shim()
    sc = glass_scene(48, 32, 6)
    gs = gpu.GpuScene(sc)
    total = gpu.n_tiles(sc.width, sc.height)
    t, t8, st, _ = _one_shot(gs, SEED, total)
    acc = gs.accumulate(SEED, 6)
    acc.add(4)
    for n in (3, 0, -1):
        with pytest.raises(G.ShimError, match=r"\(-2\)"):
            acc.add(n)
        assert acc.samples == 4
    acc.add(2)
    with pytest.raises(G.ShimError, match=r"\(-2\)"):
        acc.add(1)
    at, at8 = acc.resolve()
    assert acc.samples == 6 and np.array_equal(at.cpu().numpy(), t.cpu().numpy()) and np.array_equal(at8.cpu().numpy(), t8.cpu().numpy())
    acc.close()
    # a budget < 1, and no sample yet to resolve
    p = gs.params(SEED, 0, 1, total, samples=1)
    p.samples = 0
    out = C.c_void_p()
    assert shim.rt_hip_accum_create(gs.handle, C.byref(sc.camera), C.byref(p), C.byref(out)) == abi.EINVAL and not out.value
    acc = gs.accumulate(SEED, 6)
    with pytest.raises(G.ShimError, match=r"\(-2\)"):
        acc.resolve()
    acc.close()
    gs.close()
    sc.free()


def test_create_holds_the_pools_it_planned_with(gpu):
    """an accumulation on a glass mesh takes the parked-walk refraction member and its wide pending-ray pool at creation; passes
    made while both allocations would now fail stay on that member, and the frame is still the one-shot frame"""
    from rt_amd import abi
    from util import class_scene
    shim = abi.load_shim()
    sc = class_scene(n_packed=4, tris=400, mesh_refr=True, samples=6)
    gs = gpu.GpuScene(sc)
    total = gpu.n_tiles(sc.width, sc.height)
    t, t8, st, kernel = _one_shot(gs, SEED, total)
    assert kernel == "pt_render_tiles_tri_queued_refr"
    import torch
    acc = gs.accumulate(SEED, 6)
    stats = torch.zeros(4, dtype=torch.int64, device=torch.device("cuda", 0))
    acc.add(1, stats)
    shim.rt_hip_selftest_fail_alloc(abi.FAIL_ALLOC_PARK_WS | abi.FAIL_ALLOC_WIDE_PEND)
    try:
        acc.add(2, stats)
        acc.add(3, stats)
        at, at8 = acc.resolve()
        torch.cuda.synchronize()
    finally:
        shim.rt_hip_selftest_fail_alloc(0)
    assert acc.kernel == kernel
    assert np.array_equal(at.cpu().numpy(), t.cpu().numpy()) and np.array_equal(at8.cpu().numpy(), t8.cpu().numpy())
    assert stats.tolist() == st.tolist()
    gs.launch_status()
    acc.close()
    gs.close()
    sc.free()


def test_closing_the_scene_first_closes_its_accumulations(gpu):
    """GpuScene.close() destroys the accumulations still open on it before the scene (rt_hip.h: the scene outlives them): the
    garbage collector finalises a scene and its accumulations in any order when they die together, as after a failed test.
    The accumulation's own close() is then a no-op, and the device stays usable"""
    import torch
    from util import glass_scene
    sc = glass_scene(48, 32, 4)
    gs = gpu.GpuScene(sc)
    acc = gs.accumulate(SEED, 4)
    acc.add(2)
    torch.cuda.synchronize()
    gs.close()
    assert not acc.handle and acc.samples == 0
    acc.close()
    assert float(torch.ones(4, device="cuda").sum()) == 4.0   # no HIP error left behind for the next call to find
    gs = gpu.GpuScene(sc)
    _one_shot(gs, SEED, gpu.n_tiles(sc.width, sc.height))
    gs.launch_status()
    gs.close()
    sc.free()


def _host_frame(host, sc, opt, pass_samples=None, calls=None):
    fb = np.zeros((sc.height, sc.width, 3), dtype=np.uint8)
    lin = np.zeros((sc.height, sc.width, 3), dtype=np.float32)
    if pass_samples is None:
        host.render_ex(fb.ctypes.data, lin.ctypes.data, sc.objects, sc.n_objects, None, 0, C.byref(sc.camera), C.byref(opt))
        return fb, lin, opt.samples
    from rt_amd import abi

    def on_pass(done, total, secs, user):
        calls.append((done, total, secs))
    cb = abi.PASS_FN(on_pass)
    held = host.render_progressive(fb.ctypes.data, lin.ctypes.data, sc.objects, sc.n_objects, None, 0, C.byref(sc.camera),
                                   C.byref(opt), pass_samples, C.cast(cb, C.c_void_p), None)
    return fb, lin, held


def test_render_progressive_host_path(gpu):
    import torch
    from rt_amd import abi, scene as S
    host = abi.load_host()
    sc = S.build_scene(4, 120, 72, 20)
    opt = abi.Options()
    opt.width, opt.height, opt.samples = sc.width, sc.height, sc.samples
    host.rt_set_max_depth(sc.max_depth)
    host.rt_set_seed(SEED)
    host.rt_set_devices(1)
    full8, full, _ = _host_frame(host, sc, opt)
    # whole budget in passes of 6 (6, 12, 18, 20): render_ex's frame, byte for byte (config 4's room keeps fixed-point sums)
    calls = []
    r0 = C.c_longlong.in_dll(host, "ray_count").value
    fb, lin, held = _host_frame(host, sc, opt, 6, calls)
    assert held == 20 and host.rt_last_render_cancelled() == 0
    assert [c[0] for c in calls] == [6, 12, 18, 20] and all(c[1] == 20 and c[2] > 0 for c in calls)
    assert np.array_equal(fb, full8) and np.array_equal(lin, full)
    mean, rgb8, ost = __import__("oracle_py").PtOracle().render_pixels(sc, SEED, want_rgb8=False)
    assert C.c_longlong.in_dll(host, "ray_count").value - r0 == ost["rays"]
    # the cancel flag already raised: one pass, and a whole image of its samples
    flag = C.c_int(1)
    host.rt_set_cancel_flag(C.byref(flag))
    calls = []
    try:
        fb, lin, held = _host_frame(host, sc, opt, 6, calls)
        cancelled = host.rt_last_render_cancelled()
    finally:
        host.rt_set_cancel_flag(None)
    assert held == 6 and cancelled == 1 and [c[0] for c in calls] == [6]
    tiles = fb.reshape(sc.height // 8, 8, sc.width // 8, 8, 3)
    assert tiles.any(axis=(1, 3, 4)).all(), "a black tile"
    gs = gpu.GpuScene(sc)
    acc = gs.accumulate(SEED, 20)
    acc.add(6)
    total = gpu.n_tiles(sc.width, sc.height)
    t, t8 = acc.resolve()
    img, img8 = gs.untile(t, t8, 0, 1, total)
    torch.cuda.synchronize()
    assert np.array_equal(fb, img8.cpu().numpy()) and np.array_equal(lin, img.cpu().numpy())
    # more than one device is refused
    host.rt_set_devices(2)
    try:
        assert host.render_progressive(fb.ctypes.data, None, sc.objects, sc.n_objects, None, 0, C.byref(sc.camera),
                                       C.byref(opt), 6, None, None) == abi.EINVAL
    finally:
        host.rt_set_devices(1)
    acc.close()
    gs.close()


def test_cli_passes_write_the_one_shot_png(gpu, tmp_path):
    from rt_amd import abi
    from util import decode_png_rgb8
    exe = os.path.join(abi.PKG_DIR, "host", "raytracer")
    base = [exe, "-w", "80", "-h", "48", "-s", "10", "-c", "4", "-d", "6"]
    one, prog = str(tmp_path / "one.png"), str(tmp_path / "prog.png")
    r1 = subprocess.run(base + ["-o", one], capture_output=True, text=True, timeout=120)
    r2 = subprocess.run(base + ["-o", prog, "-p", "4"], capture_output=True, text=True, timeout=120)
    assert r1.returncode == 0 and r2.returncode == 0, (r1.stderr, r2.stderr)
    assert "pass:" not in r1.stdout
    passes = [ln for ln in r2.stdout.splitlines() if ln.startswith("pass:")]
    assert [ln.split()[1] for ln in passes] == ["4", "8", "10"], r2.stdout
    cast = lambda out: [ln for ln in out.splitlines() if ln.startswith("cast ")]
    assert cast(r1.stdout) == cast(r2.stdout) and "done." in r2.stdout
    assert np.array_equal(decode_png_rgb8(one), decode_png_rgb8(prog))
