"""Adaptive sampling on the GPU (rt_hip_tile_error, rt_hip_accum_freeze*, rt_hip_accum_run_adaptive): tiles that stop early hold
exactly the samples [0, n_k), so every slot of an adaptive frame is, BIT FOR BIT, the slot of a uniform accumulation resolved
after n_k samples -- the oracle here is the uniform accumulation, which tests/test_gpu_progressive.py pins to the one-shot frame
and the CPU oracle.  The estimate and the stop decision are compared with tests/adaptive_expected.py bit for bit."""
import numpy as np
import pytest

import adaptive_expected as ae
from conftest import SEED

pytestmark = pytest.mark.gpu

BUDGET, PASSES = 24, (3, 5, 8, 8)


@pytest.fixture(scope="module")
def gpu():
    import torch
    from rt_amd import abi, gpu as G
    assert abi.load_shim().rt_hip_device_count() >= 1, "no HIP device: the GPU tests must run on the GPU box"
    assert torch.cuda.is_available()
    return G


def _launches(name):
    import ctypes as C
    from rt_amd import abi
    shim = abi.load_shim()
    for k in range(shim.rt_hip_kernel_count()):
        n = C.c_uint64(0)
        if shim.rt_hip_kernel_launches(k, C.byref(n)).decode() == name:
            return n.value
    raise KeyError(name)


def _scene(kind, w, h, spp=BUDGET):
    from rt_amd import scene as S
    from util import class_scene, glass_scene, whitted_scene
    if kind == "room":
        return S.build_scene(4, w, h, spp), "path"
    if kind == "glass":
        return glass_scene(w, h, spp), "path"
    if kind == "whitted_glass":
        return whitted_scene(w, h, spp), "whitted"
    if kind == "whitted":
        return class_scene(n_packed=4, chk=True, refr=True, width=w, height=h, samples=spp), "whitted"
    cls = {"queued": dict(n_packed=4, tris=400), "queued_refr": dict(n_packed=4, tris=400, mesh_refr=True),
           "wide": dict(n_packed=4, wide=True), "mem": dict(n_packed=120)}[kind]
    return class_scene(**cls, width=w, height=h, samples=spp), "path"


# scene class -> the member its accumulation runs: one per body and sum form
MEMBERS = {"room": "pt_render_tiles", "glass": "pt_render_tiles_refr_pool", "queued": "pt_render_tiles_tri_queued",
           "queued_refr": "pt_render_tiles_tri_queued_refr", "whitted": "pt_whitted_tiles", "whitted_glass": "pt_whitted_tiles_mem", "wide": "pt_render_tiles_big",
           "mem": "pt_render_tiles_pool_mem_s"}


def _random_masks(rng, count, n_freezes):
    """keep masks for `n_freezes` freezes: each freezes at least one live slot and, until the last, leaves at least one live"""
    live, masks = np.ones(count, bool), []
    for i in range(n_freezes):
        idx = np.flatnonzero(live)
        last = i == n_freezes - 1
        most = len(idx) if last else len(idx) - 1
        n = int(rng.integers(1, max(1, min(most, (len(idx) + 2) // 3)) + 1)) if most >= 1 else 0
        drop = rng.choice(idx, size=n, replace=False)
        keep = rng.random(count) < 0.5          # what the mask says about frozen slots must not matter
        keep[idx] = True
        keep[drop] = False
        masks.append(keep)
        live = live & keep
    return masks


def _masked_against_uniform(gpu, kind, w, h, first=0, stride=1, seed=1):
    """passes of PASSES with a random host mask frozen after each, next to a uniform accumulation of the same passes ->
    (count map, summed counters of the masked run)"""
    import torch
    sc, integrator = _scene(kind, w, h)
    gs = gpu.GpuScene(sc)
    total = gpu.n_tiles(w, h)
    count = (total - first + stride - 1) // stride
    assert count >= 5
    uni = gs.accumulate(SEED, BUDGET, integrator=integrator, first=first, stride=stride, count=count)
    ada = gs.accumulate(SEED, BUDGET, integrator=integrator, first=first, stride=stride, count=count)
    assert ada.kernel == uni.kernel == MEMBERS[kind]
    stats = torch.zeros(4, dtype=torch.int64, device=torch.device("cuda", gs.device))
    masks = _random_masks(np.random.default_rng(seed * 100 + w), count, len(PASSES))
    frames, want, live = {}, np.zeros(count, np.uint32), np.ones(count, bool)
    valid = ae.inside_mask(w, h, first, stride, count).sum(axis=1)
    for i, (n, keep) in enumerate(zip(PASSES, masks)):
        before, rendered = _launches(MEMBERS[kind]), int(stats[3].item())
        uni.add(n)
        ada.add(n, stats)
        torch.cuda.synchronize()
        if i > 0:
            assert _launches(MEMBERS[kind]) == before + 2, "the pass over the slot list runs the accumulation's member"
        # the pass rendered the live slots and no other: its sample counter is (valid pixels of the live tiles) x samples
        assert int(stats[3].item()) - rendered == int(valid[live].sum()) * n, (kind, i)
        t, t8 = uni.resolve()
        torch.cuda.synchronize()
        frames[uni.samples] = (t.cpu().numpy().view(np.uint32), t8.cpu().numpy())
        assert ada.samples == uni.samples
        n_live = ada.freeze(mask=keep)
        want[live & ~keep] = ada.samples
        live &= keep
        assert n_live == int(live.sum()) == ada.live_tiles
        if i < len(PASSES) - 1:
            assert 0 < n_live < count
    want[live] = ada.samples
    counts = ada.tile_samples()
    assert np.array_equal(counts, want) and len(set(counts.tolist())) >= 3
    t, t8 = ada.resolve()
    torch.cuda.synchronize()
    t, t8 = t.cpu().numpy().view(np.uint32), t8.cpu().numpy()
    for k in range(count):
        ft, ft8 = frames[int(counts[k])]
        assert np.array_equal(t[k], ft[k]) and np.array_equal(t8[k], ft8[k]), (kind, k, int(counts[k]))
    gs.launch_status()
    st = stats.cpu().tolist()
    for a in (uni, ada):
        a.close()
    gs.close()
    sc.free()
    return counts, st


@pytest.mark.parametrize("kind", sorted(MEMBERS))
def test_imposed_masks_every_slot_is_the_uniform_slot_at_its_count(gpu, kind):
    _masked_against_uniform(gpu, kind, 37, 21)


@pytest.mark.parametrize("kind", ["room", "queued_refr", "whitted"])
def test_imposed_masks_at_160_x_96(gpu, kind):
    _masked_against_uniform(gpu, kind, 160, 96, seed=2)


@pytest.mark.parametrize("kind", sorted(MEMBERS))
def test_tile_subsets(gpu, kind):
    _masked_against_uniform(gpu, kind, 37, 21, first=1, stride=3, seed=3)


@pytest.mark.parametrize("kind", ["room", "glass", "queued", "whitted"])
def test_counters_are_the_sum_over_slots(gpu, kind):
    """at 24 x 16 (6 slots) the masked run's counters equal the sum of one-tile accumulations run to n_t each"""
    import torch
    w, h = 24, 16
    # six slots cannot give four freezes a slot each and a live one: the helper's count >= 5 holds, its masks adapt
    counts, st = _masked_against_uniform(gpu, kind, w, h, seed=4)
    sc, integrator = _scene(kind, w, h)
    gs = gpu.GpuScene(sc)
    stats = torch.zeros(4, dtype=torch.int64, device=torch.device("cuda", gs.device))
    for t in range(6):
        one = gs.accumulate(SEED, BUDGET, integrator=integrator, first=t, stride=1, count=1)
        one.add(int(counts[t]), stats)
        torch.cuda.synchronize()
        one.close()
    assert st == stats.cpu().tolist() and st[3] == int(counts.sum()) * 64   # 24 x 16: every tile whole
    gs.close()
    sc.free()


@pytest.mark.parametrize("kind", ["room", "glass"])
def test_nothing_frozen_is_the_one_shot_frame_and_all_frozen_stops(gpu, kind):
    import torch
    w, h, budget = 96, 64, 64
    sc, integrator = _scene(kind, w, h, budget)
    gs = gpu.GpuScene(sc)
    total = gpu.n_tiles(w, h)
    t, t8, st = gs.render_tiles(SEED, 0, 1, total, chunks=gs.suggest_chunks(total))
    torch.cuda.synchronize()
    acc = gs.accumulate(SEED, budget)
    seen = []
    ast, _ = acc.run_adaptive(threshold=0.0, min_samples=16, on_checkpoint=lambda done, live: seen.append((done, live)) and False)
    at, at8 = acc.resolve()
    torch.cuda.synchronize()
    assert acc.samples == budget and seen == [(16, total), (32, total)] and (acc.tile_samples() == budget).all()
    assert torch.equal(at, t) and torch.equal(at8, t8)
    assert [ast[k] for k in ("rays", "casts", "tests", "samples")] == st.cpu().tolist()
    acc.close()
    # threshold = +inf: everything stops at the first checkpoint
    acc, uni = gs.accumulate(SEED, budget), gs.accumulate(SEED, budget)
    acc.run_adaptive(threshold=float("inf"), min_samples=16)
    uni.add(16)
    assert acc.samples == 16 and acc.live_tiles == 0 and (acc.tile_samples() == 16).all()
    (at, at8), (ut, ut8) = acc.resolve(), uni.resolve()
    torch.cuda.synchronize()
    assert torch.equal(at, ut) and torch.equal(at8, ut8)
    stats = torch.zeros(4, dtype=torch.int64, device=torch.device("cuda", gs.device))
    acc.add(8, stats)                       # renders nothing, returns OK, advances nothing
    at2, _ = acc.resolve()
    torch.cuda.synchronize()
    assert acc.samples == 16 and stats.cpu().tolist() == [0, 0, 0, 0] and torch.equal(at2, ut)
    gs.launch_status()
    for a in (acc, uni):
        a.close()
    gs.close()
    sc.free()


def _live_after_freeze(acc):
    """which slots a freeze left live: one more sample reaches exactly those"""
    before = acc.samples
    if acc.live_tiles == 0:
        return np.zeros(acc.count, bool)
    acc.add(1)
    return acc.tile_samples() == before + 1


@pytest.mark.parametrize("w,h,first,stride", [(1, 1, 0, 1), (9, 9, 0, 1), (37, 21, 0, 1), (160, 96, 0, 1), (37, 21, 1, 3), (64, 57, 2, 3)])
def test_tile_error_on_hostile_buffers(gpu, w, h, first, stride):
    import torch
    from test_adaptive_cpu import case_count, hostile_buffers
    count = case_count(w, h, first, stride)
    cur, prev = hostile_buffers(np.random.default_rng(w * 1000 + h + first), count)
    dev = torch.device("cuda", 0)
    got = gpu.tile_error(torch.from_numpy(cur).to(dev), torch.from_numpy(prev).to(dev), w, h, first, stride, count)
    torch.cuda.synchronize()
    want = ae.tile_error(cur, prev, w, h, first, stride, count)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("dilate", [0, 1, 2])
@pytest.mark.parametrize("w,h,first,stride", [(96, 64, 0, 1), (37, 21, 1, 3)])
def test_estimate_and_decision_on_real_resolves(gpu, w, h, first, stride, dilate):
    """config 4 at 8 and 16 samples: the device's errors and its freeze against the restatement; then imposed errors with NaN
    and inf on the same accumulation's live slots"""
    import torch
    sc, _ = _scene("room", w, h, 32)
    gs = gpu.GpuScene(sc)
    count = (gpu.n_tiles(w, h) - first + stride - 1) // stride
    acc = gs.accumulate(SEED, 32, first=first, stride=stride, count=count)
    acc.add(8)
    prev, _ = acc.resolve()
    acc.add(8)
    cur, _ = acc.resolve()
    err = gpu.tile_error(cur, prev, w, h, first, stride, count)
    torch.cuda.synchronize()
    want = ae.tile_error(cur.cpu().numpy(), prev.cpu().numpy(), w, h, first, stride, count)
    got = err.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and (got > 0).any()
    thr = float(np.median(got))
    live = np.ones(count, bool)
    keep = ae.keep_mask(got, live, w, h, first, stride, count, thr, dilate)
    assert acc.freeze(error=err, threshold=thr, dilate=dilate) == int(keep.sum())
    assert 0 < keep.sum() < count or dilate > 0
    now = _live_after_freeze(acc)
    assert np.array_equal(now, keep)
    # a second freeze on hostile errors: frozen slots stay frozen whatever their error says
    rng = np.random.default_rng(dilate + w)
    e2 = rng.random(count).astype(np.float32)
    e2[rng.random(count) < 0.15] = np.nan
    e2[rng.random(count) < 0.1] = np.inf
    keep2 = ae.keep_mask(e2, now, w, h, first, stride, count, 0.7, dilate)
    assert acc.freeze(error=torch.from_numpy(e2).to(err.device), threshold=0.7, dilate=dilate) == int(keep2.sum())
    assert np.array_equal(_live_after_freeze(acc), keep2)
    assert acc.freeze(error=err, threshold=0.0, dilate=dilate) == int(keep2.sum()), "threshold <= 0 freezes nothing"
    acc.close()
    gs.close()
    sc.free()


@pytest.mark.parametrize("kind,dilate", [("room", 0), ("glass", 0), ("room", 2)])
def test_the_driver_is_the_loop_of_the_primitives(gpu, kind, dilate):
    """run_adaptive at 160 x 96, budget 256, against the same loop written here, whose decisions are adaptive_expected's applied
    to the device's own resolves.  The threshold is the median of the first checkpoint's nonzero errors: without dilation the
    first freeze splits the tiles by construction (tiles at or below it stop at 16 samples, those above go on)."""
    import torch
    w, h, budget, min_samples = 160, 96, 256, 16
    sc, _ = _scene(kind, w, h, budget)
    gs = gpu.GpuScene(sc)
    count = gpu.n_tiles(w, h)
    targets = ae.schedule(budget, min_samples)
    assert targets == [8, 16, 32, 64, 128, 256]

    def loop(threshold):
        acc = gs.accumulate(SEED, budget)
        stats = torch.zeros(4, dtype=torch.int64, device=torch.device("cuda", gs.device))
        live, first_err, prev = np.ones(count, bool), None, None
        for i, t in enumerate(targets):
            acc.add(t - acc.samples, stats)
            if t == budget:
                break
            cur, _ = acc.resolve()
            if i > 0:
                err = gpu.tile_error(cur, prev, w, h)
                torch.cuda.synchronize()
                e = ae.tile_error(cur.cpu().numpy(), prev.cpu().numpy(), w, h, 0, 1, count)
                assert np.array_equal(err.cpu().numpy().view(np.uint32), e.view(np.uint32))
                first_err = e if first_err is None else first_err
                if threshold is None:
                    break
                live = ae.keep_mask(e, live, w, h, 0, 1, count, threshold, dilate)
                assert acc.freeze(mask=live) == int(live.sum())
                if not live.any():
                    break
            prev = cur
        tiles, tiles8 = acc.resolve()
        torch.cuda.synchronize()
        out = (acc.tile_samples(), tiles.cpu().numpy().view(np.uint32), tiles8.cpu().numpy(), stats.cpu().tolist(), first_err)
        acc.close()
        return out

    first = loop(None)[4]
    threshold = float(np.median(first[first > 0]))
    assert threshold > 0 and (first > threshold).any()
    counts, tiles, tiles8, st, _ = loop(threshold)
    if dilate == 0:
        assert len(set(counts.tolist())) >= 2 and counts.min() == 16 and counts.max() > 16
    acc = gs.accumulate(SEED, budget)
    ast, secs = acc.run_adaptive(threshold=threshold, min_samples=min_samples, dilate=dilate)
    at, at8 = acc.resolve()
    torch.cuda.synchronize()
    assert np.array_equal(acc.tile_samples(), counts)
    assert np.array_equal(at.cpu().numpy().view(np.uint32), tiles) and np.array_equal(at8.cpu().numpy(), tiles8)
    assert [ast[k] for k in ("rays", "casts", "tests", "samples")] == st and secs > 0
    assert ast["samples"] == sum(int(c) * int(v) for c, v in zip(counts, ae.inside_mask(w, h, 0, 1, count).sum(axis=1)))
    gs.launch_status()
    acc.close()
    # the convenience entry point gives the same frame
    img, img8, cmap, st2, _ = gs.render_adaptive(SEED, budget, threshold=threshold, min_samples=min_samples, dilate=dilate)
    assert np.array_equal(cmap.reshape(-1), counts) and st2 == ast
    gs.close()
    sc.free()


def test_bad_freezes_change_nothing(gpu):
    import torch
    from rt_amd import gpu as G
    sc, _ = _scene("room", 37, 21)
    gs = gpu.GpuScene(sc)
    acc = gs.accumulate(SEED, BUDGET)
    err = torch.zeros(acc.count, dtype=torch.float32, device=torch.device("cuda", 0))
    with pytest.raises(G.ShimError, match=r"\(-2\)"):
        acc.freeze(error=err, threshold=0.5, dilate=1)       # no sample yet
    acc.add(4)
    with pytest.raises(G.ShimError, match=r"\(-2\)"):
        acc.freeze(error=err, threshold=0.5, dilate=3)
    with pytest.raises(G.ShimError, match=r"\(-2\)"):
        acc.run_adaptive()                                   # the driver starts from an empty accumulation
    assert acc.live_tiles == acc.count and (acc.tile_samples() == 4).all()
    acc.close()
    gs.close()
    sc.free()


def _host_adaptive(sc, threshold, min_samples, dilate, counts=True, devices=1):
    """render_adaptive of the host library (include/raytracer.h) -> (largest count, framebuffer, linear, count map)"""
    import ctypes as C
    from rt_amd import abi
    host = abi.load_host()
    w, h = sc.width, sc.height
    fb, lin = np.zeros((h, w, 3), np.uint8), np.zeros((h, w, 3), np.float32)
    cmap = np.zeros(((h + 7) // 8, (w + 7) // 8), np.uint32)
    p = abi.adapt_params(threshold=threshold, min_samples=min_samples, dilate=dilate)
    opt = abi.Options()
    opt.width, opt.height, opt.samples = w, h, sc.samples
    host.rt_set_seed(SEED)
    host.rt_set_max_depth(sc.max_depth)
    host.rt_set_devices(devices)
    host.rt_set_integrator(abi.TRACE_PATH)
    most = host.render_adaptive(fb.ctypes.data, lin.ctypes.data, cmap.ctypes.data if counts else None, sc.objects, sc.n_objects,
                                sc.meshes if sc.n_meshes else None, sc.n_meshes, C.byref(sc.camera), C.byref(opt), C.byref(p), None, None)
    return most, fb, lin, cmap


@pytest.mark.parametrize("kind", ["room", "glass"])
def test_the_host_library_and_the_image_entry_point_are_the_driver(gpu, kind):
    """render_adaptive (host library) and rt_hip_render_adaptive_image against Accumulation.run_adaptive: frame, bytes, count map,
    counters"""
    import torch
    from rt_amd import abi
    w, h, budget, min_samples, dilate = 100, 60, 64, 8, 1
    sc, _ = _scene(kind, w, h, budget)
    gs = gpu.GpuScene(sc)
    acc = gs.accumulate(SEED, budget)
    acc.add(4)
    prev, _ = acc.resolve()
    acc.add(4)
    cur, _ = acc.resolve()
    err = gpu.tile_error(cur, prev, w, h).cpu().numpy()
    acc.close()
    threshold = float(np.median(err[err > 0]))
    img, img8, cmap, st, _ = gs.render_adaptive(SEED, budget, threshold=threshold, min_samples=min_samples, dilate=dilate)
    img, img8 = img.cpu().numpy(), img8.cpu().numpy()
    assert len(set(cmap.reshape(-1).tolist())) >= 2
    himg, himg8, hmap, hst, secs = gpu.adaptive_image_host(sc, SEED, budget, threshold=threshold, min_samples=min_samples, dilate=dilate)
    assert np.array_equal(himg.view(np.uint32), img.view(np.uint32)) and np.array_equal(himg8, img8)
    assert np.array_equal(hmap, cmap) and hst == st and secs > 0
    host = abi.load_host()
    rays0 = host.rt_last_ray_bounces()
    most, fb, lin, lmap = _host_adaptive(sc, threshold, min_samples, dilate)
    assert most == int(cmap.max()) and np.array_equal(lmap, cmap)
    assert np.array_equal(lin.view(np.uint32), img.view(np.uint32)) and np.array_equal(fb, img8)
    assert host.rt_last_pixel_samples() == st["samples"] and host.rt_last_ray_bounces() == st["casts"] and not host.rt_last_render_cancelled()
    most2, fb2, _, _ = _host_adaptive(sc, threshold, min_samples, dilate, counts=False)   # the count map is optional
    assert most2 == most and np.array_equal(fb2, fb)
    try:
        assert _host_adaptive(sc, threshold, min_samples, dilate, devices=2)[0] == abi.EINVAL   # one device only
    finally:
        host.rt_set_devices(1)
    gs.close()
    sc.free()


def test_a_logical_device(gpu):
    """rt_hip_render_adaptive_image(..., device = 2, ...) under the device map (0, 0, 0): device 0's frame and count map; the
    primitives on a scene of that device agree with it"""
    import ctypes as C
    from rt_amd import abi, gpu as G
    shim = abi.load_shim()
    w, h, budget = 37, 21, 32
    sc, _ = _scene("glass", w, h, budget)
    kw = dict(threshold=0.05, min_samples=8, dilate=1)
    assert shim.rt_hip_set_device_map(None, 0) == 0
    zero = gpu.adaptive_image_host(sc, SEED, budget, device=0, **kw)
    arr = (C.c_int * 3)(0, 0, 0)
    assert shim.rt_hip_set_device_map(arr, 3) == 0, shim.rt_hip_last_error()
    try:
        two = gpu.adaptive_image_host(sc, SEED, budget, device=2, **kw)
        with pytest.raises(G.ShimError, match=r"\(-1\)"):
            gpu.adaptive_image_host(sc, SEED, budget, device=3, **kw)     # beyond the map
        gs = gpu.GpuScene(sc)                                             # the primitives while the map is set
        img, img8, cmap, st, _ = gs.render_adaptive(SEED, budget, **kw)
        gs.close()
    finally:
        shim.rt_hip_set_device_map(None, 0)
    assert np.array_equal(two[0].view(np.uint32), zero[0].view(np.uint32)) and np.array_equal(two[1], zero[1])
    assert np.array_equal(two[2], zero[2]) and two[3] == zero[3]
    assert np.array_equal(img.cpu().numpy().view(np.uint32), two[0].view(np.uint32)) and np.array_equal(cmap, two[2]) and st == two[3]
    sc.free()


def test_tile_error_refuses_host_pointers(gpu):
    import torch
    from rt_amd import gpu as G
    dev = torch.device("cuda", 0)
    d = torch.zeros((1, 64, 3), dtype=torch.float32, device=dev)
    hbuf = torch.zeros((1, 64, 3), dtype=torch.float32)
    out = torch.zeros(1, dtype=torch.float32, device=dev)
    for cur, prev, o in ((hbuf, d, out), (d, hbuf, out), (d, d, torch.zeros(1))):
        with pytest.raises((G.ShimError, ValueError)):
            gpu.tile_error(cur, prev, 8, 8, out=o)
    assert gpu.tile_error(d, d, 8, 8, 0, 0, 1).cpu().tolist() == [0.0]   # stride 0 with one tile is a launch of that tile


def test_the_cli_s_adaptive_frame(gpu, tmp_path):
    """raytracer -e <threshold>: the PNG is the driver's frame byte for byte and the printed mean is its counter; -e 0 writes the
    one-shot frame; -e with -n writes the adaptive frame as <name>.noisy.png and denoises it with the budget's first-hit buffers"""
    import os
    import re
    import subprocess
    from rt_amd import abi, scene as S
    from test_gpu_denoise import _read_png
    cli = os.path.join(os.path.dirname(abi.HOST_PATH), "raytracer")
    w, h, budget, thr = 96, 64, 64, 0.05
    sc = S.build_scene(4, w, h, budget)
    gs = gpu.GpuScene(sc)
    img, img8, cmap, st, _ = gs.render_adaptive(SEED, budget, threshold=thr)
    one, one8, _ = gs.render_image(SEED, budget)

    def run(*extra, out="a.png"):
        path = str(tmp_path / out)
        r = subprocess.run([cli, "-w", str(w), "-h", str(h), "-s", str(budget), "-c", "4", "-r", str(SEED), "-d", str(sc.max_depth),
                            "-o", path, *extra], capture_output=True, text=True, timeout=120)
        return r, path
    r, path = run("-e", str(thr))
    assert r.returncode == 0, r.stdout + r.stderr
    assert np.array_equal(_read_png(path), img8.cpu().numpy())
    m = re.search(r"adaptive: threshold 0.05, mean ([0-9.]+) samples per pixel of 64, ([0-9.]+) % of the tiles", r.stdout)
    assert m and abs(float(m.group(1)) - st["samples"] / (w * h)) < 0.006
    assert abs(float(m.group(2)) - 100.0 * float((cmap >= budget).mean())) < 0.06
    assert "checkpoint: 16 of 64 samples" in r.stdout
    r0, path0 = run("-e", "0", out="zero.png")
    assert r0.returncode == 0, r0.stdout + r0.stderr
    assert np.array_equal(_read_png(path0), one8.cpu().numpy()) and "mean 64.00 samples per pixel" in r0.stdout
    rn, pathn = run("-e", str(thr), "-n", "3", out="den.png")
    assert rn.returncode == 0, rn.stdout + rn.stderr
    assert np.array_equal(_read_png(str(tmp_path / "den.noisy.png")), img8.cpu().numpy())
    assert "first-hit buffers of 64 samples" in rn.stdout
    total = gpu.n_tiles(w, h)
    aov = gs.untile_aov(gs.render_aov(SEED, budget, 0, 1, total, want=gpu.DENOISE_AOV), 0, 1, total)
    _, den8 = gpu.denoise(img, aov, w, h, iterations=3)
    assert np.array_equal(_read_png(pathn), den8.cpu().numpy())
    bad, _ = run("-e", "-1")
    assert bad.returncode != 0 and "Usage" in bad.stderr
    both, _ = run("-e", str(thr), "-p", "8")
    assert both.returncode != 0
    gs.close()
    sc.free()
