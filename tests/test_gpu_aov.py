"""First-hit feature buffers on the GPU (rt_hip_render_aov_*): albedo, normal, depth, object id and hit count equal the CPU
expectation built from the compiled reference (tests/aov_expected.py) BIT FOR BIT, for every scene class of the kernel pick table,
at ragged edges and tile subsets, at the BASELINE configurations, and at the edges of the accepted range; an AOV launch takes no
pool and reports no failure; the host library's render_aov and the CLI's -a files are the same buffers.  The last test checks
that every AOV form was launched by a test that compared it."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from aov_expected import expected_image, expected_pixels, mismatch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 1666943821


def _aov_launches():
    from rt_amd import abi
    shim = abi.load_shim()
    out = {}
    for k in range(shim.rt_hip_aov_kernel_count()):
        n = C.c_uint64(0)
        out[shim.rt_hip_aov_kernel_launches(k, C.byref(n)).decode()] = n.value
    return out


@pytest.fixture
def gpu():
    import torch
    from rt_amd import abi, gpu as G
    assert abi.load_shim().rt_hip_device_count() >= 1, "no HIP device: the GPU tests must run on the GPU box"
    assert torch.cuda.is_available()
    return G


def _assert_equal(got, exp, what):
    msg = mismatch(got, exp)
    assert not msg, f"{what}: {msg}"


def _pick_classes():
    from test_gpu_parity import PICK_ROWS
    seen, out = set(), []
    for cls, _, _, _ in PICK_ROWS:
        c = {k: v for k, v in cls.items() if k != "depth"}   # max_depth is no part of an AOV launch
        key = tuple(sorted(c.items()))
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


CLASSES = _pick_classes()
FORM = {  # the AOV form a class takes (pt_aov_pick)
    "n_packed=4": "pt_aov_tiles", "n_packed=4+chk=True": "pt_aov_tiles_chk", "n_packed=4+refr=True": "pt_aov_tiles",
    "n_packed=4+chk=True+refr=True": "pt_aov_tiles_chk", "n_packed=4+glass2=True": "pt_aov_tiles",
}


@pytest.mark.parametrize("cls", CLASSES, ids=["+".join(f"{a}={b}" for a, b in c.items()) for c in CLASSES])
def test_every_scene_class_equals_the_reference(gpu, ref_mesh, cls):
    from util import class_scene
    sc = class_scene(**cls, width=48, height=32, samples=3)
    gs = gpu.GpuScene(sc)
    got = gs.aov_image(SEED, 3)
    name = gs.aov_kernel_name()
    key = "+".join(f"{a}={b}" for a, b in cls.items())
    if key in FORM:
        assert name == FORM[key]
    _assert_equal(got, expected_image(ref_mesh(5), sc, SEED, 3), f"{name} {cls}")
    gs.close()
    sc.free()


@pytest.mark.parametrize("cls", [dict(n_packed=4), dict(n_packed=4, tris=40, mesh_chk=True), dict(n_packed=4, tris=400, chk=True),
                                 dict(n_packed=300, tris=60)], ids=["spheres", "flat_mesh_chk", "hierarchy_chk", "mem"])
def test_ragged_image_and_tile_subsets(gpu, ref_mesh, cls):
    """37 x 21 (ragged in both directions): launches of tile subsets give the full launch's tiles, pixels outside the image read 0
    (object 0xFFFFFFFF), and rt_hip_untile_aov puts every subset's tiles in their places"""
    import torch
    from rt_amd import abi
    from util import class_scene
    W, H, S = 37, 21, 2
    sc = class_scene(**cls, width=W, height=H, samples=S)
    gs = gpu.GpuScene(sc)
    total = gpu.n_tiles(W, H)
    full = gs.render_aov(SEED, S)
    torch.cuda.synchronize()
    tx = (W + 7) // 8
    for t in range(total):   # the ragged tiles' outside pixels
        for pit in range(64):
            x, y = (t % tx) * 8 + (pit & 7), (t // tx) * 8 + (pit >> 3)
            if x >= W or y >= H:
                assert full["object"][t, pit].item() == -1 and full["hits"][t, pit].item() == 0
                assert full["depth"][t, pit].item() == 0 and (full["albedo"][t, pit] == 0).all() and (full["normal"][t, pit] == 0).all()
    img = {f: np.zeros((H, W, 3) if abi.AOV_CHANNELS[f] == 3 else (H, W), np.uint32) for f in abi.AOV_FIELDS}
    for first, stride, count in ((1, 3, (total - 1 + 2) // 3), (0, 3, (total + 2) // 3), (2, 3, (total - 2 + 2) // 3),
                                 (0, 1, 5), (4, 2, 3), (total - 1, 1, 1)):
        part = gs.render_aov(SEED, S, first, stride, count)
        torch.cuda.synchronize()
        for f in abi.AOV_FIELDS:
            a, b = part[f][:count].cpu().numpy(), full[f][first:first + stride * count:stride].cpu().numpy()
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (f, first, stride, count)
        if stride == 3:
            sub = gs.untile_aov(part, first, stride, count)
            torch.cuda.synchronize()
            for f in abi.AOV_FIELDS:
                img[f] |= sub[f].cpu().numpy().view(np.uint32)   # disjoint tile sets; zeros elsewhere
    got = {f: img[f].view(np.float32) if f in ("albedo", "normal", "depth") else img[f] for f in abi.AOV_FIELDS}
    _assert_equal(got, gs.aov_image(SEED, S), f"untiled subsets {cls}")
    _assert_equal(got, expected_image(ref_mesh(5), sc, SEED, S), f"ragged {cls}")
    gs.close()
    sc.free()


def _sample_pixels(w, h, n, rng):
    """about n pixels: whole edge tiles (the last column and row of tiles, the first tile) and random ones"""
    tx, ty = (w + 7) // 8, (h + 7) // 8
    pix = set()
    for t in (0, tx - 1, (ty - 1) * tx, tx * ty - 1, (ty // 2) * tx + tx - 1):
        for pit in range(64):
            x, y = (t % tx) * 8 + (pit & 7), (t // tx) * 8 + (pit >> 3)
            if x < w and y < h:
                pix.add(y * w + x)
    while len(pix) < n:
        pix.add(int(rng.integers(0, w * h)))
    return np.array(sorted(pix))


@pytest.mark.parametrize("config", [1, 2, 3, 4, 5])
def test_baseline_configurations(gpu, ref_mesh, config):
    """each BASELINE configuration at its own size (config 5 at 4K), 4 samples: about 2,000 pixels, edge tiles included"""
    from rt_amd import scene as S
    sc = S.build_scene(config, samples=4)
    gs = gpu.GpuScene(sc)
    got = gs.aov_image(SEED, 4)
    pix = _sample_pixels(sc.width, sc.height, 2000, np.random.default_rng(config))
    exp = expected_pixels(ref_mesh(5), sc, SEED, 4, pix)
    flat = {f: (a.reshape(-1, 3) if a.ndim == 3 else a.reshape(-1))[pix] for f, a in got.items()}
    _assert_equal(flat, exp, f"config {config} ({gs.aov_kernel_name()})")
    assert flat["hits"].max() == 4
    gs.close()
    sc.free()


def test_range_edges(gpu, ref_mesh):
    """a camera inside a sphere (every sample hits it from within), a floor of radius 1e19 (wide range: the scalar-load forms),
    and 1,024 samples per pixel on a 16 x 16 image"""
    from rt_amd import abi, scene as S
    from util import class_scene
    inside = S.custom_scene([dict(flags=abi.M_DEFAULT | abi.M_CHECKERED, radius=5.0, center=(0, 0, 0), color=(0.9, 0.6, 0.3)),
                             dict(flags=abi.M_DEFAULT, radius=1.0, center=(0.5, 0.2, -3.0), color=(0.2, 0.8, 0.4))],
                            24, 16, 1, 5, (0.3, 0.1, 1.0), (0, 0, -1))
    wide = class_scene(n_packed=4, wide=True, chk=True, width=24, height=16)
    deep = class_scene(n_packed=4, chk=True, width=16, height=16)
    for sc, samples, what in ((inside, 5, "camera inside a sphere"), (wide, 3, "wide-range floor"), (deep, 1024, "1024 spp")):
        gs = gpu.GpuScene(sc)
        got = gs.aov_image(SEED, samples)
        if sc is inside:
            assert (got["hits"] == samples).all()
        if sc is wide:
            assert gs.aov_kernel_name() == "pt_aov_tiles_big_chk"
        _assert_equal(got, expected_image(ref_mesh(5), sc, SEED, samples), what)
        gs.close()


def test_an_aov_launch_takes_no_pool_and_reports_no_failure(gpu, ref_mesh):
    """a glass mesh through the hierarchy: its beauty launches need the pending-ray pool and the parked-walk workspace; the AOV
    launch takes neither (rt_hip_pool_bytes unchanged), leaves the status word at 0, and rejects samples < 1"""
    import torch
    from rt_amd import abi
    from util import class_scene
    shim = abi.load_shim()
    shim.rt_hip_release_cache()
    sc = class_scene(n_packed=4, tris=400, mesh_refr=True, width=40, height=24, samples=2)
    gs = gpu.GpuScene(sc)
    gs.launch_status()
    park, pend = C.c_size_t(0), C.c_size_t(0)
    assert shim.rt_hip_pool_bytes(0, C.byref(park), C.byref(pend)) == 0
    before = (park.value, pend.value)
    got = gs.aov_image(SEED, 2)
    torch.cuda.synchronize()
    assert shim.rt_hip_pool_bytes(0, C.byref(park), C.byref(pend)) == 0
    assert (park.value, pend.value) == before
    flags = C.c_uint32(7)
    assert shim.rt_hip_launch_status(0, C.byref(flags)) == 0 and flags.value == 0
    assert gs.aov_kernel_name() == "pt_aov_tiles_tri_big"
    _assert_equal(got, expected_image(ref_mesh(5), sc, SEED, 2), "glass mesh")
    p = gs.params(SEED, 0, 1, 1, 1)
    p.samples = 0
    out = abi.RtHipAov()
    buf = torch.zeros(192, device="cuda")
    out.albedo = buf.data_ptr()
    assert shim.rt_hip_render_aov_tiles(gs.handle, C.byref(sc.camera), C.byref(p), C.byref(out), None) == abi.EINVAL
    assert shim.rt_hip_render_aov_tiles(gs.handle, C.byref(sc.camera), C.byref(gs.params(SEED, 0, 1, 1, 1)), C.byref(abi.RtHipAov()),
                                        None) == abi.EINVAL
    gs.close()


def _read_pfm(path):
    with open(path, "rb") as f:
        kind = f.readline().strip()
        w, h = map(int, f.readline().split())
        scale = float(f.readline())
        assert scale < 0   # little-endian
        ch = 3 if kind == b"PF" else 1
        a = np.frombuffer(f.read(), dtype="<f4")
    assert a.size == w * h * ch
    a = a.reshape((h, w, ch) if ch == 3 else (h, w))
    return a[::-1]   # PFM rows run bottom to top


def test_host_library_and_cli_equal_the_python_buffers(gpu, tmp_path):
    """render_aov through libraytracer_amd.so, rt_hip_render_aov_image, and the CLI's -a PFM files hold GpuScene.aov_image's
    buffers bit for bit (the CLI: the frame's own samples and seed; the PFMs show the PNG's picture)"""
    from rt_amd import abi, scene as S
    w, h, spp = 40, 24, 3
    sc = S.build_scene(3, w, h, spp)
    gs = gpu.GpuScene(sc)
    want = gs.aov_image(SEED, spp)
    host = abi.load_host()
    host.rt_set_seed(SEED)
    opt = abi.Options()
    opt.width, opt.height, opt.samples = w, h, spp
    got = {f: np.zeros((h, w, 3) if abi.AOV_CHANNELS[f] == 3 else (h, w), np.float32 if f in ("albedo", "normal", "depth") else np.uint32)
           for f in abi.AOV_FIELDS}
    img = abi.RtAovImage()
    img.albedo, img.normal, img.depth = got["albedo"].ctypes.data, got["normal"].ctypes.data, got["depth"].ctypes.data
    img.object_id, img.hits = got["object"].ctypes.data, got["hits"].ctypes.data
    assert host.render_aov(C.byref(img), sc.objects, sc.n_objects, sc.meshes, sc.n_meshes, C.byref(sc.camera), C.byref(opt)) == spp
    _assert_equal(got, want, "render_aov")
    _assert_equal(gpu.aov_image_host(sc, SEED, spp), want, "rt_hip_render_aov_image")
    cli = os.path.join(ROOT, "raytracer.c_amd", "host", "raytracer")
    prefix = str(tmp_path / "frame")
    r = subprocess.run([cli, "-w", str(w), "-h", str(h), "-s", str(spp), "-c", "3", "-r", str(SEED), "-o", str(tmp_path / "f.png"),
                        "-a", prefix], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    for f in ("albedo", "normal", "depth"):
        a = _read_pfm(f"{prefix}_{f}.pfm")
        assert np.array_equal(a.view(np.uint32), want[f].view(np.uint32)), f
    gs.close()
    sc.free()


from util import AOV_FORM_CLASSES as FORM_CLASSES   # one scene class per AOV form (pt_aov_pick)


def test_zz_every_aov_form_was_compared(gpu, ref_mesh):
    """last in this file: every AOV form (rt_hip_aov_kernel_launches) is launched, and its launch counted, by a comparison that
    passes -- one scene of its class each, whole buffers against the reference"""
    from rt_amd import abi
    from util import class_scene
    shim = abi.load_shim()
    forms = [shim.rt_hip_aov_kernel_launches(k, None).decode() for k in range(shim.rt_hip_aov_kernel_count())]
    assert sorted(forms) == sorted(f for f, _ in FORM_CLASSES)
    for form, cls in FORM_CLASSES:
        k = forms.index(form)
        before, after = C.c_uint64(0), C.c_uint64(0)
        shim.rt_hip_aov_kernel_launches(k, C.byref(before))
        sc = class_scene(**cls, width=24, height=16, samples=2)
        gs = gpu.GpuScene(sc)
        assert gs.aov_kernel_name() == form, cls
        got = gs.aov_image(SEED, 2)
        shim.rt_hip_aov_kernel_launches(k, C.byref(after))
        assert after.value == before.value + 1, form
        _assert_equal(got, expected_image(ref_mesh(5), sc, SEED, 2), form)
        print(f"{form:28s} launches {after.value:4d}  compared on {cls}")
        gs.close()
        sc.free()
