"""First-hit feature buffers without a GPU: the CPU expectation (tests/aov_expected.py) pinned on hand-built scenes whose answer
is known, and the C-ABI, host library and CLI entry points checked for their arguments and for failing loudly without a device."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np
import pytest

from aov_expected import BACKGROUND, NO_OBJECT, expected_pixels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 1666943821


def _scene(objs, meshes=None, w=16, h=12, cam=(0, 0, 10), target=(0, 0, 0)):
    from rt_amd import scene as S
    return S.custom_scene(objs, w, h, 1, 5, cam, target, meshes=meshes)


def _centre(sc):
    return (sc.height // 2) * sc.width + sc.width // 2


def test_sphere_straight_ahead(ref_mesh):
    """a sphere of radius 2 at distance 10: every sample hits it, object 0, depth a little over 8, the normal faces the camera"""
    from rt_amd import abi
    sc = _scene([dict(flags=abi.M_DEFAULT, radius=2.0, center=(0, 0, 0), color=(0.2, 0.5, 0.9))])
    e = expected_pixels(ref_mesh(5), sc, SEED, 4, [_centre(sc)])
    assert e["hits"][0] == 4 and e["object"][0] == 0
    assert 8.0 <= float(e["depth"][0]) < 8.6   # (the pixel right of and below the centre: a little off the axis)
    np.testing.assert_allclose(e["albedo"][0], np.float32([0.2, 0.5, 0.9]), rtol=1e-7)
    assert e["normal"][0][2] > 0.5 and 0.9 < np.linalg.norm(e["normal"][0]) <= 1.0 + 1e-6   # a mean of unit normals


def test_a_pixel_that_misses(ref_mesh):
    """nothing in view: BACKGROUND albedo, zero normal, +inf depth, no object"""
    from rt_amd import abi
    sc = _scene([dict(flags=abi.M_DEFAULT, radius=1.0, center=(0, 0, 40), color=(1, 1, 1))])   # behind the camera
    e = expected_pixels(ref_mesh(5), sc, SEED, 3, [0, _centre(sc)])
    assert (e["hits"] == 0).all() and (e["object"] == NO_OBJECT).all()
    assert np.isinf(e["depth"]).all() and (e["depth"] > 0).all()
    assert (e["normal"] == 0).all()
    # three times BACKGROUND, times 1/3, rounded once: what the device computes
    want = np.float32((BACKGROUND + BACKGROUND + BACKGROUND) * (1.0 / 3.0))
    assert (e["albedo"] == want).all()


def test_checkered_sphere(ref_mesh):
    """one sample per pixel on an M_CHECKERED sphere: the albedo is 0.3 or 0.7 times its colour, and both occur"""
    from rt_amd import abi
    col = (0.5, 0.25, 1.0)
    sc = _scene([dict(flags=abi.M_DEFAULT | abi.M_CHECKERED, radius=3.0, center=(0, 0, 0), color=col)], w=12, h=10)
    e = expected_pixels(ref_mesh(5), sc, SEED, 1, np.arange(12 * 10))
    hit = e["hits"] == 1
    assert hit.sum() > 20
    seen = set()
    for a in e["albedo"][hit]:
        for c in (0.3, 0.7):
            if np.array_equal(a, np.float32([col[0] * c, col[1] * c, col[2] * c])):
                seen.add(c)
                break
        else:
            raise AssertionError(f"albedo {a} is neither 0.3 nor 0.7 times {col}")
    assert seen == {0.3, 0.7}


def test_mesh_in_front_of_a_sphere(ref_mesh):
    """a triangle between the camera and a sphere: the first hit is the mesh, id n_spheres + 0, its normal the triangle's"""
    from rt_amd import abi
    objs = [dict(flags=abi.M_DEFAULT, radius=2.0, center=(0, 0, 0), color=(0.9, 0.1, 0.1)),
            dict(flags=abi.M_DEFAULT, radius=0.5, center=(30, 0, 0), color=(0.1, 0.9, 0.1))]
    tri = [[(-5.0, -5.0, 4.0), (5.0, -5.0, 4.0), (0.0, 6.0, 4.0)]]
    sc = _scene(objs, meshes=[dict(flags=abi.M_DEFAULT, color=(0.3, 0.3, 0.8), triangles=tri)])
    e = expected_pixels(ref_mesh(5), sc, SEED, 2, [_centre(sc)])
    assert e["object"][0] == 2 and e["hits"][0] == 2
    assert 6.0 <= float(e["depth"][0]) < 6.2
    np.testing.assert_allclose(e["albedo"][0], np.float32([0.3, 0.3, 0.8]), rtol=1e-7)
    assert abs(abs(float(e["normal"][0][2])) - 1.0) < 1e-6


# ---- the entry points without a device -------------------------------------------------------------------------------------

def _no_gpu():
    from rt_amd import abi
    return abi.load_shim().rt_hip_device_count() == 0


def _params(w=16, h=16, samples=1):
    from rt_amd import abi
    p = abi.RtHipParams()
    p.width, p.height, p.samples, p.seed = w, h, samples, SEED
    return p


def test_bad_arguments_rejected():
    from rt_amd import abi, scene as S
    shim = abi.load_shim()
    sc = S.build_scene(1, 16, 16, 1)
    buf = np.zeros((16, 16, 3), np.float32)
    some = abi.RtHipAov()
    some.albedo = buf.ctypes.data
    none = abi.RtHipAov()
    p = _params()
    # rt_hip_render_aov_tiles: no scene, camera or params; no output
    assert shim.rt_hip_render_aov_tiles(None, C.byref(sc.camera), C.byref(p), C.byref(some), None) == abi.EINVAL
    assert shim.rt_hip_render_aov_tiles(None, None, C.byref(p), C.byref(some), None) == abi.EINVAL
    assert shim.rt_hip_render_aov_tiles(None, C.byref(sc.camera), None, C.byref(some), None) == abi.EINVAL
    assert shim.rt_hip_render_aov_tiles(None, C.byref(sc.camera), C.byref(p), C.byref(none), None) == abi.EINVAL
    assert shim.rt_hip_render_aov_tiles(None, C.byref(sc.camera), C.byref(p), None, None) == abi.EINVAL
    # rt_hip_render_aov_image: arguments are checked before the device is looked for
    for bad in (dict(samples=0), dict(samples=-3), dict(w=1)):
        q = _params(w=bad.get("w", 16), samples=bad.get("samples", 1))
        assert shim.rt_hip_render_aov_image(sc.objects, sc.n_objects, None, 0, C.byref(sc.camera), C.byref(q), 0,
                                            C.byref(some)) == abi.EINVAL
    assert shim.rt_hip_render_aov_image(sc.objects, sc.n_objects, None, 0, C.byref(sc.camera), C.byref(p), 0,
                                        C.byref(none)) == abi.EINVAL
    assert shim.rt_hip_render_aov_image(sc.objects, sc.n_objects, None, 0, None, C.byref(p), 0, C.byref(some)) == abi.EINVAL
    assert shim.rt_hip_render_aov_image(sc.objects, sc.n_objects, None, 0, C.byref(sc.camera), None, 0, C.byref(some)) == abi.EINVAL
    # rt_hip_untile_aov: buffers and a sane size are required, the tile range must lie in the image
    assert shim.rt_hip_untile_aov(None, 16, 16, 0, 1, 1, C.byref(some), None) == abi.EINVAL
    assert shim.rt_hip_untile_aov(C.byref(some), 0, 16, 0, 1, 1, C.byref(some), None) == abi.EINVAL
    assert shim.rt_hip_untile_aov(C.byref(some), 16, 16, 3, 1, 2, C.byref(some), None) == abi.EINVAL
    assert shim.rt_hip_aov_kernel_name(None) == b""
    assert shim.rt_hip_aov_kernel_launches(-1, None) is None
    assert shim.rt_hip_aov_kernel_launches(shim.rt_hip_aov_kernel_count(), None) is None


def test_aov_forms_are_not_members_of_the_family():
    """the AOV kernels have their own list: the family (and with it the pick table and the coverage table) stays at 35"""
    from rt_amd import abi
    shim = abi.load_shim()
    assert shim.rt_hip_kernel_count() == 35
    fam = {shim.rt_hip_kernel_launches(k, None).decode() for k in range(shim.rt_hip_kernel_count())}
    aov = [shim.rt_hip_aov_kernel_launches(k, None).decode() for k in range(shim.rt_hip_aov_kernel_count())]
    assert len(aov) == 10 and len(set(aov)) == 10 and all(n.startswith("pt_aov_tiles") for n in aov)
    assert not fam & set(aov)


def test_no_device_is_an_error_not_a_fallback():
    from rt_amd import abi, scene as S
    if not _no_gpu():
        pytest.skip("a GPU is visible")
    shim = abi.load_shim()
    sc = S.build_scene(3, 16, 16, 1)
    buf = np.full((16, 16, 3), 7.0, np.float32)
    out = abi.RtHipAov()
    out.albedo = buf.ctypes.data
    meshes = sc.hip_meshes()
    rc = shim.rt_hip_render_aov_image(sc.objects, sc.n_objects, meshes, sc.n_meshes, C.byref(sc.camera), C.byref(_params()), 0,
                                      C.byref(out))
    assert rc == abi.ENODEV and b"no HIP device" in shim.rt_hip_last_error()
    assert (buf == 7.0).all()
    host = abi.load_host()
    opt = abi.Options()
    opt.width = opt.height = 16
    opt.samples = 2
    img = abi.RtAovImage()
    img.albedo = buf.ctypes.data
    assert host.render_aov(C.byref(img), sc.objects, sc.n_objects, sc.meshes, sc.n_meshes, C.byref(sc.camera), C.byref(opt)) == abi.ENODEV
    assert (buf == 7.0).all()
    sc.free()


def test_cli_feature_buffers_without_gpu_exit_loudly(tmp_path):
    if not _no_gpu():
        pytest.skip("a GPU is visible")
    cli = os.path.join(ROOT, "raytracer.c_amd", "host", "raytracer")
    prefix = str(tmp_path / "frame")
    r = subprocess.run([cli, "-w", "16", "-h", "12", "-s", "2", "-c", "1", "-o", str(tmp_path / "f.png"), "-a", prefix],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0
    assert not glob.glob(str(tmp_path / "*.pfm"))


def test_cli_lists_the_flag():
    cli = os.path.join(ROOT, "raytracer.c_amd", "host", "raytracer")
    r = subprocess.run([cli], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "-a <prefix" in r.stderr
