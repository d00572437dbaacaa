"""Progressive rendering (rt_hip_accum_*, render_progressive, the CLI's -p) without a GPU: the libraries export the entry
points the headers declare, the CLI refuses bad -p arguments before it touches a device, and creating an accumulation
checks its arguments first."""
import ctypes as C
import os
import re
import subprocess

from conftest import ROOT

ACCUM = ["rt_hip_accum_create", "rt_hip_accum_add", "rt_hip_accum_add_host", "rt_hip_accum_resolve", "rt_hip_accum_read_image",
         "rt_hip_accum_samples", "rt_hip_accum_kernel", "rt_hip_accum_destroy"]


def _header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_libraries_export_and_headers_declare_the_entry_points():
    from rt_amd import abi
    shim_h, host_h = _header("rt_hip.h"), _header("raytracer.h")
    assert "typedef struct RtHipAccum RtHipAccum;" in shim_h
    for n in ACCUM:
        assert re.search(r"\b%s\s*\(" % n, shim_h), n
        assert getattr(C.CDLL(abi.SHIM_PATH), n) is not None
        assert n in abi.SHIM_SYMBOLS
    assert re.search(r"\bint\s+render_progressive\s*\(", host_h)
    assert getattr(C.CDLL(abi.HOST_PATH), "render_progressive") is not None
    abi.load_host()


def _cli(*args):
    from rt_amd import abi
    exe = os.path.join(abi.PKG_DIR, "host", "raytracer")
    return subprocess.run([exe, "-w", "32", "-h", "24", "-o", os.devnull, *args], capture_output=True, text=True, timeout=60)


def test_cli_progressive_usage_errors():
    for args in (["-s", "8", "-p", "0"], ["-s", "8", "-p", "9"], ["-s", "8", "-p", "4", "-g", "2"]):
        r = _cli(*args)
        assert r.returncode != 0, args
        assert "Usage:" in r.stderr and "-p <samples per pass" in r.stderr, (args, r.stderr)
        assert "seed =" not in r.stdout, args   # refused before anything ran


def test_accum_create_checks_its_arguments():
    from rt_amd import abi, scene as S
    shim = abi.load_shim()
    sc = S.build_scene(1, 16, 16, 1)
    p = abi.RtHipParams()
    p.width, p.height, p.samples, p.max_depth = 16, 16, 4, 4
    p.tile_first, p.tile_stride, p.tile_count = 0, 1, 4
    out = C.c_void_p(1)
    assert shim.rt_hip_accum_create(None, C.byref(sc.camera), C.byref(p), C.byref(out)) == abi.EINVAL
    assert not out.value
    assert shim.rt_hip_accum_create(None, None, C.byref(p), C.byref(out)) == abi.EINVAL
    p.samples = 0
    assert shim.rt_hip_accum_create(None, C.byref(sc.camera), C.byref(p), C.byref(out)) == abi.EINVAL
    # the other entry points refuse a NULL accumulation
    assert shim.rt_hip_accum_add(None, 1, None, None) == abi.EINVAL
    assert shim.rt_hip_accum_resolve(None, None, None, None) == abi.EINVAL
    assert shim.rt_hip_accum_read_image(None, None, None) == abi.EINVAL
    assert shim.rt_hip_accum_samples(None) == 0
    shim.rt_hip_accum_destroy(None)
    sc.free()
