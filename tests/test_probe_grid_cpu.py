"""Probe grids without a GPU: the vectorised restatement of the shade (tests/probe_grid_expected.py) against the scalar one, bit for
bit, and every refusal of rt_hip_probe_shade and its siblings -- arguments are checked before a device is looked for, so each comes
back RT_HIP_EINVAL on a machine that has none."""
import ctypes as C

import numpy as np
import pytest

import probe_grid_expected as PG
from rt_amd import abi

OK, EINVAL = 0, -2
PTR = C.c_void_p(0x1000)   # a pointer that is not NULL: no refused call reads it


def bits(a, dtype):
    a = np.ascontiguousarray(np.asarray(a, dtype=dtype))
    return a.view(np.uint64 if dtype == np.float64 else np.uint32)


def same(a, b, dtype):
    """equal bit for bit, any NaN equal to any NaN"""
    a, b = np.asarray(a, dtype=dtype), np.asarray(b, dtype=dtype)
    nan = np.isnan(a) & np.isnan(b)
    return bool(((bits(a, dtype) == bits(b, dtype)) | nan).all())


@pytest.mark.parametrize("count", PG.COUNTS)
@pytest.mark.parametrize("flags", (0, PG.FACING))
def test_vectorised_equals_scalar(count, flags):
    grid = PG.Grid(count=count, flags=flags)
    coeff = PG.coefficients(grid)
    m = 500
    p, n = PG.entries(grid, m)
    rng = np.random.default_rng(3)
    status = np.ones(m, dtype=np.uint32)
    status[5::17] = 0
    status[9::23] = 2
    p[11::29, 1] = np.nan
    n[13::31, 2] = np.inf
    albedo = rng.random((m, 3)).astype(np.float32)
    add = rng.random((m, 3)).astype(np.float32)
    for st, al, ad in ((status, albedo, add), (None, None, None), (status, None, add)):
        E, color = PG.shade(grid, coeff, p, n, st, al, ad)
        for i in range(m):
            Es, cs = PG.shade_scalar(grid, coeff, p[i], n[i], None if st is None else st[i], None if al is None else al[i],
                                     None if ad is None else ad[i])
            assert same(E[i], Es, np.float64), (i, E[i], Es)
            assert same(color[i], cs, np.float32), (i, color[i], cs)
    # every class occurs
    assert (status != 1).any() and np.isnan(E).any() and np.isfinite(E).any()


@pytest.mark.parametrize("count", PG.COUNTS)
def test_the_shared_entries_hold_a_uniform_wave_and_a_straddling_one(count):
    """what tests/test_gpu_probe_grid.py relies on to reach both arms of the kernel: entries [k, k + 64), k a multiple of 64, lie in one
    cell with per-lane fractions (an interior cell where the grid has one), and entries [k + 64, k + 128) alternate between two cells
    where an axis has at least 3 probes"""
    grid = PG.Grid(count=count)
    p, _ = PG.entries(grid, 1000)
    one, two = PG.wave_runs(grid)
    assert one % 64 == 0 and two == one + 64 and two + 64 <= 257
    cells = PG._cells(grid, p)
    cell = np.stack([cells[a][0] for a in range(3)], axis=1)
    frac = np.stack([cells[a][3] for a in range(3)], axis=1)
    assert (cell[one:two] == cell[one]).all()
    assert cell[one].tolist() == [(N - 1) // 2 if N >= 2 else 0 for N in count]
    for a in range(3):
        if count[a] >= 2:
            assert len(set(frac[one:two, a].tolist())) == 64 and (frac[one:two, a] > 0).all() and (frac[one:two, a] < 1).all()
    if max(count) >= 3:
        a = [k for k in range(3) if count[k] >= 3][0]
        assert (cell[two:two + 64:2] == cell[one]).all() and (cell[two + 1:two + 64:2, a] == cell[one, a] - 1).all()


def test_positions_formula():
    grid = PG.Grid(count=(2, 3, 4))
    pos = PG.positions(grid)
    assert pos.shape == (24, 3)
    assert pos[(3 * 3 + 2) * 2 + 1].tolist() == [PG.ORIGIN[0] + 1.0 * PG.STEP[0], PG.ORIGIN[1] + 2.0 * PG.STEP[1], PG.ORIGIN[2] + 3.0 * PG.STEP[2]]


def good_grid():
    return PG.Grid(count=(2, 3, 4)).abi()


def shade_rc(grid, coeff=PTR, points=PTR, normals=PTR, m=4, irradiance=PTR, color=PTR):
    return abi.load_shim().rt_hip_probe_shade(C.byref(grid), coeff, points, normals, None, None, None, m, irradiance, color, None)


BAD_GRIDS = {
    "struct_size": lambda g: setattr(g, "struct_size", C.sizeof(abi.RtHipProbeGrid) - 1),
    "flags": lambda g: setattr(g, "flags", 2),
    "reserved": lambda g: setattr(g, "reserved", 1),
    "step_zero": lambda g: g.step.__setitem__(1, 0.0),
    "step_negative": lambda g: g.step.__setitem__(0, -0.1),
    "step_nan": lambda g: g.step.__setitem__(2, float("nan")),
    "step_inf": lambda g: g.step.__setitem__(2, float("inf")),
    "origin_nan": lambda g: g.origin.__setitem__(0, float("nan")),
    "origin_inf": lambda g: g.origin.__setitem__(1, float("-inf")),
    "count_zero": lambda g: g.count.__setitem__(2, 0),
    "count_product": lambda g: [g.count.__setitem__(a, v) for a, v in enumerate((4097, 4096, 1))],
    "count_wraps": lambda g: [g.count.__setitem__(a, v) for a, v in enumerate((65536, 65536, 65536))],
    "miss_color_nan": lambda g: g.miss_color.__setitem__(1, float("nan")),
    "miss_color_inf": lambda g: g.miss_color.__setitem__(2, float("inf")),
}


@pytest.mark.parametrize("what", sorted(BAD_GRIDS))
def test_bad_grid_is_einval_everywhere(what):
    shim = abi.load_shim()
    g = good_grid()
    BAD_GRIDS[what](g)
    assert shade_rc(g) == EINVAL, shim.rt_hip_last_error()
    assert shade_rc(g, m=0) == EINVAL
    assert shim.rt_hip_probe_grid_positions(C.byref(g), PTR, None) == EINVAL
    assert shim.rt_hip_probe_grid_workspace_bytes(C.byref(g), 1024) == 0
    p = abi.probe_params(abi.PROBE_SPHERE, 4, 1)
    assert shim.rt_hip_bake_probe_grid(PTR, C.byref(g), C.byref(p), 1024, PTR, PTR, None, None, None, None) == EINVAL
    cam = abi.Camera()
    assert shim.rt_hip_probe_preview(PTR, C.byref(cam), C.byref(g), PTR, 32, 24, 1, 0, PTR, PTR, None, None) == EINVAL


def test_grid_at_the_limit_passes_the_checks():
    g = good_grid()
    for a, v in enumerate((4096, 4096, 1)):
        g.count[a] = v
    assert shade_rc(g, m=0) == OK
    assert abi.load_shim().rt_hip_probe_grid_workspace_bytes(C.byref(g), 1024) > 24 * (1 << 24)


@pytest.mark.parametrize("null", ("grid", "coeff", "points", "normals", "both outputs"))
def test_null_pointers_are_einval(null):
    shim = abi.load_shim()
    g = good_grid()
    if null == "grid":
        rc = shim.rt_hip_probe_shade(None, PTR, PTR, PTR, None, None, None, 4, PTR, PTR, None)
    elif null == "both outputs":
        rc = shade_rc(g, irradiance=None, color=None)
    else:
        rc = shade_rc(g, **{null: None})
    assert rc == EINVAL, shim.rt_hip_last_error()


@pytest.mark.parametrize("m", (1 << 32, (1 << 32) + 5, (1 << 64) - 1))
def test_too_many_entries_is_einval(m):
    assert shade_rc(good_grid(), m=m) == EINVAL


def test_no_entries_is_ok_without_a_device():
    g = good_grid()
    assert shade_rc(g, m=0) == OK
    assert shade_rc(g, m=0, irradiance=None) == OK
    g.flags = abi.GRID_FACING
    assert shade_rc(g, m=0, color=None) == OK


def test_defaults():
    g = abi.RtHipProbeGrid()
    abi.load_shim().rt_hip_probe_grid_defaults(C.byref(g))
    assert g.struct_size == C.sizeof(abi.RtHipProbeGrid) == 88 and g.flags == 0 and g.reserved == 0
    assert list(g.origin) == [0.0] * 3 and list(g.step) == [1.0] * 3 and list(g.count) == [1] * 3
    assert [np.float32(c) for c in g.miss_color] == [np.float32(10.0 / 255.0)] * 3


def test_bake_and_preview_refusals():
    shim = abi.load_shim()
    g = good_grid()
    hemi = abi.probe_params(abi.PROBE_HEMISPHERE, 4, 1)
    assert shim.rt_hip_bake_probe_grid(PTR, C.byref(g), C.byref(hemi), 1024, PTR, PTR, None, None, None, None) == EINVAL
    p = abi.probe_params(abi.PROBE_SPHERE, 4, 1)
    assert shim.rt_hip_bake_probe_grid(PTR, C.byref(g), C.byref(p), 0, PTR, PTR, None, None, None, None) == EINVAL
    assert shim.rt_hip_bake_probe_grid(None, C.byref(g), C.byref(p), 1024, PTR, PTR, None, None, None, None) == EINVAL
    assert shim.rt_hip_bake_probe_grid(PTR, C.byref(g), C.byref(p), 1024, C.c_void_p(0x1008), PTR, None, None, None, None) == EINVAL
    assert shim.rt_hip_probe_grid_workspace_bytes(C.byref(g), 0) == 0
    assert shim.rt_hip_probe_grid_workspace_bytes(C.byref(g), 96) == shim.rt_hip_probe_workspace_bytes(24, abi.PROBE_SPHERE, 96) + 768
    cam = abi.Camera()
    for w, h, spp, rgb in ((1, 24, 1, PTR), (32, 24, 0, PTR), (32, 24, 1, None)):
        assert shim.rt_hip_probe_preview(PTR, C.byref(cam), C.byref(g), PTR, w, h, spp, 0, PTR, rgb, None, None) == EINVAL
    # the host form on a scene the caller holds: its arguments before its scene
    assert shim.rt_hip_probe_preview_scene_image(None, C.byref(cam), C.byref(g), C.byref(p), 32, 24, 1, PTR, PTR, None, None) == EINVAL
    assert shim.rt_hip_probe_preview_scene_image(PTR, C.byref(cam), C.byref(g), C.byref(p), 32, 24, 1, None, None, None, None) == EINVAL
    assert shim.rt_hip_probe_preview_scene_image(PTR, C.byref(cam), C.byref(g), C.byref(hemi), 32, 24, 1, PTR, PTR, None, None) == EINVAL
    assert shim.rt_hip_probe_preview_workspace_bytes(None, 1, 24) == 0
    assert shim.rt_hip_probe_preview_workspace_bytes(None, 32, 24) >= 32 * 24 * (16 + 8 + 48 + 36)
