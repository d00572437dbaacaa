"""Phase 1 of the small spheres on the fp16 matrix pipe (pt_filter.h, filter_mfma16; PT_MFMA16).

The filter only removes candidates that the exact test would reject, so nothing it does may show: the shipped build and the
build whose every sphere goes through the packed-fp32 loop (-DPT_MFMA16=0, `make shim-mfma0`) must agree bit for bit in the
float tiles, the byte tiles and the four counters -- on scenes with 31, 32, 33 and 38 small spheres behind the six walls (one
short of the 32-row matrix tile, which keeps the scene on the packed loop; exactly the tile; one and six spheres past it), each
at 64 x 64, at a ragged 70 x 35 and on a tile subset (first 3, stride 5), 8 spp.  And the PT_DIAG build, which puts every
dropped primitive through the exact test, must count no violation on config 4's scene, on 32 spheres of radius 1e-3 on a grid
and on 32 spheres tangent to the walls (64 x 64, 4 spp, depth 16).  The same build counts the trips whose small spheres went
through the matrix pipe: more than none on every scene with 32 small spheres or more, none with 31 -- selection happens inside
the kernel, so this is how the tests know which form they compared.  And its twin with -DPT_MFMA16=0 (`make shim-diag-mfma0`)
counts the packed loop's candidates on the same rays: what the matrix form keeps beyond them stays below 2 % of config 4's filter
evaluations (more, and phase 2 eats what phase 1 saves).

The EDGE scenes of tests/mfma16_child.py (edge_scenes: 64 x 64, 8 spp for frames, 4 spp under PT_DIAG, depth 16) take the same three
statements to where the prologue's selection rule changes its answer and away from config 4's operating point.  The matrix pipe must
run (0 < matrix_trips < trips) with no violation, and shipped must equal packed, on: the room scaled by 1/8 about the origin (near_R
16.5; 1/8 is the smallest power of two that leaves the walls wall-sized), the camera placed for near_R in [247.5, 250], the origin near
a corner of the room, no walls with 32 and with 64 small spheres (mf_first = 0), floor and ceiling only (n_big 2), two walls listed
behind the rows (n_big 4, the walls at mf_first + 32 and + 33), 64 spheres with six walls, rows on the axes, at the origin, concentric
and identical -- and on the family's other member whose body has the filter, pt_render_tiles_chk (one checkered sphere; the family
table gives MFMA_FILT to pt_render_tiles and pt_render_tiles_chk alone).  It must NOT run (matrix_trips == 0), with the same frames and
no violation, on: near_R in (250, 252.5], five leading walls (n_big 4: the fifth is row 0), a wall-sized sphere amid the rows, 65
spheres, no walls and 31 small spheres.  Four of them -- scaled 1/8, near_R under 250, no walls 32, five walls -- also meet the CPU oracle
through util.assert_parity, so these operating points are compared with the reference and not only with a sibling build.

Each build renders the whole list in ONE child process (RT_HIP_SHIM_PATH); the lists are rendered once per module."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import mfma16_child as CH
from conftest import SEED
from util import assert_parity, fixed_point_floor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raytracer.c_amd", "csrc")
LIBS = {"shipped": os.path.join(CSRC, "librt_hip.so"), "packed": os.path.join(CSRC, "variants", "librt_hip_mfma0.so"),
        "diag": os.path.join(CSRC, "librt_hip_diag.so"), "diag_packed": os.path.join(CSRC, "variants", "librt_hip_diag_mfma0.so")}

_RUNS = {}


def _run(lib, mode):
    if (lib, mode) not in _RUNS:
        assert os.path.exists(LIBS[lib]), f"{LIBS[lib]} is not built (make all)"
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mfma16_child.py"), mode],
                           env=dict(os.environ, RT_HIP_SHIM_PATH=LIBS[lib]), capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
        _RUNS[(lib, mode)] = {r["scene"]: r for r in (json.loads(l) for l in p.stdout.splitlines() if l.startswith("{"))}
    return _RUNS[(lib, mode)]


SIZES = ["64x64", "70x35", "64x64 subset"]


@pytest.mark.gpu
@pytest.mark.parametrize("n_small", [31, 32, 33, 38])
def test_matrix_filter_matches_packed_filter(n_small):
    a, b = _run("shipped", "frames"), _run("packed", "frames")
    for size in SIZES:
        name = f"{n_small} small {size}"
        assert a[name]["kernel"] == b[name]["kernel"] == "pt_render_tiles"
        assert a[name]["n"] == n_small + 6
        assert a[name]["counters"] == b[name]["counters"], f"{name}: rays, casts, tests or samples differ"
        assert a[name]["tiles"] == b[name]["tiles"], f"{name}: float tiles differ"
        assert a[name]["tiles8"] == b[name]["tiles8"], f"{name}: byte tiles differ"
        assert a[name]["counters"][0] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["config 4 64x64", "tiny grid", "tangent"])
def test_matrix_filter_matches_on_edge_scenes(scene):
    a, b = _run("shipped", "frames")[scene], _run("packed", "frames")[scene]
    assert a["kernel"] == b["kernel"] == "pt_render_tiles"
    assert (a["counters"], a["tiles"], a["tiles8"]) == (b["counters"], b["tiles"], b["tiles8"])


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["config 4", "tiny grid", "tangent"])
def test_matrix_filter_drops_nothing_the_exact_test_accepts(scene):
    r = _run("diag", "diag")[scene]
    assert r["kernel"] == "pt_render_tiles"
    print(scene, r)
    assert r["filter_evals"] > 100000 and 0 < r["candidates"] < r["filter_evals"], "the check was vacuous"
    assert r["violations"] == 0
    assert 0 < r["matrix_trips"] < r["trips"], "the matrix pipe did not run: the scene fell back to the packed loop"


@pytest.mark.gpu
@pytest.mark.parametrize("n_small, on", [(31, False), (32, True), (33, True), (38, True)])
def test_matrix_filter_is_selected_from_32_small_spheres_on(n_small, on):
    a, b = _run("diag", "diag")[f"{n_small} small"], _run("diag_packed", "diag")[f"{n_small} small"]
    print(n_small, a, b)
    assert a["kernel"] == b["kernel"] == "pt_render_tiles" and a["n"] == n_small + 6
    assert (a["matrix_trips"] > 0) == on and b["matrix_trips"] == 0
    assert a["violations"] == b["violations"] == 0
    assert (a["counters"], a["tiles"], a["tiles8"], a["trips"], a["filter_evals"]) == (b["counters"], b["tiles"], b["tiles8"], b["trips"], b["filter_evals"])
    if not on:
        assert a["candidates"] == b["candidates"]


@pytest.mark.gpu
def test_matrix_filter_keeps_few_candidates_the_packed_filter_drops():
    a, b = _run("diag", "diag")["config 4"], _run("diag_packed", "diag")["config 4"]
    assert a["matrix_trips"] > 0 and b["matrix_trips"] == 0 and b["violations"] == 0
    assert (a["counters"], a["tiles"], a["filter_evals"]) == (b["counters"], b["tiles"], b["filter_evals"]), "the two builds did not filter the same rays"
    share = (a["candidates"] - b["candidates"]) / a["filter_evals"]
    print("config 4: candidates %d (matrix) vs %d (packed) of %d filter evaluations: %.4f %%" % (a["candidates"], b["candidates"], a["filter_evals"], 100 * share))
    assert share < 0.02


EDGES = CH.edge_scenes()


@pytest.fixture(scope="module")
def gpu():
    import torch
    from rt_amd import abi, gpu as G
    assert abi.load_shim().rt_hip_device_count() >= 1, "no HIP device: the GPU tests must run on the GPU box"
    assert torch.cuda.is_available()
    return G


@pytest.mark.gpu
@pytest.mark.parametrize("scene", list(EDGES))
def test_matrix_filter_on_the_edges_of_its_selection_rule(scene):
    e = EDGES[scene]
    a, b, d, dp = _run("shipped", "frames")[scene], _run("packed", "frames")[scene], _run("diag", "diag")[scene], _run("diag_packed", "diag")[scene]
    print(scene, d)
    assert a["kernel"] == b["kernel"] == d["kernel"] and (e["kernel"] is None or a["kernel"] == e["kernel"])
    assert a["n"] == len(e["objs"]) and a["n_big"] == e["n_big"]
    assert (a["counters"], a["tiles"], a["tiles8"]) == (b["counters"], b["tiles"], b["tiles8"]), f"{scene}: shipped and packed frames differ"
    assert a["counters"][0] > 0
    assert d["violations"] == dp["violations"] == 0
    assert d["filter_evals"] > 10000 and 0 < d["candidates"] < d["filter_evals"], "the check was vacuous"
    assert (d["counters"], d["tiles"], d["trips"], d["filter_evals"]) == (dp["counters"], dp["tiles"], dp["trips"], dp["filter_evals"])
    assert dp["matrix_trips"] == 0
    if e["on"]:
        assert 0 < d["matrix_trips"] < d["trips"], "the matrix pipe did not run: the scene fell back to the packed loop"
        print("%s (%s, near_R %.2f): candidates %d (matrix) vs %d (packed) of %d filter evaluations: %.4f %%"
              % (scene, d["kernel"], d["near_R"], d["candidates"], dp["candidates"], d["filter_evals"], 100.0 * (d["candidates"] - dp["candidates"]) / d["filter_evals"]))
    else:
        assert d["matrix_trips"] == 0, "the matrix pipe ran on a scene it must leave to the packed loop"
        assert d["candidates"] == dp["candidates"]


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["scaled 1/8", "near_R under 250", "no walls 32", "five walls"])
def test_edge_scenes_meet_the_oracle(gpu, pt, scene):
    sc, e = CH.edge_scene(scene, 8)
    mean, rgb8, ost = pt.render_pixels(sc, SEED)
    gs = gpu.GpuScene(sc)
    CH.check_edge(gs, e)
    img, img8, st = gs.render_image(SEED)
    assert gs.last_launch_kernel() == "pt_render_tiles" and gs.launch_status() == 0
    assert_parity(img.cpu().numpy(), img8.cpu().numpy(), st, mean, rgb8, ost, what=scene, hdr=True, abs_floor=fixed_point_floor(sc))
    gs.close()
