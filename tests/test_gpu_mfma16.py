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

Each build renders the whole list in ONE child process (RT_HIP_SHIM_PATH); the lists are rendered once per module."""
import json
import os
import subprocess
import sys

import pytest

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
