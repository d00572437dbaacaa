#!/usr/bin/env python3
"""How far the rooms of tests/dir_park_scenes.py (PARK_ROWS: one all-diffuse, deep-path room per swapping pooled kernel, and
the deep glass room) drive the retry stack of the direction rounds (pt_body_pooled.h, PT_DIR_PARK): the PT_DIAG build's
counters per scene, from one child process (tests/dir_park_child.py).  tests/test_gpu_dir_park.py asserts the columns that
must not be zero; this prints them all.
usage: python tools/dir_park_reach.py [--out profiles/r11_dir_park_reach.txt]      (needs `make shim-diag`)"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
DIAG_LIB = os.path.join(ROOT, "raytracer.c_amd", "csrc", "librt_hip_diag.so")
COLUMNS = [("trips", "trips"), ("rounds", "reject_rounds"), ("parked", "parked"), ("no_room", "no_room"),
           ("swaps put off", "swaps_put_off"), ("dry drains", "dry_drains"), ("parked w. children", "parked_children")]


def main():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    from dir_park_scenes import PARK_SCENES
    assert os.path.exists(DIAG_LIB), f"{DIAG_LIB} missing: make shim-diag"
    scenes = ",".join(PARK_SCENES + ["deep_glass:0"])
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "dir_park_child.py"), scenes],
                       env=dict(os.environ, RT_HIP_SHIM_PATH=DIAG_LIB), capture_output=True, text=True, timeout=600, cwd=ROOT)
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-3000:])
        return 1
    recs = [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")]
    lines = ["retry stack of the direction rounds, PT_DIAG build, one 8 x 8 tile per scene (tests/dir_park_scenes.py):",
             "64 spp, depth 16, one chunk; deep_glass: 32 spp, depth 26, the shim's own chunk count",
             "%-32s %-13s %6s" % ("kernel", "scene", "chunks") + "".join(" %*s" % (max(9, len(h)), h) for h, _ in COLUMNS)]
    for r in recs:
        assert r["violations"] == 0, r
        lines.append("%-32s %-13s %6d" % (r["kernel"], r["scene"], r["chunks"]) +
                     "".join(" %*d" % (max(9, len(h)), r[k]) for h, k in COLUMNS))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if out:
        with open(out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
