#!/usr/bin/env python3
"""Child process of tests/test_gpu_dir_park.py: renders one named scene with the shim RT_HIP_SHIM_PATH names -- the PT_DIAG
build, or a variant build of the A/B knob PT_DIR_PARK -- and prints one JSON line: the kernel, the frame (floats and bytes as
hex digests, so that two builds can be compared bit for bit), the four counters and, from the PT_DIAG build, the direction
rounds' and the retry stack's counters.

usage: dir_park_child.py SCENE [CHUNKS]   with SCENE in dir_park_scenes.SCENES
The PT_DIAG build counts the retry stack's two events past the 44 a caller's buffer was known to hold, and only when told that
the buffer has 64 words: RT_HIP_DIAG_PARK_COUNTS=1 (set here)."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "raytracer.c_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

SEED = 1666943821


def main():
    which = sys.argv[1]
    chunks = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    diag = "diag" in os.path.basename(os.environ.get("RT_HIP_SHIM_PATH", ""))
    if diag:
        os.environ["RT_HIP_DIAG_PARK_COUNTS"] = "1"   # read by the shim at every launch
    import torch
    from rt_amd import gpu as G
    from dir_park_scenes import SCENES
    sc = SCENES[which]()
    gs = G.GpuScene(sc)
    stats = torch.zeros(64 if diag else 4, dtype=torch.int64, device="cuda")
    total = G.n_tiles(sc.width, sc.height)
    t, t8, _ = gs.render_tiles(SEED, 0, 1, total, stats=stats, chunks=chunks)
    torch.cuda.synchronize()
    st = stats.cpu().tolist()
    rec = {"scene": which, "kernel": gs.last_launch_kernel(), "stats": st[:4],
           "frame": hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest(),
           "frame8": hashlib.sha256(t8.cpu().numpy().tobytes()).hexdigest()}
    if diag:
        d = st[4:]
        rec.update(trips=d[0], reject_rounds=d[10], reject_lanes=d[11], violations=d[12], parked=d[44], no_room=d[45])
    print(json.dumps(rec), flush=True)
    gs.close()


if __name__ == "__main__":
    main()
