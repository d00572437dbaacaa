#!/usr/bin/env python3
"""Child process of tests/test_gpu_dir_park.py and tools/dir_park_reach.py: renders the named scenes, one after the other,
with the shim RT_HIP_SHIM_PATH names -- the PT_DIAG build, a variant build of the A/B knob PT_DIR_PARK, or the shipped
library -- and prints one JSON line per scene: the kernel, the frame (floats and bytes as hex digests, so that two builds
can be compared bit for bit), the four counters and, from the PT_DIAG build, the direction rounds' and the retry stack's counters.

usage: dir_park_child.py SCENE[:CHUNKS][,SCENE[:CHUNKS]...] [CHUNKS]   with every SCENE in dir_park_scenes.SCENES
       (CHUNKS after the list: for every scene that names none, default 1; 0: whatever GpuScene.suggest_chunks answers for
       the scene's own samples and depth)
The PT_DIAG build counts the retry stack's events past the 44 slots a caller's buffer was known to hold, and only when told
that the buffer has 64 words: RT_HIP_DIAG_PARK_COUNTS=1 (set here).  Slots (stats[4 + slot]):
  44 parked            paths written to the retry stack
  45 no_room           retries that found no room on the list and were carried in their lane
  46 swaps_put_off     trips with idle lanes and jobs left in the pool whose swap waited for the stack to shrink
  47 dry_drains        trips that ran with no busy lane, for the stack's retries alone
  48 parked_children   M_REFRACTION forms: paths written to the retry stack with pending second children (stack_n > 0)"""
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
    default_chunks = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    diag = "diag" in os.path.basename(os.environ.get("RT_HIP_SHIM_PATH", ""))
    if diag:
        os.environ["RT_HIP_DIAG_PARK_COUNTS"] = "1"   # read by the shim at every launch
    import torch
    from rt_amd import gpu as G
    from dir_park_scenes import SCENES
    for item in which.split(","):
        name, _, own = item.partition(":")
        chunks = int(own) if own else default_chunks
        sc = SCENES[name]()
        gs = G.GpuScene(sc)
        stats = torch.zeros(64 if diag else 4, dtype=torch.int64, device="cuda")
        total = G.n_tiles(sc.width, sc.height)
        n = chunks if chunks else gs.suggest_chunks(total, samples=sc.samples, max_depth=sc.max_depth)
        t, t8, _ = gs.render_tiles(SEED, 0, 1, total, stats=stats, chunks=n)
        torch.cuda.synchronize()
        st = stats.cpu().tolist()
        rec = {"scene": name, "kernel": gs.last_launch_kernel(), "chunks": n, "stats": st[:4],
               "frame": hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest(),
               "frame8": hashlib.sha256(t8.cpu().numpy().tobytes()).hexdigest()}
        if diag:
            d = st[4:]
            rec.update(trips=d[0], reject_rounds=d[10], reject_lanes=d[11], violations=d[12], parked=d[44], no_room=d[45],
                       swaps_put_off=d[46], dry_drains=d[47], parked_children=d[48])
        print(json.dumps(rec), flush=True)
        gs.launch_status()
        gs.close()


if __name__ == "__main__":
    main()
