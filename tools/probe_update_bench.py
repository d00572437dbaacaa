#!/usr/bin/env python3
"""What an update round of a probe grid costs ("Probe updates"): 16^3 probes x 16 rays, maps of 8 x 8 texels, in config
4's room and in config 5's mesh, in one run:
  one round (rt_hip_probe_grid_update, stride 1, warm state) next to the full bake of the same grid (rt_hip_bake_probe_grid +
  rt_hip_bake_probe_grid_depth) at 16 and at 256 rays a probe, every workspace allocated beforehand;
  the round's pieces on the same 65,536 rays: the generator (rt_hip_probe_rays), the radiance query (GpuScene.trace_rays, one sample a
  ray), the ray query (GpuScene.query_rays), the three blend kernels (rt_hip_probe_blend_coeff, _blend_moments, _age_step); the two
  folds have no call of their own, so what the round takes beyond those pieces (two generators, both queries, the blends) is
  printed as "folds and the rest", a difference and not a measurement;
  and the moved-light experiment of tests/test_gpu_probe_update.py on config 2's scene: the three L0 distances and the rounds to halve.
The method is tools/probe_shade_bench.py's: a window is launches enqueued back to back between two device events, the figure is the
window over its launches, the median of --repeats windows after one warm window.  This process starts no GPU work of its own: the
measurement runs in a child process under a time limit.  Also the registers, scratch and LDS bytes of the four new kernels.
usage: python tools/probe_update_bench.py [--repeats 9] [--out profiles/r27_probe_update.txt]"""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "raytracer.c_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from probe_shade_bench import SEED, grid_over, timed  # noqa: E402

N, RAYS, RES, FULL = 16, 16, 8, (16, 256)
W, H = 64, 64   # (the frame's size plays no part in a round)
WINDOW = 5
CHILD_SECONDS = 540


def kernel_resources():
    """-> lines: VGPRs, SGPRs, scratch and LDS bytes of probe.hip's update kernels, from the compiler's metadata"""
    csrc = os.path.join(ROOT, "raytracer.c_amd", "csrc")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "probe.s")
        subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
                        "--cuda-device-only", "-S", "-o", asm, os.path.join(csrc, "probe.hip")], check=True, capture_output=True)
        text = open(asm).read()
    out = []
    for block in text.split("- .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+\S*?(k_probe_(?:grid_positions_strided|coeff_blend|moment_blend|age_step))E", block)
        keys = {k: re.search(r"\.%s:\s+(\d+)" % k, block) for k in ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")}
        if name and all(keys.values()):
            out.append(f"{name.group(1)}: {keys['vgpr_count'].group(1)} VGPRs, {keys['sgpr_count'].group(1)} SGPRs, scratch "
                       f"{keys['private_segment_fixed_size'].group(1)} B, LDS {keys['group_segment_fixed_size'].group(1)} B")
    return out


def moved_light():
    """the experiment of tests/test_gpu_probe_update.py::test_the_state_follows_a_moved_light, with its parameters -> dict"""
    import numpy as np
    import torch
    from rt_amd import abi, gpu, scene as Sc
    sc = Sc.build_scene(2, 33, 17, 1, 4)
    gs = gpu.GpuScene(sc)
    grid = abi.probe_grid((-15.0, 0.0, -12.0), (15.0, 8.0, 16.0), (3, 3, 2))
    seed, s = 20261020, 8
    host = lambda t: (torch.cuda.synchronize(), t.cpu().numpy())[1]
    dist = lambda a, b: float(np.sqrt(((a[:, 0, :] - b[:, 0, :]) ** 2).sum()))
    lights = [i for i in range(sc.n_objects) if max(sc.objects[i].emission.tuple()) > 0]
    a = host(gs.spheres()).copy()
    b = a.copy()
    b[lights[0], :3] = (-a[lights[0], 0], a[lights[0], 1] + 10.0, -a[lights[0], 2])

    def run(change, fast):
        gs.update_spheres(a)
        state = gs.probe_grid_state(grid, s, seed, hysteresis=0.9, change=change, fast=fast)
        state.coeff.copy_(gs.bake_probe_grid(grid, 4096, seed + 1, max_depth=4))
        state.age.fill_(4096 // s)   # warm: the bake stands for that many rounds, so the first round blends at 1 - h
        before = host(state.coeff).copy()
        gs.update_spheres(b)
        trail = []
        for _ in range(40):
            state.update()
            trail.append(host(state.coeff).copy())
        return before, trail

    before, trail = run(0.0, 0.0)
    truth = host(gs.bake_probe_grid(grid, 4096, seed + 2, max_depth=4))
    once = host(gs.bake_probe_grid(grid, s, seed + 3, max_depth=4))
    _, quick = run(0.25, 0.5)
    d0 = dist(before, truth)
    halved = [next((k + 1 for k, c in enumerate(t) if dist(c, truth) <= 0.5 * d0), None) for t in (trail, quick)]
    gs.close()
    return dict(before=d0, after=dist(trail[-1], truth), once=dist(once, truth), halved_plain=halved[0], halved_fast=halved[1])


def measure(repeats):
    """(the child's work) -> dict: per config the round, its pieces and the full bakes, ms"""
    import torch
    from rt_amd import abi, gpu, scene as Sc
    out = {}
    for config in (4, 5):
        sc = Sc.build_scene(config, W, H, 1)
        gs = gpu.GpuScene(sc)
        shim, dev = gs.shim, gs.dev
        grid = grid_over(gs, N, True)
        vis = abi.probe_vis(grid, res=RES)
        n = N ** 3
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        ptr = lambda t: C.c_void_p(t.data_ptr())
        radius = gpu._grid_radius(grid)
        coeff, mom = gs.bake_probe_grid(grid, RAYS, SEED, vis=vis)
        coeff, mom = coeff.clone(), mom.clone()
        age = torch.full((n,), 100, dtype=torch.int32, device=dev)
        change = torch.zeros(n, dtype=torch.float64, device=dev)
        status = torch.ones(n, dtype=torch.int32, device=dev)
        coeff_f = torch.zeros((n, 9, 3), dtype=torch.float32, device=dev)
        upd = abi.probe_update()
        p = abi.probe_params(abi.PROBE_SPHERE, RAYS, SEED, gs.scene.max_depth, 0.0, radius)
        ws = gpu._workspace(shim.rt_hip_probe_update_workspace_bytes(C.byref(grid), C.byref(vis), C.byref(upd), n * RAYS), dev)
        rounds = [0]

        def one_round():
            upd.round = rounds[0] & 0xFFFFFFFF
            rounds[0] += 1
            assert shim.rt_hip_probe_grid_update(gs.handle, C.byref(grid), C.byref(vis), C.byref(p), C.byref(upd), n * RAYS, ptr(ws), ptr(coeff),
                                                 ptr(coeff_f), ptr(mom), ptr(age), ptr(change), ptr(status), None, stream) == 0
        rec = dict(round_ms=timed(one_round, repeats, WINDOW))

        for rays in FULL:
            q = abi.probe_params(abi.PROBE_SPHERE, rays, SEED, gs.scene.max_depth, 0.0, radius)
            ws_b = gpu._workspace(shim.rt_hip_probe_grid_workspace_bytes(C.byref(grid), n * rays), dev)
            ws_d = gpu._workspace(shim.rt_hip_probe_grid_depth_workspace_bytes(C.byref(grid), RES, n * rays), dev)
            c2, m2 = torch.empty_like(coeff), torch.empty_like(mom)

            def full():
                assert shim.rt_hip_bake_probe_grid(gs.handle, C.byref(grid), C.byref(q), n * rays, ptr(ws_b), ptr(c2), None, None, None, stream) == 0
                assert shim.rt_hip_bake_probe_grid_depth(gs.handle, C.byref(grid), C.byref(vis), C.byref(q), n * rays, ptr(ws_d), ptr(m2), None,
                                                         stream) == 0
            rec[f"full_{rays}_ms"] = timed(full, min(repeats, 5), 3)
            del ws_b, ws_d
        rec["round_again_ms"] = timed(one_round, repeats, WINDOW)   # the round once more, after: the run's own drift

        pos = gpu.probe_grid_positions(grid)
        rays_t = torch.empty((n * RAYS, 6), dtype=torch.float64, device=dev)

        def generator():
            assert shim.rt_hip_probe_rays(ptr(pos), None, n, C.byref(p), 0, n * RAYS, ptr(rays_t), stream) == 0
        rec["generator_ms"] = timed(generator, repeats, WINDOW)
        rec["trace_ms"] = timed(lambda: gs.trace_rays(rays_t, 1, SEED, origin_radius=radius, want=("status", "radiance")), repeats, WINDOW)
        rec["query_ms"] = timed(lambda: gs.query_rays(rays_t, origin_radius=radius, want=("status", "t")), repeats, WINDOW)
        total = torch.rand((n, 9, 3), dtype=torch.float64, device=dev)
        sums = torch.rand((n, RES * RES, 3), dtype=torch.float64, device=dev)

        def blends():
            assert shim.rt_hip_probe_blend_coeff(ptr(total), RAYS, C.byref(grid), C.byref(upd), ptr(age), ptr(coeff), ptr(coeff_f), ptr(change),
                                                 stream) == 0
            assert shim.rt_hip_probe_blend_moments(ptr(sums), C.byref(grid), C.byref(vis), C.byref(upd), ptr(age), ptr(mom), stream) == 0
            assert shim.rt_hip_probe_age_step(C.byref(grid), C.byref(upd), ptr(age), stream) == 0
        rec["blends_ms"] = timed(blends, repeats, WINDOW)
        assert gs.launch_status() == 0
        out[f"config {config}"] = rec
        gs.close()
        sc.free()
    out["moved_light"] = moved_light()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help="measure in this process and print one JSON line (what the tool starts itself)")
    args = ap.parse_args()
    if args.child:
        print(json.dumps(measure(args.repeats)))
        return
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--repeats", str(args.repeats)], capture_output=True, text=True,
                       timeout=CHILD_SECONDS)
    if r.returncode != 0:
        sys.stderr.write(r.stderr)
        raise SystemExit(f"the measuring process failed ({r.returncode}); nothing more is started")
    got = json.loads(r.stdout.strip().splitlines()[-1])
    lines = [f"{N}^3 probes, {RAYS} rays a probe a round, maps of {RES} x {RES} texels, stride 1, warm ages; a figure is a window of {WINDOW} calls "
             f"(3 for a full bake) between two device events over its calls, the median of {args.repeats} windows (5 for a full bake) after a "
             f"warm one; one process; workspaces allocated beforehand (the two queries go through the Python wrappers, which allocate "
             f"their outputs from torch's pool)"]
    for name, rec in got.items():
        if name == "moved_light":
            continue
        pieces = 2 * rec["generator_ms"] + rec["trace_ms"] + rec["query_ms"] + rec["blends_ms"]
        lines.append(f"{name}: one round {rec['round_ms']:.3f} ms (again after: {rec['round_again_ms']:.3f}); full bake + depth at "
                     + ", ".join(f"{k} rays {rec[f'full_{k}_ms']:.3f} ms ({rec[f'full_{k}_ms'] / rec['round_ms']:.2f} x the round)" for k in FULL))
        lines.append(f"  pieces on the same rays: generator {rec['generator_ms']:.3f} ms (runs twice a round), radiance query {rec['trace_ms']:.3f} ms, "
                     f"ray query {rec['query_ms']:.3f} ms, blends and age step {rec['blends_ms']:.3f} ms; folds and the rest (a difference) "
                     f"{rec['round_ms'] - pieces:.3f} ms")
    m = got["moved_light"]
    lines.append(f"moved light (config 2, 3 x 3 x 2 probes, 40 rounds of 8 rays, h = 0.9, the state warm at age 512): L0 distance to a 4,096-ray "
                 f"bake at B before the move {m['before']:.6g}, after 40 rounds {m['after']:.6g}, one fresh 8-ray bake {m['once']:.6g}; rounds to "
                 f"halve the distance: plain {m['halved_plain']}, with change = 0.25 and fast = 0.5 {m['halved_fast']}")
    lines += kernel_resources()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
