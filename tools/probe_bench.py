#!/usr/bin/env python3
"""What a light-probe bake costs next to tracing the same rays ("Light probes"): 4,096 sphere probes at 256 samples in
config 4's room and in config 5's mesh.  Times by device events, the best of --repeats after one warm run: the whole bake
(rt_hip_bake_probes in one slice), the generator alone (rt_hip_probe_rays), the resolve alone (rt_hip_probe_resolve), and the same
N x S rays through rt_hip_trace_rays alone in one call -- the figure that exists without the probes, the baseline.  The fold has no
entry point of its own: its time is the bake's less the other three.  Also the scratch and LDS bytes the compiler reports for the
four kernels of csrc/probe.hip (one device-only compile to assembly; its .amdhsa metadata).
usage: python tools/probe_bench.py [--repeats 5] [--out profiles/r24_probe.txt]"""
import argparse
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "raytracer.c_amd"))

N, S, SEED = 4096, 256, 7


def timed(fn, repeats):
    import torch
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b))
    return best


def kernel_resources():
    """-> lines: scratch and LDS bytes of probe.hip's kernels, from the compiler's metadata"""
    csrc = os.path.join(ROOT, "raytracer.c_amd", "csrc")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "probe.s")
        subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
                        "--cuda-device-only", "-S", "-o", asm, os.path.join(csrc, "probe.hip")], check=True, capture_output=True)
        text = open(asm).read()
    out = []
    for block in text.split("- .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+\S*?(k_probe_[a-z]+)", block)
        scratch = re.search(r"\.private_segment_fixed_size:\s+(\d+)", block)
        lds = re.search(r"\.group_segment_fixed_size:\s+(\d+)", block)
        if name and scratch and lds:
            out.append(f"{name.group(1)}: scratch {scratch.group(1)} B, LDS {lds.group(1)} B")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from rt_amd import abi, gpu, scene as Sc
    shim = abi.load_shim()
    lines = []
    for config in (4, 5):
        sc = Sc.build_scene(config, 64, 64, 1)
        gs = gpu.GpuScene(sc)
        info = Sc.scene_info(config)
        # a 16 x 16 x 16 lattice one unit wide about the point the camera looks at
        g = (np.arange(16) - 7.5) / 16.0
        pos = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3) + np.array(list(info.cam_target))
        radius = float(np.linalg.norm(pos, axis=1).max())
        d_pos = torch.as_tensor(pos, device="cuda")
        rays = torch.empty((N * S, 6), dtype=torch.float64, device="cuda")
        p = abi.probe_params(abi.PROBE_SPHERE, S, SEED, sc.max_depth, 0.0, radius)
        stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)

        def generator():
            rc = shim.rt_hip_probe_rays(C.c_void_p(d_pos.data_ptr()), None, N, C.byref(p), 0, N * S, C.c_void_p(rays.data_ptr()), stream())
            assert rc == 0, shim.rt_hip_last_error()
        t_gen = timed(generator, args.repeats)
        t_trace = timed(lambda: gs.trace_rays(rays, 1, SEED, origin_radius=radius), args.repeats)
        out = {}

        def bake():
            out.update(gs.bake_probes(d_pos, S, SEED, origin_radius=radius, details=True))
        t_bake = timed(bake, args.repeats)
        t_resolve = timed(lambda: gpu.probe_resolve(out["sum"], S), args.repeats)
        assert gs.launch_status() == 0
        t_fold = t_bake - t_gen - t_trace - t_resolve
        lines.append(f"config {config}, {N} probes x {S} samples ({gs.trace_kernel_name()}): bake {t_bake:.3f} ms; rt_hip_trace_rays alone, one call "
                     f"{t_trace:.3f} ms; generator {t_gen:.3f} ms; resolve {t_resolve:.3f} ms; fold (the bake less the three) {t_fold:.3f} ms; "
                     f"overhead over tracing alone {100.0 * (t_bake / t_trace - 1.0):.1f} %")
        gs.close()
        sc.free()
    lines += kernel_resources()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
