#!/usr/bin/env python3
"""What the probes' visibility weight costs ("Probe visibility"): at 1920 x 1080 on config 4's room and on config 5's
mesh, grids of 8^3, 16^3 and 32^3 probes with maps of 8 x 8 texels, in one run:
  k_probe_shade_vis next to k_probe_shade, both with the facing weight, on the frame's first hits and with baked coefficients and
  moments; the depth bake (rt_hip_bake_probe_grid_depth) next to the radiance bake of the same rays (rt_hip_bake_probe_grid); the
  whole _vis preview next to the plain one.
The method is tools/probe_shade_bench.py's: a window is LAUNCHES launches enqueued back to back between two device events, every
buffer allocated beforehand, the figure is the window over LAUNCHES, the median of --repeats windows after one warm window (the bakes
and the previews: windows of fewer launches, as that tool takes its own).  This process starts no GPU work of its own: the
measurement runs in a child process under a time limit.  Also the registers and scratch bytes the compiler reports for the new kernels.
usage: python tools/probe_vis_bench.py [--repeats 9] [--out profiles/r26_probe_vis.txt]"""
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

from probe_shade_bench import ENTRY_BYTES, H, LAUNCHES, SEED, W, grid_over, timed  # noqa: E402

RES, BAKE_SAMPLES = 8, 16
CHILD_SECONDS = 420


def kernel_resources():
    """-> lines: VGPRs, SGPRs, scratch and LDS bytes of probe.hip's visibility kernels, from the compiler's metadata"""
    csrc = os.path.join(ROOT, "raytracer.c_amd", "csrc")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "probe.s")
        subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
                        "--cuda-device-only", "-S", "-o", asm, os.path.join(csrc, "probe.hip")], check=True, capture_output=True)
        text = open(asm).read()
    out = []
    for block in text.split("- .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+\S*?(k_probe_(?:shade_vis|depth_fold|depth_resolve|shade))E", block)
        keys = {k: re.search(r"\.%s:\s+(\d+)" % k, block) for k in ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")}
        if name and all(keys.values()):
            out.append(f"{name.group(1)}: {keys['vgpr_count'].group(1)} VGPRs, {keys['sgpr_count'].group(1)} SGPRs, scratch "
                       f"{keys['private_segment_fixed_size'].group(1)} B, LDS {keys['group_segment_fixed_size'].group(1)} B")
    return out


def measure(repeats):
    """(the child's work) -> dict: per config and grid the two shades, the two bakes and the two previews, ms"""
    import numpy as np
    import torch
    from rt_amd import abi, gpu, scene as Sc
    out = {}
    for config in (4, 5):
        sc = Sc.build_scene(config, W, H, 1)
        gs = gpu.GpuScene(sc)
        shim = gs.shim
        x, y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
        uv = torch.as_tensor(np.stack([(x + 0.5) / (W - 1.0), (y + 0.5) / (H - 1.0)], axis=2).reshape(-1, 2), device="cuda")
        hits = gs.query_uv(uv, want=("status", "point", "normal", "object"))
        total = gpu.n_tiles(W, H)
        albedo = gs.untile_aov(gs.render_aov(SEED, 1, 0, 1, total, want=("albedo",)), 0, 1, total)["albedo"].reshape(-1, 3)
        add = torch.zeros((W * H, 3), dtype=torch.float32, device="cuda")
        color = torch.empty((W * H, 3), dtype=torch.float32, device="cuda")
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        ptr = lambda t: C.c_void_p(t.data_ptr())
        rec = dict(hit_fraction=float((hits["status"] == 1).double().mean()), grids={})
        for n in (8, 16, 32):
            grid = grid_over(gs, n, True)
            vis = abi.probe_vis(grid, res=RES)
            coeff, mom = gs.bake_probe_grid(grid, BAKE_SAMPLES, SEED, vis=vis)
            tail = (ptr(hits["point"]), ptr(hits["normal"]), ptr(hits["status"]), ptr(albedo), ptr(add), W * H, None, ptr(color), stream)

            def plain():
                assert shim.rt_hip_probe_shade(C.byref(grid), ptr(coeff), *tail) == 0

            def weighed():
                assert shim.rt_hip_probe_shade_vis(C.byref(grid), C.byref(vis), ptr(coeff), ptr(mom), *tail) == 0
            g = dict(shade_ms=timed(plain, repeats), shade_vis_ms=timed(weighed, repeats))
            g["shade_again_ms"] = timed(plain, repeats)   # the plain shade once more, after: the run's own drift
            g["bake_ms"] = timed(lambda: gs.bake_probe_grid(grid, BAKE_SAMPLES, SEED), 3, 3)
            g["depth_bake_ms"] = timed(lambda: gs.probe_depth_moments(grid, vis, BAKE_SAMPLES, SEED), 3, 3)
            g["preview_ms"] = timed(lambda: gs.probe_preview(grid, coeff, aov_samples=1, seed=SEED), repeats, 5)
            g["preview_vis_ms"] = timed(lambda: gs.probe_preview(grid, coeff, aov_samples=1, seed=SEED, vis=vis, moments=mom), repeats, 5)
            g["d_max"], g["bias"] = vis.d_max, vis.bias
            rec["grids"][f"{n}^3"] = g
        assert gs.launch_status() == 0
        out[f"config {config}"] = rec
        gs.close()
        sc.free()
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
    lines = [f"{W} x {H}, maps of {RES} x {RES} texels, grids baked with {BAKE_SAMPLES} rays a probe, the facing weight on both sides; a figure is a "
             f"window of {LAUNCHES} launches between two device events over {LAUNCHES} (5 for a preview, 3 for a bake), the median of "
             f"{args.repeats} windows (3 for a bake) after a warm one; one process; entry traffic {ENTRY_BYTES} B an entry, moments up to "
             f"{8 * 4 * 16} B an entry on top"]
    for name, rec in got.items():
        lines.append(f"{name} ({100 * rec['hit_fraction']:.1f} % of the pixels hit):")
        for key, g in rec["grids"].items():
            lines.append(f"  {key:5s} k_probe_shade {g['shade_ms']:.3f} ms (again after: {g['shade_again_ms']:.3f}); k_probe_shade_vis "
                         f"{g['shade_vis_ms']:.3f} ms, {g['shade_vis_ms'] / g['shade_ms']:.2f} x; radiance bake {g['bake_ms']:.3f} ms, depth bake "
                         f"{g['depth_bake_ms']:.3f} ms, {g['depth_bake_ms'] / g['bake_ms']:.2f} x; preview {g['preview_ms']:.3f} ms, _vis preview "
                         f"{g['preview_vis_ms']:.3f} ms, {g['preview_vis_ms'] / g['preview_ms']:.2f} x (d_max {g['d_max']:.3f}, bias {g['bias']:.4f})")
    lines += kernel_resources()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
