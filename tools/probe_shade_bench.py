#!/usr/bin/env python3
"""What shading a frame from a probe grid costs ("Probe grids"): k_probe_shade at 1920 x 1080 on config 4's room and on
config 5's mesh, grids of 8^3, 16^3 and 32^3 probes with and without the facing weight, next to the steps of the preview it belongs
to -- the pixel-centre ray query, the first-hit albedo launch --, the denoiser on the same frame, and the whole preview next to
rt_hip_render_tiles' 64-spp frame.
How a time is taken: a window is LAUNCHES launches enqueued back to back between two device events, with every buffer allocated
beforehand -- for the shade the launches are the C call itself, so that the host's part of a launch (about ten microseconds) hides
behind the launches already queued --, and the figure is the window over LAUNCHES; the median of --repeats windows after one warm
window.  The entry traffic is what the kernel moves per entry whatever the grid: point and normal (48 B), status (4 B), albedo and
add (24 B) in, colour (12 B) out.
The wave-uniform path against the gather alone: the shade's measurements with the product and with a build of the shim with
-DPT_SHADE_UNIFORM=0 (make variant NAME=gather DEFS=-DPT_SHADE_UNIFORM=0), on the real frame and on the frame's entries ordered by
cell (waves do not straddle cells but at a cell's last entries).  The two builds are measured in turn, --rounds times each, a process
a turn, and the figure is the median over the rounds.
This process starts no GPU work of its own: every measurement runs in a child process under a time limit.  Also the registers and
scratch bytes the compiler reports for csrc/probe.hip's grid kernels.
usage: python tools/probe_shade_bench.py [--repeats 9] [--rounds 2] [--out profiles/r25_probe_shade.txt]"""
import argparse
import ctypes as C
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "raytracer.c_amd"))

W, H, SEED = 1920, 1080, 7
ENTRY_BYTES = 48 + 4 + 24 + 12
LAUNCHES = 20
CHILD_SECONDS = 240
GATHER = os.path.join(ROOT, "raytracer.c_amd", "csrc", "variants", "librt_hip_gather.so")


def timed(fn, repeats, launches=LAUNCHES):
    """-> ms a launch: the median over `repeats` windows of `launches` calls of fn between two device events, after one warm window"""
    import torch
    for _ in range(launches):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / launches)
    return statistics.median(ms)


def kernel_resources():
    """-> lines: VGPRs, SGPRs, scratch and LDS bytes of probe.hip's grid kernels, from the compiler's metadata"""
    csrc = os.path.join(ROOT, "raytracer.c_amd", "csrc")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "probe.s")
        subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
                        "--cuda-device-only", "-S", "-o", asm, os.path.join(csrc, "probe.hip")], check=True, capture_output=True)
        text = open(asm).read()
    out = []
    for block in text.split("- .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+\S*?(k_probe_(?:shade|grid_positions|pixel_centres|emission|tonemap))", block)
        keys = {k: re.search(r"\.%s:\s+(\d+)" % k, block) for k in ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")}
        if name and all(keys.values()):
            out.append(f"{name.group(1)}: {keys['vgpr_count'].group(1)} VGPRs, {keys['sgpr_count'].group(1)} SGPRs, scratch "
                       f"{keys['private_segment_fixed_size'].group(1)} B, LDS {keys['group_segment_fixed_size'].group(1)} B")
    return out


def grid_over(gs, n, facing):
    """n^3 probes spanning the scene's bounds (rt_hip_scene_bounds): the cube about the triangles' bounding sphere, or without
    triangles the cube of half-side `reach` about the world's origin (wall-sized spheres are not part of the reach)"""
    from rt_amd import abi
    centre, radius, reach, flags = (C.c_double * 3)(), C.c_double(), C.c_double(), C.c_uint32()
    assert gs.shim.rt_hip_scene_bounds(gs.handle, C.byref(centre), C.byref(radius), C.byref(reach), C.byref(flags)) == 0
    r = radius.value if radius.value > 0 else max(reach.value, 1.0)
    origin = [(centre[a] if radius.value > 0 else 0.0) - r for a in range(3)]
    return abi.probe_grid(origin, [2.0 * r / (n - 1)] * 3, [n] * 3, facing=facing)


def measure(repeats, context):
    """(a child's work) -> dict: per config the shade's ms per (grid, facing) on the frame and on the frame ordered by cell; with
    `context` also the preview's other steps, the denoiser, the whole preview, a bake and the 64-spp frame"""
    import numpy as np
    import torch
    from rt_amd import gpu, scene as Sc
    out = {}
    for config in (4, 5):
        sc = Sc.build_scene(config, W, H, 1)
        gs = gpu.GpuScene(sc)
        shim = gs.shim
        x, y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
        uv = torch.as_tensor(np.stack([(x + 0.5) / (W - 1.0), (y + 0.5) / (H - 1.0)], axis=2).reshape(-1, 2), device="cuda")
        hits = gs.query_uv(uv, want=("status", "point", "normal", "object"))
        total = gpu.n_tiles(W, H)
        aov = gs.untile_aov(gs.render_aov(SEED, 1, 0, 1, total), 0, 1, total)
        albedo = aov["albedo"].reshape(-1, 3)
        add = torch.zeros((W * H, 3), dtype=torch.float32, device="cuda")
        color = torch.empty((W * H, 3), dtype=torch.float32, device="cuda")
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        rec = dict(hit_fraction=float((hits["status"] == 1).double().mean()), shade={}, kernel=gs.query_kernel_name())
        for n in (8, 16, 32):
            coeff = torch.randn((n ** 3, 9, 3), dtype=torch.float64, device="cuda")
            for facing in (False, True):
                grid = grid_over(gs, n, facing)

                def launch_of(p, nr, st, al):
                    args = (C.byref(grid), C.c_void_p(coeff.data_ptr()), C.c_void_p(p.data_ptr()), C.c_void_p(nr.data_ptr()), C.c_void_p(st.data_ptr()),
                            C.c_void_p(al.data_ptr()), C.c_void_p(add.data_ptr()), W * H, None, C.c_void_p(color.data_ptr()), stream)

                    def launch():
                        assert shim.rt_hip_probe_shade(*args) == 0
                    return launch
                t_frame = timed(launch_of(hits["point"], hits["normal"], hits["status"], albedo), repeats)
                # the same entries ordered by cell
                g = ((hits["point"] - torch.tensor(list(grid.origin), device="cuda")) / grid.step[0]).clamp(0, n - 1).floor().clamp(max=n - 2).long()
                order = torch.argsort((g[:, 2] * n + g[:, 1]) * n + g[:, 0] + (hits["status"] != 1).long() * n ** 3, stable=True)
                sp, sn, ss, sa = (t[order].contiguous() for t in (hits["point"], hits["normal"], hits["status"], albedo))
                t_sorted = timed(launch_of(sp, sn, ss, sa), repeats)
                rec["shade"][f"{n}^3{' facing' if facing else ''}"] = dict(frame_ms=t_frame, by_cell_ms=t_sorted)
        if context:
            into = {k: hits[k] for k in ("status", "point", "normal", "object")}
            rec["query_ms"] = timed(lambda: gs.query_uv(uv, want=tuple(into), out=into), repeats)
            rec["aov_ms"] = timed(lambda: gs.render_aov(SEED, 1, 0, 1, total, want=("albedo",)), repeats)
            grid = grid_over(gs, 16, True)
            coeff = gs.bake_probe_grid(grid, 16, SEED)
            frame, _ = gs.probe_preview(grid, coeff, aov_samples=1, seed=SEED)
            frame = frame.contiguous()
            clean = torch.empty_like(frame)
            rec["denoise_ms"] = timed(lambda: gpu.denoise(frame, aov, W, H, out=clean), repeats, 5)
            rec["preview_ms"] = timed(lambda: gs.probe_preview(grid, coeff, aov_samples=1, seed=SEED), repeats, 5)
            rec["bake_16^3_x16_ms"] = timed(lambda: gs.bake_probe_grid(grid, 16, SEED), 3, 5)
            rec["render_64spp_ms"] = timed(lambda: gs.render_tiles(SEED, 0, 1, total, samples=64), 3, 2)
            assert gs.launch_status() == 0
        out[f"config {config}"] = rec
        gs.close()
        sc.free()
    return out


def child(repeats, context, shim_path=None):
    """one measurement in a process of its own, under a time limit -> its dict"""
    env = dict(os.environ)
    env.pop("RT_HIP_SHIM_PATH", None)
    if shim_path:
        env["RT_HIP_SHIM_PATH"] = shim_path
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--repeats", str(repeats)] + (["--context"] if context else [])
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=CHILD_SECONDS)
    if r.returncode != 0:
        sys.stderr.write(r.stderr)
        raise SystemExit(f"a measuring process failed ({r.returncode}); nothing more is started")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help="measure in this process and print one JSON line (what the tool starts itself)")
    ap.add_argument("--context", action="store_true", help="with --child: also the preview's other steps, the denoiser and the frames")
    args = ap.parse_args()
    if args.child:
        print(json.dumps(measure(args.repeats, args.context)))
        return
    have_gather = os.path.exists(GATHER)
    uniform, gather = [], []
    for _ in range(args.rounds):   # the two builds in turn
        uniform.append(child(args.repeats, False))
        if have_gather:
            gather.append(child(args.repeats, False, GATHER))
    ctx = child(args.repeats, True)
    over = lambda runs, name, key, f: statistics.median(r[name]["shade"][key][f] for r in runs)
    lines = [f"{W} x {H}; a figure is a window of {LAUNCHES} launches between two device events over {LAUNCHES} (5 for the denoiser, the preview and "
             f"the bake, 2 for the 64-spp frame), the median of {args.repeats} windows after a warm one; the shade's figures are the median over "
             f"{args.rounds} processes a build, the builds in turn; entry traffic {ENTRY_BYTES} B an entry"]
    for name, rec in ctx.items():
        lines.append(f"{name} ({rec['kernel']}, {100 * rec['hit_fraction']:.1f} % of the pixels hit): pixel-centre query {rec['query_ms']:.3f} ms; "
                     f"albedo AOV launch {rec['aov_ms']:.3f} ms; denoiser on the preview's frame (rt_hip_denoise, defaults) {rec['denoise_ms']:.3f} ms; "
                     f"whole preview (16^3 facing) {rec['preview_ms']:.3f} ms; bake of 16^3 probes x 16 samples {rec['bake_16^3_x16_ms']:.3f} ms; "
                     f"rt_hip_render_tiles at 64 spp {rec['render_64spp_ms']:.3f} ms")
        for key in rec["shade"]:
            t = over(uniform, name, key, "frame_ms")
            gbs = ENTRY_BYTES * W * H / (t * 1e-3) / 1e9
            line = (f"  k_probe_shade {key:12s}: frame {t:.3f} ms ({gbs:.0f} GB/s of entry traffic); entries ordered by cell "
                    f"{over(uniform, name, key, 'by_cell_ms'):.3f} ms")
            if gather:
                line += (f"; gather alone (-DPT_SHADE_UNIFORM=0): frame {over(gather, name, key, 'frame_ms'):.3f} ms, ordered by cell "
                         f"{over(gather, name, key, 'by_cell_ms'):.3f} ms")
            lines.append(line)
    if not gather:
        lines.append("(no variants/librt_hip_gather.so: the gather-alone arm was not measured)")
    lines += kernel_resources()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
