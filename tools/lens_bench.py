#!/usr/bin/env python3
"""What a lens frame costs next to the pinhole frame of the same size and samples ("Thin-lens camera"): config 4's room
at 1920 x 1080 x 64 spp and config 5's mesh at 480 x 270 x 16 spp.  Times by device events around whole frames, the best of --repeats
after one warm frame: the lens frame (GpuScene.render_lens: generator, rt_hip_trace_rays, sum, resolve) and the pinhole frame
(GpuScene.render_image: render_tiles, untouched by the lens).  The split of the lens frame over its kernels is a profiler's job
(rocprofv3 --kernel-trace --stats -- python tools/lens_bench.py --repeats 1, in a run of its own); this tool prints frames only.
usage: python tools/lens_bench.py [--repeats 5] [--out profiles/r23_lens.txt]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "raytracer.c_amd"))


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from rt_amd import gpu, scene as S
    lines = []
    for config, w, h, spp, focus in ((4, 1920, 1080, 64, 50.0), (5, 480, 270, 16, 10.0)):
        sc = S.build_scene(config, w, h, spp)
        gs = gpu.GpuScene(sc)
        pinhole = timed(lambda: gs.render_image(7), args.repeats)
        lens = timed(lambda: gs.render_lens(0.25, focus, spp, 7), args.repeats)
        sliced = timed(lambda: gs.render_lens(0.25, focus, spp, 7, slice_pixels=1 << 18), args.repeats)
        lines.append(f"config {config} {w}x{h}x{spp}: pinhole frame ({gs.last_launch_kernel()}) {pinhole:.3f} ms, lens frame ({gs.trace_kernel_name()}) "
                     f"{lens:.3f} ms, ratio {lens / pinhole:.2f}; lens frame in slices of 2^18 pixels {sliced:.3f} ms")
        gs.close()
        sc.free()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
