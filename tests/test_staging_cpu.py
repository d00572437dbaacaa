"""The layout of a host form's one device allocation (raytracer.c_amd/csrc/rt_staging.h) is host arithmetic with no HIP call in
it: tests/staging_check.cpp runs it over the part lists of the seven host-array entry points, stand-alone, under the address and
undefined-behaviour sanitizers of the host compiler."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_host_form_s_parts_are_aligned_disjoint_and_inside_the_total(tmp_path):
    exe = str(tmp_path / "staging_check")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "raytracer.c_amd", "csrc"), "-o", exe,
                            os.path.join(ROOT, "tests", "staging_check.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert int(run.stdout.split()[0]) > 4000 and run.stdout.split()[1:] == ["plans", "checked"]
