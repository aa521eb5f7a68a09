"""The planner's cases for RT_ALGO_WAVEFRONT_AA, checked without a GPU: tests/native/aa_plan_check.cpp
(its own main) compiled with g++ against csrc/render_plan.cpp alone and run as a child process, as
test_native_units.py runs plan_check.

aa_plan_check: mode 6 accepted / refused, RT_ALGO_AUTO with tuning aa_wavefront 0 and 1, the other
               algorithms' refusals unchanged, the tuning key's place and range, the working-set
               layout and budget with the running sums.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rust-raytrace_amd", "csrc")
NATIVE = os.path.join(ROOT, "tests", "native")
CXXFLAGS = ["-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-O1", "-g", "-I" + CSRC,
            "-I" + os.path.join(ROOT, "include")]


def test_aa_render_planner(tmp_path):
    exe = str(tmp_path / "aa_plan_check")
    cmd = [os.environ.get("CXX", "g++")] + CXXFLAGS + ["-o", exe, os.path.join(NATIVE, "aa_plan_check.cpp"),
                                                      os.path.join(CSRC, "render_plan.cpp")]
    cc = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert cc.returncode == 0, cc.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert run.returncode == 0, run.stdout
    assert "aa_plan_check ok" in run.stdout
