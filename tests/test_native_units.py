"""Host-only C++ units checked without a GPU and without loading anything into Python:
each is a stand-alone program (tests/native/*.cpp, its own main) compiled with g++ against
the sources under csrc/ and run as a child process.

plan_check: the render planner (csrc/render_plan.cpp alone) -- chunking, regions, the
            working-set layout, sphere sources, stream shape, the fused tail, the algorithm.
pool_check: HostCopyPool (csrc/host_copy_pool.hpp alone) under ThreadSanitizer and under
            AddressSanitizer + UBSan.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rust-raytrace_amd", "csrc")
NATIVE = os.path.join(ROOT, "tests", "native")
CXXFLAGS = ["-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-I" + CSRC,
            "-I" + os.path.join(ROOT, "include")]


def _build_and_run(tmp_path, name, sources, extra, env=None):
    exe = str(tmp_path / name)
    cmd = [os.environ.get("CXX", "g++")] + CXXFLAGS + extra + ["-o", exe] + sources + ["-pthread"]
    cc = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert cc.returncode == 0, cc.stdout
    run_env = dict(os.environ)
    run_env.update(env or {})
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=run_env, timeout=300)
    assert run.returncode == 0, run.stdout
    return run.stdout


def test_render_planner(tmp_path):
    out = _build_and_run(tmp_path, "plan_check",
                         [os.path.join(NATIVE, "plan_check.cpp"), os.path.join(CSRC, "render_plan.cpp")], ["-O1", "-g"])
    assert "plan_check ok" in out


@pytest.mark.parametrize("san,env", [
    ("thread", {"TSAN_OPTIONS": "halt_on_error=1"}),
    ("address,undefined", {"ASAN_OPTIONS": "detect_leaks=1:halt_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1"}),
], ids=["tsan", "asan-ubsan"])
def test_host_copy_pool_sanitized(tmp_path, san, env):
    out = _build_and_run(tmp_path, "pool_check", [os.path.join(NATIVE, "pool_check.cpp")],
                         ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=" + san, "-fno-sanitize-recover=all"], env)
    assert "pool_check ok" in out
