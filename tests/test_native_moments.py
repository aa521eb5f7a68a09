"""Moments accumulators without a GPU: the planner's rules and the format version 2 checkpoint file, each a
stand-alone C++ program (its own main) compiled with g++ and run as a child process, as
test_native_progressive.py runs its programs.

moments_plan_check: csrc/render_plan.cpp alone under AddressSanitizer + UBSan -- which calls each kind of
                    accumulator refuses, the noise calls' argument checks, the buffer's size and its
                    overflow.
checkpoint2_check:  csrc/host_checkpoint.cpp alone under AddressSanitizer + UBSan -- a round trip of sums and
                    squares, each reader against the other version's file, then the version 2 reader against an
                    empty file, a file cut at every header field boundary, in the sums, where the squares begin
                    and in the squares, a wrong magic and version, pixel counts off by one, 2^59 and 2^61.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rust-raytrace_amd", "csrc")
NATIVE = os.path.join(ROOT, "tests", "native")
CXXFLAGS = ["-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-O1", "-g", "-I" + CSRC,
            "-I" + os.path.join(ROOT, "include")]
SANITIZE = ["-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
SAN_ENV = {"ASAN_OPTIONS": "detect_leaks=1:halt_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1"}


def _build_and_run(tmp_path, name, sources, extra=(), args=(), env=None):
    exe = str(tmp_path / name)
    cmd = [os.environ.get("CXX", "g++")] + CXXFLAGS + list(extra) + ["-o", exe] + sources
    cc = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert cc.returncode == 0, cc.stdout
    run_env = dict(os.environ)
    run_env.update(env or {})
    run = subprocess.run([exe] + list(args), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300,
                         env=run_env)
    assert run.returncode == 0, run.stdout
    return run.stdout


def test_moments_planner_sanitized(tmp_path):
    out = _build_and_run(tmp_path, "moments_plan_check",
                         [os.path.join(NATIVE, "moments_plan_check.cpp"), os.path.join(CSRC, "render_plan.cpp")],
                         extra=SANITIZE, env=SAN_ENV)
    assert "moments_plan_check ok" in out


def test_checkpoint_version_2_sanitized(tmp_path):
    scratch = tmp_path / "files"
    scratch.mkdir()
    out = _build_and_run(tmp_path, "checkpoint2_check",
                         [os.path.join(NATIVE, "checkpoint2_check.cpp"), os.path.join(CSRC, "host_checkpoint.cpp")],
                         extra=SANITIZE, args=[str(scratch)], env=SAN_ENV)
    assert "checkpoint2_check ok" in out
