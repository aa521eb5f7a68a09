"""The planner's cases for skybox chain scenes, checked without a GPU: tests/native/sky_plan_check.cpp
(its own main) compiled with g++ against csrc/render_plan.cpp alone and run as a child process, as
test_native_aa.py runs aa_plan_check.  And the scene generator the GPU tests use.

sky_plan_check: with needs_path false, every algorithm x jitter x spp x aa_wavefront is planned for a
                skybox scene as for the same scene with a solid background (mode, sources, streams);
                with a path-only class the chain algorithms still refuse.
"""
import os
import subprocess

import libraytrace as lr
from libraytrace import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rust-raytrace_amd", "csrc")
NATIVE = os.path.join(ROOT, "tests", "native")
CXXFLAGS = ["-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-O1", "-g", "-I" + CSRC,
            "-I" + os.path.join(ROOT, "include")]


def test_sky_render_planner(tmp_path):
    exe = str(tmp_path / "sky_plan_check")
    cmd = [os.environ.get("CXX", "g++")] + CXXFLAGS + ["-o", exe, os.path.join(NATIVE, "sky_plan_check.cpp"),
                                                      os.path.join(CSRC, "render_plan.cpp")]
    cc = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert cc.returncode == 0, cc.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert run.returncode == 0, run.stdout
    assert "sky_plan_check ok" in run.stdout


def test_skybox_chain_scene_has_chain_classes_only(tmp_path):
    """skybox_scene without its Transparent sphere, plus a Fresnel sphere, a plane and a directional
    light; it parses, and the oracle renders it with sky in the mirrors."""
    from oracle import ref64
    paths = [str(tmp_path / f"f{k}.ppm") for k in range(6)]
    for p, f in zip(paths, scenes.skybox_faces(size=8, seed=2)):
        scenes.write_ppm(p, f)
    spec, old = scenes.skybox_chain_scene(paths, 48, 32), scenes.skybox_scene(paths, 48, 32)
    kinds = [o["material"]["kind"] for o in spec.objects]
    assert set(kinds) == {"phong", "fresnel"} and kinds.count("fresnel") == 2
    assert [o["shape"] for o in spec.objects].count("plane") == 1
    assert sorted(l["kind"] for l in spec.lights) == ["directional", "point"]
    assert spec.objects[:2] == old.objects[:2] and spec.camera == old.camera and not spec.camera.get("dof")
    assert [o["material"]["kind"] for o in old.objects].count("transparent") == 1      # the old generator is unchanged
    lr.Scene.deserialize(spec.to_text()).close()
    deep, flat = ref64.render(spec), ref64.render(spec, max_depth=0)
    assert (deep["rgb64"] != flat["rgb64"]).any() and (deep["rgb64"] > 0).any()
