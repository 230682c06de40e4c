"""Host check of the scene code (csrc/rt_scene.cpp), CPU only: compiles tests/cpp/test_scene.cpp against
rt_scene.cpp and rt_bvh.cpp.  No GPU and no HIP runtime call."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raytracing-with-zig_amd", "csrc")


def test_scene_records_tree_and_training(tmp_path):
    exe = tmp_path / "test_scene"
    subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-ffp-contract=off", "-pthread", "-x", "hip",
                    "--offload-arch=gfx950", "--offload-host-only",
                    os.path.join(ROOT, "tests", "cpp", "test_scene.cpp"), os.path.join(CSRC, "rt_scene.cpp"),
                    os.path.join(CSRC, "rt_bvh.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, timeout=300)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0, out.stdout
    assert out.stdout.strip().endswith("OK")
