"""Host check of the tree-in-LDS rule shared by the BVH launchers and the training (csrc/rt_kernel.h
bvh_lds_plan), CPU only: the shipped build and the RTZIG_STACK16=1 knob's."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("stack16", [0, 1])
def test_lds_plan_table(tmp_path, stack16):
    exe = tmp_path / "test_lds_plan"
    subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-x", "hip", "--offload-arch=gfx950",
                    "--offload-host-only", f"-DRTZIG_STACK16={stack16}",
                    os.path.join(ROOT, "tests", "cpp", "test_lds_plan.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, timeout=300)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout
    assert out.stdout.strip().endswith("OK")
