"""The domain rule of rt_trace_rays (csrc/rt_trace.h trace_tree_ok) on the CPU: the header compiles
with plain g++, and the predicate is false on every ray the contract bars from the tree and true on
every ray it keeps there (tests/cpp/test_trace_domain.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_trace_domain(tmp_path):
    exe = tmp_path / "test_trace_domain"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror",
                    os.path.join(ROOT, "tests", "cpp", "test_trace_domain.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout
    assert out.stdout.strip().endswith("OK")
