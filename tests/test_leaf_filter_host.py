"""The leaf round's candidate filter on the host (csrc/rt_leaf_filter.h): never drops a sphere the
reference would hit, and does drop the family it exists for.  CPU; tests/cpp/test_leaf_filter.cpp."""
import subprocess

import probe_support as ps


def test_leaf_filter_sound_and_useful(tmp_path):
    exe = ps.build_leaf_filter_host(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout
    assert out.stdout.strip().endswith("OK")


def test_leaf_filter_dump_holds_both_answers(tmp_path):
    exe = ps.build_leaf_filter_host(tmp_path)
    cases, behind = ps.leaf_filter_cases(exe, tmp_path, 1 << 12)
    assert cases.shape == (4, 1 << 12) and set(behind.tolist()) == {0, 1}
    assert 0.1 < behind.mean() < 0.9
