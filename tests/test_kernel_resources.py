"""The shipped kernels' register budget, checked at build time (CPU; hipcc cross-compiles gfx950):
no sample kernel uses scratch memory (a stray by-reference flag or dynamically indexed local array
puts per-lane state in scratch: slower, and a spilling kernel faulted on the MI355X in round 4,
profiles/r04_occupancy), and the uninstrumented BVH kernels keep 4 waves per SIMD (<= 128 VGPRs,
DESIGN §5.1)."""
import re

from abi_support import resources


def test_no_scratch_and_bvh_kernels_at_four_waves():
    rows = resources("rt_kernel.hip")
    samples = {k: v for k, v in rows.items() if "sample_kernel" in k}
    assert len(samples) == 24, sorted(samples)
    assert all(v["ScratchSize [bytes/lane]"] == 0 for v in samples.values()), \
        {k: v["ScratchSize [bytes/lane]"] for k, v in samples.items() if v["ScratchSize [bytes/lane]"]}
    # sample_kernel_bvh<kLdsScene, kProf = false, kDirect> and the fast twin: 4 waves per SIMD
    plain = {k: v for k, v in rows.items() if re.search(r"sample_kernel_(bvh|fast)ILb[01]ELb0E", k)}
    assert len(plain) == 8
    assert all(v["Occupancy [waves/SIMD]"] == 4 and v["VGPRs"] <= 128 for v in plain.values()), plain
