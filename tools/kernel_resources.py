#!/usr/bin/env python3
"""Register and LDS budget of every kernel in rt_kernel.hip as the compiler
allocated it (hipcc -Rpass-analysis=kernel-resource-usage with the flags of csrc/Makefile,
tools/kernel_build.py), printed as a table and, given a tag, written to
profiles/<tag>/kernel_resources.json.  rocprofv3's VGPR_Count column is not this count (it reports
64 for the 127-VGPR parity kernel), so the summaries quote the compiler's figures from here.

    python tools/kernel_resources.py [<tag>] [-D...]
"""
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_build  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def resources(extra=()):
    return kernel_build.resources("rt_kernel.hip", tuple(extra))


if __name__ == "__main__":
    tag = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("-") else None
    extra = sys.argv[2:] if tag else sys.argv[1:]
    res = resources(extra)
    if tag:
        d = os.path.join(ROOT, "profiles", tag)
        os.makedirs(d, exist_ok=True)
        json.dump({"source": "hipcc -Rpass-analysis=kernel-resource-usage " + " ".join(extra), "kernels": res},
                  open(os.path.join(d, "kernel_resources.json"), "w"), indent=1)
    for k, v in res.items():
        name = re.sub(r"^_ZN3rtk\d+", "", k)[:34]
        print(f"{name:34s} vgpr={v.get('VGPRs')} sgpr={v.get('TotalSGPRs')} scratch={v.get('ScratchSize [bytes/lane]')} "
              f"spill={v.get('VGPRs Spill')} waves={v.get('Occupancy [waves/SIMD]')}")
