"""One way to compile a kernel file of raytracing-with-zig_amd/csrc for inspection, with the flags the
product is built with: they are read from the Makefile (`make print-hipflags`), their only home.
resources("rt_kernel.hip") gives {kernel: {"VGPRs": 127, "ScratchSize [bytes/lane]": 0, ...}},
assembly("rt_kernel.hip", ("-DRTZIG_MARKS=1",)) the device assembly's lines; each (source, extra) is
compiled once per process.  The tests import this module by path."""
import functools
import os
import re
import subprocess
import tempfile

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "raytracing-with-zig_amd", "csrc")


@functools.lru_cache(maxsize=None)
def _hipcc():
    flags = subprocess.run(["make", "-s", "-C", CSRC, "print-hipflags"], capture_output=True, text=True, check=True).stdout
    return [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), *flags.split(), "--cuda-device-only"]  # HIPCC: as the Makefile


@functools.lru_cache(maxsize=None)
def resources(source, extra=()):
    """The compiler's resource remarks of every kernel in `source`: {mangled name: {remark: int}}."""
    err = subprocess.run(_hipcc() + ["-c", "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage", *extra, source],
                         cwd=CSRC, check=True, capture_output=True, text=True).stderr
    out, cur = {}, None
    for line in err.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z /\[\]]+?): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return out


@functools.lru_cache(maxsize=None)
def assembly(source, extra=()):
    """The device assembly of `source` (hipcc -S), as a tuple of lines."""
    with tempfile.TemporaryDirectory(prefix="rtzig_asm_") as d:
        out = os.path.join(d, "k.s")
        subprocess.run(_hipcc() + ["-S", "-o", out, *extra, source], cwd=CSRC, check=True, capture_output=True, text=True)
        return tuple(open(out).read().split("\n"))
