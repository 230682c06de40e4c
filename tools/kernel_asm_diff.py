#!/usr/bin/env python3
"""Are the kernels of two sets of compiler assembly listings the same machine code?

    kernel_asm_diff.py A.s [B.s ...] -- C.s [D.s ...]

Each side is the union of its files (hipcc $(HIPFLAGS) --cuda-device-only -S).  A kernel is the text
from its `_Z...:` label to its `.Lfunc_end`, plus its `.amdhsa_kernel ... .end_amdhsa_kernel` block
(registers, LDS, scratch), with `;` comments and trailing blanks stripped and the per-file function
index of local labels (.LBB<n>_, .LJTI<n>_, .Lfunc_end<n>, .Ltmp<n>) replaced by a placeholder, so
that the order of the functions and the file they are in do not matter.  Reports the kernels found
on one side only, those whose text differs and the number that is identical; exit status 0 only when
both sides hold the same kernels and all are identical.
"""
import re
import sys

LABEL = re.compile(r"^(_Z\w+):")
LOCAL = re.compile(r"\.?(LBB|BB|LJTI|Lfunc_end|Ltmp)\d+")
DESCRIPTOR = re.compile(r"^\s*\.amdhsa_kernel\s+(\S+)")


def kernels(paths):
    """{mangled name: normalised text} of every kernel in the files."""
    body, desc = {}, {}
    for path in paths:
        name = block = None  # the function / the descriptor block being collected
        for raw in open(path):
            line = LOCAL.sub(lambda m: m.group(1) + "#", raw.split(";", 1)[0].rstrip())
            if LABEL.match(raw):
                name = LABEL.match(raw).group(1)
                if name in body:
                    sys.exit(f"{path}: {name} defined twice on one side")
                body[name] = []
            if DESCRIPTOR.match(raw):
                block = desc.setdefault(DESCRIPTOR.match(raw).group(1), [])
            if block is not None:
                block.append(line)
                if ".end_amdhsa_kernel" in raw:
                    block = None
            elif name is not None and line:
                body[name].append(line)
            if raw.startswith(".Lfunc_end"):
                name = None
    return {k: "\n".join(body[k] + desc[k]) for k in body if k in desc}  # a kernel has a descriptor


def main(argv):
    if "--" not in argv or argv[0] == "--" or argv[-1] == "--":
        sys.exit(__doc__)
    cut = argv.index("--")
    a, b = kernels(argv[:cut]), kernels(argv[cut + 1:])
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    differ = sorted(k for k in set(a) & set(b) if a[k] != b[k])
    for what, names in (("only on the left: ", only_a), ("only on the right:", only_b), ("differs:          ", differ)):
        for k in names:
            print(what, k)
    same = len(set(a) & set(b)) - len(differ)
    print(f"{len(a)} kernels left, {len(b)} right: {same} identical, {len(differ)} differ, "
          f"{len(only_a)} only left, {len(only_b)} only right")
    return 0 if not (only_a or only_b or differ) and a else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
