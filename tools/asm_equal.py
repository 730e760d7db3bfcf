#!/usr/bin/env python3
"""Are two builds' kernels the same machine code?   tools/asm_equal.py <dir_a> <dir_b>

Reads every *.s of each directory (`make asm` in csrc/ writes them), splits the listings by kernel symbol -- whichever file a
kernel is in, so a kernel may move between translation units -- and compares each kernel's instructions and labels.  Comments
and directives are dropped; the numbers the assembler printer gives a function's labels (.LBB<n>_, .Ltmp<n>, .Lfunc_*<n>,
.LJTI<n>) depend on the kernel's place in its file and are normalised.  Prints `identical` or `differs` per kernel, for a
differing one both instruction counts and its resource lines; exits 1 if a kernel differs or is missing on one side."""
import glob
import os
import re
import sys

RESOURCES = ("next_free_vgpr", "next_free_sgpr", "group_segment_fixed_size", "private_segment_fixed_size")
LABEL_NUMBERS = [(re.compile(r"\.LBB\d+_"), ".LBB_"), (re.compile(r"\.Ltmp\d+"), ".Ltmp"),
                 (re.compile(r"\.Lfunc_([a-z]+)\d+"), r".Lfunc_\1"), (re.compile(r"\.LJTI\d+"), ".LJTI")]


def kernels(directory):
    """{symbol: (code lines, {resource: value})} of every kernel in the directory's listings; a symbol seen twice with two texts is an error"""
    out = {}
    for path in sorted(glob.glob(os.path.join(directory, "*.s"))):
        name, code, res = None, [], {}
        for raw in open(path):
            line = raw.split(";")[0].strip()
            m = re.match(r"\.type\s+(\S+),@function", line)
            if m:
                name, code, res = m.group(1), [], {}
            elif name and line.startswith(".Lfunc_end"):
                if res:  # only kernels have a descriptor; device functions that were not inlined do not
                    if name in out and out[name] != (code, res):  # the same text twice: a header-only library's kernel in two units
                        sys.exit(f"{directory}: kernel {name} is defined twice, differently")
                    out[name] = (code, res)
                name = None
            elif name and line.startswith(".amdhsa_"):
                key, _, value = line[len(".amdhsa_"):].partition(" ")
                if key in RESOURCES:
                    res[key] = value.strip()
            elif name and line and (not line.startswith(".") or line.endswith(":")):
                for pattern, plain in LABEL_NUMBERS:
                    line = pattern.sub(plain, line)
                code.append(line)
    return out


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad = 0
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            print(f"missing in {sys.argv[2] if name in a else sys.argv[1]}: {name}")
        elif a[name][0] != b[name][0]:
            count = lambda code: sum(not line.endswith(":") for line in code)
            print(f"differs    {name}\n    instructions {count(a[name][0])} -> {count(b[name][0])}")
            for key in RESOURCES:
                print(f"    {key} {a[name][1].get(key)} -> {b[name][1].get(key)}")
        else:
            print(f"identical  {name}")
            continue
        bad += 1
    print(f"{len(a)} kernels in {sys.argv[1]}, {len(b)} in {sys.argv[2]}, {bad} differing or missing")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
