"""Compares the kernels of two sets of gfx950 device assembly listings, instruction for instruction.

Each listing is made with the Makefile's flags:  hipcc $(CXXFLAGS) -S --cuda-device-only -o FILE.s csrc/FILE.hip
A side may be several listings joined by commas (a kernel that moved to another translation unit is found in either).

python tools/listing_diff.py BEFORE.s[,MORE.s] AFTER.s[,MORE.s] [--only SUBSTRING]

Prints, per kernel of either side, both instruction counts and whether the two sequences agree once labels are blanked
(branch targets, and the kernel's own name where it appears as an operand).  Sequences only: no instruction is looked for.
Needs no GPU.  Exit status 1 if a kernel found on both sides differs."""
import re
import subprocess
import sys


def kernels(paths):
    """{demangled kernel name: [instruction lines, labels blanked]} of the .amdhsa_kernel symbols of the listings."""
    out = {}
    for path in paths.split(","):
        text = open(path).read()
        names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, flags=re.M))
        name = None
        for line in text.splitlines():
            s = line.split(";")[0].strip()
            m = re.match(r"^([A-Za-z_.$][\w.$]*):", s)
            if m and not m.group(1).startswith(".L"):
                name = m.group(1) if m.group(1) in names else None
                if name:
                    out[name] = []
            elif name and s.startswith(".Lfunc_end"):
                name = None
            elif name and s and not s.startswith(".") and not s.endswith(":"):
                out[name].append(re.sub(r"\.L\w+|_Z\w+", "L", s))
    if not out:
        return {}
    short = subprocess.run(["c++filt", *out], capture_output=True, text=True).stdout.splitlines()
    return {re.sub(r"\(anonymous namespace\)::|^void ", "", d): out[k] for d, k in zip(short, out)}


only = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else ""
a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
differ = 0
print("| kernel | instructions before | after | sequence |\n|---|---|---|---|")
for k in sorted(set(a) | set(b)):
    if only not in k:
        continue
    if k in a and k in b:
        same = a[k] == b[k]
        differ += not same
        print(f"| `{k}` | {len(a[k])} | {len(b[k])} | {'identical' if same else 'DIFFERS'} |")
    else:
        print(f"| `{k}` | {len(a[k]) if k in a else '-'} | {len(b[k]) if k in b else '-'} | only on one side |")
sys.exit(1 if differ else 0)
