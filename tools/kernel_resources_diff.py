#!/usr/bin/env python3
"""The compiler's resource-usage table of every kernel of the device library, and the difference between two such tables.  Needs hipcc, no GPU.
(tools/kernel_resources.py reads the same figures from the assembly listing of one tree; this one covers the host unit too and compares two trees.)

Each translation unit of raytracer_amd/csrc is compiled as __graft_entry__.build() compiles it, plus -Rpass-analysis=kernel-resource-usage:

  hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -fvisibility=hidden [-mllvm -simplifycfg-sink-common=false: rt_shade, rt_tail]
        -Rpass-analysis=kernel-resource-usage -c raytracer_amd/csrc/<unit>.hip -o <tmp>/<unit>.o

and the remarks become one line per kernel: unit, SGPRs, VGPRs, AGPRs, scratch bytes per lane, SGPR / VGPR spills, waves per SIMD, LDS bytes per block, demangled
name.  A trailing `false` template argument of k_trace is dropped from the name, so that tables from before and after k_trace<kStack, kCount> gained its
defaulted third argument line up; and of k_temporal<kMoving, kClip, kDeform> alike.

  python tools/kernel_resources_diff.py                         > table.txt     # this tree (--root DIR: another checkout, e.g. a `git worktree` of the parent commit)
  python tools/kernel_resources_diff.py --against parent.txt                    # this tree's table, then what differs from parent.txt"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

UNITS = (("rt_runtime", []), ("rt_trace", []), ("rt_shade", ["-mllvm", "-simplifycfg-sink-common=false"]), ("rt_tail", ["-mllvm", "-simplifycfg-sink-common=false"]))
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-fvisibility=hidden", "-Rpass-analysis=kernel-resource-usage"]
FIELDS = ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "SGPRs Spill", "VGPRs Spill", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]")
HEADER = "%-11s %5s %5s %5s %7s %6s %6s %5s %6s  %s" % ("unit", "SGPRs", "VGPRs", "AGPRs", "scratch", "sSpill", "vSpill", "waves", "LDS", "kernel")


def remarks_of(root, unit, extra, tmp, hipcc):
    cmd = [hipcc] + FLAGS + extra + ["-c", os.path.join(root, "raytracer_amd", "csrc", unit + ".hip"), "-o", os.path.join(tmp, unit + ".o")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit("%s failed:\n%s" % (" ".join(cmd), r.stderr[-4000:]))
    return r.stderr


def table_of(root, hipcc):
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        for unit, extra in UNITS:
            kernels, current = {}, None
            for line in remarks_of(root, unit, extra, tmp, hipcc).splitlines():
                m = re.search(r"remark: .*Function Name: (\S+)", line)
                if m:
                    current = kernels.setdefault(m.group(1), {})
                    continue
                m = re.search(r"remark:\s+([^:]+): (\S+)", line)
                if m and current is not None:
                    current[m.group(1).strip()] = m.group(2)
            names = subprocess.run(["c++filt"] + list(kernels), capture_output=True, text=True).stdout.splitlines()
            for mangled, name in zip(kernels, names):
                name = re.sub(r"(k_trace<\d+, (?:true|false)), false>", r"\1>", name)
                name = re.sub(r"(k_temporal<(?:true|false), (?:true|false)), false>", r"\1>", name)   # (and of k_temporal<kMoving, kClip, kDeform>)
                name = re.sub(r"\(.*$", "", name)   # the argument list adds nothing: a kernel's name and template arguments identify it
                rows.append("%-11s %5s %5s %5s %7s %6s %6s %5s %6s  %s" % ((unit,) + tuple(kernels[mangled].get(f, "?") for f in FIELDS) + (name,)))
    return sorted(rows, key=lambda r: (r.split()[0], r.split(None, 9)[9]))


def keyed(rows):
    return {(r.split()[0], r.split(None, 9)[9]): r for r in rows if r and not r.startswith(("unit ", "#"))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--hipcc", default=os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
    ap.add_argument("--against", help="a table this tool printed earlier: list what differs")
    args = ap.parse_args()
    rows = table_of(args.root, args.hipcc)
    print(HEADER)
    print("\n".join(rows))
    if args.against:
        ours, theirs = keyed(rows), keyed(open(args.against).read().splitlines())
        same = [k for k in ours if k in theirs and ours[k].split()[1:9] == theirs[k].split()[1:9]]
        print("\n# against %s: %d kernels identical in every column" % (os.path.basename(args.against), len(same)))
        for k in ours:
            if k in theirs and k not in same:
                print("# differs: %s\n#   there: %s" % (ours[k], theirs[k]))
        for k in ours:
            if k not in theirs:
                print("# new:     %s" % ours[k])
        for k in theirs:
            if k not in ours:
                print("# gone:    %s" % theirs[k])


if __name__ == "__main__":
    main()
