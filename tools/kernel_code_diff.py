#!/usr/bin/env python3
"""Code size and code identity of every kernel (and out-of-line device function) of the two kernel units (rt_trace, rt_shade) in two trees.  Needs hipcc and the LLVM binary tools, no GPU.
(tools/kernel_resources_diff.py compares the compiler's resource table, which does not show a kernel whose schedule moved within the same registers.)

Each unit of both trees is compiled as __graft_entry__.build() compiles it, to a device code object:

  hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -fvisibility=hidden [-mllvm -simplifycfg-sink-common=false: rt_shade] --cuda-device-only -c <unit>.hip

unbundled (clang-offload-bundler), and every function symbol is listed with its size in bytes in both and one of
  same bytes   the function's bytes are the other tree's
  same code*   the same size and, instruction for instruction, the same disassembly once the 32-bit literals of `s_add_u32 / s_addc_u32 sN, sN, literal` are masked:
               pc-relative offsets of a kernel whose distance to the unit's constant tables moved because other kernels grew
  DIFFERS, new, gone   (a kernel whose argument list changed is `gone` under its old mangled name and `new` under the other)
A kernel that is `gone` and one that is `new` under the same name and template arguments are one kernel whose mangled name moved -- a type of its argument list was
renamed, or, for k_temporal, the defaulted third template argument (kDeform) was added behind the two it had: a trailing `false` of k_temporal<a, b, false> is
dropped, as tools/kernel_resources_diff.py drops k_trace's --: they are compared as one, and the state carries a `~` (same bytes~: the renamed kernel holds the
parent's bytes).

  python tools/kernel_code_diff.py --parent <a git worktree of the parent commit> [--root <this tree>]"""
import argparse
import hashlib
import os
import re
import subprocess
import sys
import tempfile

UNITS = (("rt_trace", []), ("rt_shade", ["-mllvm", "-simplifycfg-sink-common=false"]))
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-fvisibility=hidden", "--cuda-device-only"]


def run(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit("%s failed:\n%s" % (" ".join(cmd), r.stderr[-4000:]))
    return r.stdout


def code_object(root, unit, extra, tmp, label, hipcc, llvm):
    bundle, elf = os.path.join(tmp, "%s_%s.co" % (label, unit)), os.path.join(tmp, "%s_%s.elf" % (label, unit))
    run([hipcc] + FLAGS + extra + ["-c", os.path.join(root, "raytracer_amd", "csrc", unit + ".hip"), "-o", bundle])
    run([os.path.join(llvm, "clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + bundle, "--output=" + elf, "--unbundle"])
    return elf


def functions(elf, llvm):
    """mangled name -> (size, sha1 of the function's bytes)"""
    m = re.search(r"\]\s+\.text\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)", run([os.path.join(llvm, "llvm-readelf"), "-SW", elf]))
    address, offset = int(m.group(1), 16), int(m.group(2), 16)
    data = open(elf, "rb").read()
    out = {}
    for line in run([os.path.join(llvm, "llvm-readelf"), "-sW", elf]).splitlines():
        f = line.split()
        if len(f) >= 8 and f[3] == "FUNC" and int(f[2]):
            start = offset + int(f[1], 16) - address
            out[f[7]] = (int(f[2]), hashlib.sha1(data[start:start + int(f[2])]).hexdigest())
    return out


def listing(elf, name, llvm):
    lines = run([os.path.join(llvm, "llvm-objdump"), "-d", "--no-show-raw-insn", "--disassemble-symbols=" + name, elf]).splitlines()[6:]
    lines = [re.sub(r"^\s*[0-9a-f]+:", "", re.sub(r"//.*", "", line)).strip() for line in lines]
    return [re.sub(r"^(s_addc?_u32 (s\d+), \2, )0x[0-9a-f]{6,8}$", r"\1<pc-relative>", line) for line in lines]


def plain_name(demangled):
    """name and template arguments: what identifies a kernel whatever its argument list is spelled as"""
    name = re.sub(r"\(.*$", "", demangled)
    return re.sub(r"(k_temporal<(?:true|false), (?:true|false)), false>", r"\1>", name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="the tree to compare against, e.g. a `git worktree` of the parent commit")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--hipcc", default=os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
    ap.add_argument("--llvm-bin", default="/opt/rocm/llvm/bin")
    args = ap.parse_args()
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        for unit, extra in UNITS:
            then_elf = code_object(args.parent, unit, extra, tmp, "parent", args.hipcc, args.llvm_bin)
            now_elf = code_object(args.root, unit, extra, tmp, "this", args.hipcc, args.llvm_bin)
            then, now = functions(then_elf, args.llvm_bin), functions(now_elf, args.llvm_bin)
            names = sorted(set(then) | set(now))
            plain = dict(zip(names, (plain_name(p) for p in run(["c++filt"] + names).splitlines())))
            # a kernel gone under one mangled name and new under another, with the same name and template arguments: one kernel, renamed
            gone, new = [n for n in names if n not in now], [n for n in names if n not in then]
            renamed = {}
            for n in gone:
                twins = [m for m in new if plain[m] == plain[n]]
                if len(twins) == 1 and sum(plain[g] == plain[n] for g in gone) == 1:
                    renamed[n] = twins[0]
            for name in names:
                if name in renamed.values():
                    continue
                other = renamed.get(name, name)
                a, b = then.get(name), now.get(other)
                state = "new" if a is None else "gone" if b is None else "same bytes" if a == b else "DIFFERS"
                if state == "DIFFERS" and a[0] == b[0] and listing(then_elf, name, args.llvm_bin) == listing(now_elf, other, args.llvm_bin):
                    state = "same code*"
                rows.append((unit, a[0] if a else "-", b[0] if b else "-", state + ("~" if other != name else ""), plain[name]))
    print("%-9s %8s %8s  %-10s %s" % ("unit", "parent", "this", "code", "kernel"))
    for row in rows:
        print("%-9s %8s %8s  %-10s %s" % row)
    renamed = sum(r[3].endswith("~") for r in rows)
    count = lambda state: sum(r[3].rstrip("~") == state for r in rows)   # noqa: E731
    print("# %d functions hold the parent's bytes, %d its instructions with other pc-relative offsets (*); %d differ, %d new, %d gone; %d of them under another mangled name (~)" % (
        count("same bytes"), count("same code*"), count("DIFFERS"), count("new"), count("gone"), renamed))


if __name__ == "__main__":
    main()
