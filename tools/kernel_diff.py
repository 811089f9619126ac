#!/usr/bin/env python3
"""Compare the gfx950 kernels of two builds of the library, byte for byte.  No GPU, no timing.

    tools/kernel_diff.py A B [--rename REGEX REPLACEMENT]... [--only REGEX] [--llvm-bin DIR]

A and B are libraries, or bare code objects (hipcc --cuda-device-only --no-gpu-bundle-output -c: one translation unit, a minute).
For every kernel (by demangled name, over all translation units of a library) it compares
  * the instruction bytes of the kernel's symbol, and
  * its metadata entry: vgpr_count, agpr_count, sgpr_count, private_segment_fixed_size (scratch), group_segment_fixed_size
    (static LDS) and kernarg_segment_size.
It prints the kernels found on one side only, the kernels that differ (with both sets of numbers) and the number of identical
ones, and exits 1 on any difference.

--rename rewrites the demangled names of A before matching (re.sub), for a refactor that changes a template's parameter list:
    --rename 'maxsim_stream_kernel<(\\d+), (\\d+), (\\w+), (\\d+), true, (\\w+)>' 'maxsim_stream_kernel<\\1, \\2, \\3, \\4, \\5>'
--only restricts the comparison to the names (after renaming) that match.

The code objects are extracted with `llvm-objdump --offloading` into a temporary directory; addresses, sizes and metadata come
from `llvm-readelf`.  The tool compares bytes and numbers; it does not disassemble.
"""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

META_KEYS = ("vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size",
             "kernarg_segment_size")


def run(cmd, **kw):
    return subprocess.run(cmd, check=True, stdout=subprocess.PIPE, universal_newlines=True, **kw).stdout


def code_objects(lib, llvm_bin, work):
    """extract the gfx950 code objects of `lib` (one per translation unit) into `work`; a bare code object stands for itself"""
    with open(lib, "rb") as f:
        head = f.read(20)
    if head[:4] == b"\x7fELF" and head[18:20] == b"\xe0\x00":      # e_machine = EM_AMDGPU
        return [lib]
    local = os.path.join(work, os.path.basename(lib))
    shutil.copy(lib, local)
    run([os.path.join(llvm_bin, "llvm-objdump"), "--offloading", os.path.basename(local)], cwd=work)
    prefix = os.path.basename(local) + "."
    objs = sorted(os.path.join(work, f) for f in os.listdir(work) if f.startswith(prefix) and "amdgcn" in f and f.endswith("gfx950"))
    if not objs:
        sys.exit("%s: no gfx950 code object found" % lib)
    return objs


def sections(obj, llvm_bin):
    """section index -> (address, file offset)"""
    out = {}
    for line in run([os.path.join(llvm_bin, "llvm-readelf"), "-SW", obj]).splitlines():
        m = re.match(r"\s*\[\s*(\d+)\]\s+(\S*)\s+(\S+)\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", line)
        if m:
            out[int(m.group(1))] = (int(m.group(4), 16), int(m.group(5), 16))
    return out


def kernel_metadata(obj, llvm_bin):
    """mangled kernel name -> {key: value} from the NT_AMDGPU_METADATA note"""
    text = run([os.path.join(llvm_bin, "llvm-readelf"), "--notes", obj])
    meta = {}
    in_kernels = False
    cur = None
    for line in text.splitlines():
        if line.startswith("amdhsa.kernels:"):
            in_kernels = True
            continue
        if in_kernels and re.match(r"\S", line):        # the next top-level key ends the list
            in_kernels = False
        if not in_kernels:
            continue
        m = re.match(r"  (-| ) \.(\w+):\s*(.*)$", line)      # a key of a kernel entry (list items start with "  - ")
        if not m:
            continue
        if m.group(1) == "-":
            cur = {}
        key, val = m.group(2), m.group(3).strip().strip("'\"")
        if key == "name":
            meta[val] = cur
        elif key in META_KEYS:
            cur[key] = int(val)
    return meta


def kernels(lib, llvm_bin, work):
    """demangled kernel name -> [(instruction bytes, metadata)], one per code object that defines it"""
    out = {}
    readelf = os.path.join(llvm_bin, "llvm-readelf")
    for obj in code_objects(lib, llvm_bin, work):
        sec = sections(obj, llvm_bin)
        meta = kernel_metadata(obj, llvm_bin)
        with open(obj, "rb") as f:
            blob = f.read()
        found = set()
        # the symbol table twice, in the same order: the metadata knows the mangled names, people read the demangled ones
        for line, pretty in zip(run([readelf, "-sW", obj]).splitlines(), run([readelf, "-sW", "--demangle", obj]).splitlines()):
            p = line.split()
            if len(p) < 8 or p[3] != "FUNC" or p[7] not in meta or p[7] in found:     # (.dynsym and .symtab both list a kernel)
                continue
            addr, size, ndx = int(p[1], 16), int(p[2]), int(p[6])
            if pretty.split()[:7] != p[:7]:             # the two listings must describe the same symbol line by line
                sys.exit("%s: the demangled symbol table does not line up with the plain one at %s" % (obj, p[7]))
            s_addr, s_off = sec[ndx]
            found.add(p[7])
            # a kernel that several translation units instantiate appears once per unit: all copies are kept
            out.setdefault(pretty.split(None, 7)[7], []).append((blob[s_off + addr - s_addr: s_off + addr - s_addr + size], meta[p[7]]))
        missing = [k for k in meta if k not in found]
        if missing:
            sys.exit("%s: no symbol for kernel %s" % (obj, missing[0]))
    return out


def load(lib, llvm_bin, renames, only):
    with tempfile.TemporaryDirectory() as work:
        ks = kernels(lib, llvm_bin, work)
    out = {}
    for name, val in ks.items():
        for pat, rep in renames:
            name = re.sub(pat, rep, name)
        if only and not re.search(only, name):
            continue
        if name in out:
            sys.exit("%s: two kernels are called %s after renaming" % (lib, name))
        out[name] = sorted(val, key=lambda cm: (cm[0], sorted(cm[1].items())))
    return out


def fmt_meta(m):
    return "  ".join("%s=%s" % (k.replace("_segment", "").replace("_fixed_size", ""), m.get(k, "?")) for k in META_KEYS)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--rename", nargs=2, action="append", default=[], metavar=("REGEX", "REPLACEMENT"),
                    help="rewrite the demangled kernel names of A before matching")
    ap.add_argument("--only", default=None, metavar="REGEX", help="compare only the kernels whose name matches")
    ap.add_argument("--llvm-bin", default=os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin"))
    args = ap.parse_args()

    a = load(args.a, args.llvm_bin, args.rename, args.only)
    b = load(args.b, args.llvm_bin, [], args.only)
    only_a = sorted(set(a) - set(b))
    only_b = sorted(set(b) - set(a))
    same, differ = 0, []
    for name in sorted(set(a) & set(b)):
        if a[name] == b[name]:
            same += 1
            continue
        if len(a[name]) != len(b[name]):
            print("defined %d times in A, %d times in B: %s" % (len(a[name]), len(b[name]), name))
        # every differing copy of a kernel that several translation units define is reported
        pairs = [(x, y) for x, y in zip(a[name], b[name]) if x != y] or [(a[name][0], b[name][0])]
        differ.append((name, pairs))

    for name in only_a:
        print("only in A: %s" % name)
    for name in only_b:
        print("only in B: %s" % name)
    for name, pairs in differ:
        what = [w for w, d in (("code", any(x[0] != y[0] for x, y in pairs)), ("metadata", any(x[1] != y[1] for x, y in pairs))) if d]
        print("differs (%s): %s" % (", ".join(what) or "number of copies", name))
        for (code_a, meta_a), (code_b, meta_b) in pairs:
            print("    A: %6d bytes  %s" % (len(code_a), fmt_meta(meta_a)))
            print("    B: %6d bytes  %s" % (len(code_b), fmt_meta(meta_b)))
    print("kernels: %d in A, %d in B; %d identical, %d differ, %d only in A, %d only in B"
          % (len(a), len(b), same, len(differ), len(only_a), len(only_b)))
    return 1 if (differ or only_a or only_b) else 0


if __name__ == "__main__":
    sys.exit(main())
