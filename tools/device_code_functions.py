"""Which functions of a device object differ from another build's?  (No GPU.)

tools/device_code_diff.py compares a file's whole .text and notes; after a change that adds kernels both
differ.  This compares, function by function, two objects that it kept (--keep DIR: DIR/obj_rev/FILE.o and
DIR/obj_tree/FILE.o): the bytes of each function's code, and each kernel's resource notes (registers, spills,
scratch, LDS, kernel arguments).  Functions whose bytes differ are disassembled: when the only differing
instructions are s_add_u32 / s_addc_u32 that directly follow an s_getpc_b64 (checked per instruction: the
PC-relative address of a called function, which moves when code is added to the file) the function counts as
unchanged.
Exit status 1 when an existing function differs otherwise, or an existing kernel's notes differ.

Usage: python tools/device_code_functions.py DIR/obj_rev/kernels.hip.o DIR/obj_tree/kernels.hip.o"""
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from device_code_diff import CSRC, ROOT, make_vars

HIPCC = make_vars(os.path.join(ROOT, CSRC, "Makefile"))["HIPCC"]
LLVM = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(HIPCC))), "llvm", "bin") + os.sep


def run(*a):
    return subprocess.run(a, check=True, stdout=subprocess.PIPE).stdout.decode()


def load(obj):
    secs = run(LLVM + "llvm-readelf", "-S", "-W", obj)
    m = re.search(r"\]\s+\.text\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", secs)
    addr, off, size = (int(x, 16) for x in m.groups())
    data = open(obj, "rb").read()
    funcs = {}
    for line in run(LLVM + "llvm-readelf", "-s", "-W", obj).splitlines():
        f = line.split()
        if len(f) >= 8 and f[3] == "FUNC":
            a, s = int(f[1], 16), int(f[2])
            funcs[f[7]] = data[off + a - addr: off + a - addr + s]
    notes = run(LLVM + "llvm-readelf", "--notes", obj)
    kern = {}
    for block in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
        block = ".agpr_count:" + block
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        keys = {}
        for k in (".agpr_count", ".vgpr_count", ".sgpr_count", ".sgpr_spill_count", ".vgpr_spill_count",
                  ".private_segment_fixed_size", ".group_segment_fixed_size", ".max_flat_workgroup_size",
                  ".kernarg_segment_size", ".uses_dynamic_stack", ".wavefront_size"):
            mm = re.search(re.escape(k) + r":\s+(\S+)", block)
            keys[k] = mm.group(1) if mm else None
        kern[name] = keys
    return funcs, kern


def disasm(obj, sym):
    out = run(LLVM + "llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", "--disassemble-symbols=" + sym, obj)
    return [re.sub(r"\s*//.*$", "", l).strip() for l in out.splitlines() if l.startswith("\t")]


moved = 0
rev, tree = sys.argv[1], sys.argv[2]
fa, ka = load(rev)
fb, kb = load(tree)
print("functions: %d in the parent's kernels.hip, %d in the working tree's" % (len(fa), len(fb)))
print("new functions:", ", ".join(sorted(set(fb) - set(fa))) or "none")
print("removed functions:", ", ".join(sorted(set(fa) - set(fb))) or "none")
same = diff = 0
for n in sorted(fa):
    if n not in fb:
        continue
    if fa[n] == fb[n]:
        same += 1
    else:
        diff += 1
        nd = sum(x != y for x, y in zip(fa[n], fb[n])) if len(fa[n]) == len(fb[n]) else -1
        what = ""
        if nd >= 0:
            da, db = disasm(rev, n), disasm(tree, n)
            ops = sorted({x.split()[0] + " / " + y.split()[0] for x, y in zip(da, db) if x != y})
            what = "; differing instructions (%d): %s" % (sum(x != y for x, y in zip(da, db)), ", ".join(ops))
            # an address computation: s_getpc_b64, then s_add_u32 and s_addc_u32 on its register pair
            back = {"s_add_u32": 1, "s_addc_u32": 2}
            after_getpc = all(x == y or (x.split()[0] in back and k >= back[x.split()[0]] and
                                         da[k - back[x.split()[0]]].startswith("s_getpc_b64") and
                                         db[k - back[x.split()[0]]].startswith("s_getpc_b64"))
                              for k, (x, y) in enumerate(zip(da, db)))
            if set(ops) <= {"s_add_u32 / s_add_u32", "s_addc_u32 / s_addc_u32"} and len(da) == len(db) and after_getpc:
                what += " -- the PC-relative addresses of called functions"
                moved += 1
        print("  .text differs: %s (%d | %d bytes, %s%s)" % (n, len(fa[n]), len(fb[n]),
                                                         "%d bytes differ" % nd if nd >= 0 else "sizes differ", what))
print("existing functions with identical .text: %d, with different .text: %d, of which %d differ only in the "
      "literals of s_add_u32 / s_addc_u32 after s_getpc_b64 (calls of functions that moved)" % (same, diff, moved))
print("kernels in the notes: %d in the parent, %d in the working tree" % (len(ka), len(kb)))
print("new kernels in the notes:", ", ".join(sorted(set(kb) - set(ka))) or "none")
nsame = 0
for n in sorted(ka):
    if ka[n] == kb.get(n):
        nsame += 1
    else:
        print("  notes differ: %s %s | %s" % (n, ka[n], kb.get(n)))
print("existing kernels with identical resource notes: %d of %d" % (nsame, len(ka)))
for n in sorted(set(kb) - set(ka)):
    print("  %s: %s" % (n, " ".join("%s=%s" % (k[1:], v) for k, v in kb[n].items())))
sys.exit(1 if diff != moved or nsame != len(ka) else 0)
