"""Is the compiled code of this tree the code of another revision?  (No GPU.)

For a git revision (default: the parent, HEAD for uncommitted work) and for the working tree, compiles every
file of the Makefile's SRCS_DEV for the device alone with the Makefile's COMMON and DEVICE flags, and compares
per file (a) the bytes of .text and (b) llvm-readelf --notes (kernel names, VGPR / SGPR counts, spills,
scratch, LDS).  The whole object is not compared: two builds of one source differ outside those sections.
--host compares instead the .text* sections of the SRCS_HOST objects (--cuda-host-only).
One line per file; exit status 1 on any difference.

Usage: python tools/device_code_diff.py [--rev REV] [--host] [--keep DIR] [-DNAME=VALUE ...]"""
import argparse
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join("raytracercpp_amd", "csrc")
JOBS = 8


def make_vars(makefile):
    """The Makefile's plain assignments, $(NAME) expanded (EXTRA empty)."""
    raw = {}
    for line in open(makefile):
        m = re.match(r"^(\w+)\s*\??=\s*(.*)$", line.rstrip("\n"))
        if m:
            raw[m.group(1)] = m.group(2).strip()
    raw["EXTRA"] = ""

    def expand(s):
        return re.sub(r"\$\((\w+)\)", lambda m: expand(raw.get(m.group(1), "")), s)

    return {k: expand(v) for k, v in raw.items()}


def run(cmd, **kw):
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, **kw)
    if r.returncode != 0:
        sys.exit("%s\n%s" % (" ".join(cmd), r.stderr.decode(errors="replace")))
    return r.stdout


def compile_one(tree, out_dir, src, host, defines):
    """Returns (text bytes, notes) of src compiled in tree."""
    csrc = os.path.join(tree, CSRC)
    v = make_vars(os.path.join(csrc, "Makefile"))
    llvm = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(v["HIPCC"]))), "llvm", "bin")
    obj = os.path.join(out_dir, src + ".o")
    side = ["--cuda-host-only"] if host else ["--cuda-device-only", "--no-gpu-bundle-output"]
    run([v["HIPCC"]] + v["COMMON"].split() + v["DEVICE"].split() + side + defines + ["-c", "-x", "hip", "-o", obj, src],
        cwd=csrc)
    if not host:
        txt = obj + ".text"
        run([os.path.join(llvm, "llvm-objcopy"), "-O", "binary", "--only-section=.text", obj, txt])
        notes = run([os.path.join(llvm, "llvm-readelf"), "--notes", obj]).decode()
        return open(txt, "rb").read(), notes
    # host: functions defined in headers have sections of their own (.text.<symbol>)
    names = sorted(set(re.findall(r"\]\s+(\.text\S*)\s+PROGBITS", run([os.path.join(llvm, "llvm-readelf"), "-S", "-W", obj]).decode())))
    text = b""
    for i in range(0, len(names), 256):
        part = names[i:i + 256]
        run([os.path.join(llvm, "llvm-objcopy")] +
            ["--dump-section=%s=%s.s%d" % (n, obj, i + k) for k, n in enumerate(part)] + [obj, obj + ".copy"])
        for k, n in enumerate(part):
            text += n.encode() + b"\0" + open("%s.s%d" % (obj, i + k), "rb").read()
    return text, ""


def first_diff(a, b):
    la, lb = a.splitlines(), b.splitlines()
    for x, y in zip(la, lb):
        if x != y:
            return "%s | %s" % (x.strip(), y.strip())
    return "%d | %d lines" % (len(la), len(lb))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rev", help="the revision to compare the working tree with (default: the parent)")
    ap.add_argument("--host", action="store_true", help="the host objects' .text instead")
    ap.add_argument("--keep", help="a directory to keep the objects in")
    args, defines = ap.parse_known_args()
    bad = [d for d in defines if not d.startswith("-D")]
    if bad:
        ap.error("only -D flags are passed on: %s" % " ".join(bad))
    if not args.rev:
        # the parent of the work: HEAD while the sources have uncommitted changes, HEAD~1 once committed
        dirty = subprocess.run(["git", "-C", ROOT, "diff", "--quiet", "HEAD", "--", CSRC, "include"]).returncode != 0
        args.rev = "HEAD" if dirty else "HEAD~1"

    with tempfile.TemporaryDirectory() as tmp:
        work = args.keep or tmp
        rev_tree = os.path.join(work, "rev")
        os.makedirs(rev_tree, exist_ok=True)
        tar = run(["git", "-C", ROOT, "archive", args.rev, CSRC, "include"])
        subprocess.run(["tar", "-x", "-C", rev_tree], input=tar, check=True)
        trees = {"rev": rev_tree, "tree": ROOT}
        files = {k: make_vars(os.path.join(t, CSRC, "Makefile"))["SRCS_HOST" if args.host else "SRCS_DEV"].split()
                 for k, t in trees.items()}
        if files["rev"] != files["tree"]:
            sys.exit("the file lists differ: %s | %s" % (files["rev"], files["tree"]))
        jobs = {}
        with ThreadPoolExecutor(JOBS) as pool:
            for k, t in trees.items():
                out_dir = os.path.join(work, "obj_" + k)
                os.makedirs(out_dir, exist_ok=True)
                for f in files[k]:
                    jobs[k, f] = pool.submit(compile_one, t, out_dir, f, args.host, defines)
        print("%s against %s, %s%s" % ("working tree", run(["git", "-C", ROOT, "rev-parse", "--short", args.rev]).decode().strip(),
                                       "host" if args.host else "device", "".join(" " + d for d in defines)))
        ndiff = 0
        for f in files["tree"]:
            (ta, na), (tb, nb) = jobs["rev", f].result(), jobs["tree", f].result()
            what = []
            if ta != tb:
                what.append(".text differs (%d | %d bytes)" % (len(ta), len(tb)))
            if na != nb:
                what.append("notes differ: " + first_diff(na, nb))
            ndiff += bool(what)
            print("%-22s %s" % (f, "; ".join(what) if what else
                                "identical (.text %d bytes%s)" % (len(tb), "" if args.host else ", notes %d lines" % len(nb.splitlines()))))
        return 1 if ndiff else 0


if __name__ == "__main__":
    sys.exit(main())
