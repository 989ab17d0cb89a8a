"""Did the device code move?  Compares the gfx950 code objects of two builds: two libraries, or two object directories.

    python tools/codeobj_diff.py A/libpsdr_hip.so B/libpsdr_hip.so
    python tools/codeobj_diff.py A/lib/obj B/lib/obj                  # api_*.o by name: says which unit moved

Per code object: the set of kernel symbols, the disassembly (`llvm-objdump -d`) and the metadata notes (`llvm-readelf --notes`: registers,
scratch, LDS and kernarg size of every kernel), each without the line that names the file.  Not the bytes: a code object embeds the name
of the source it was compiled from, so the same kernels compiled from a renamed source hash differently.  Prints the first difference of
every code object that has one and exits 1; exits 0 when there is none.  Needs no GPU."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "psdr_jit_amd"))
import isa_lint  # noqa: E402  (by path: needs none of the package's native libraries)

READELF = os.path.join(os.path.dirname(isa_lint.OBJDUMP or ""), "llvm-readelf")


def _lines(tool, flag, path):
    out = subprocess.run([tool, flag, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, check=True).stdout
    return [l for l in out.split("\n") if path not in l]


def describe(path):
    """(kernel symbols, disassembly lines, note lines) of one code object"""
    notes = _lines(READELF, "--notes", path)
    kernels = sorted(m.group(1) for l in notes for m in [re.match(r"\s*\.symbol:\s*'?([^']+?)'?\s*$", l)] if m)
    return kernels, _lines(isa_lint.OBJDUMP, "-d", path), notes


def bundles(path, tmp):
    """{label: code object file} of a library (by position: one per linked unit) or of a directory of objects (by file name)"""
    files = sorted(f for f in os.listdir(path) if f.endswith(".o")) if os.path.isdir(path) else [None]
    found = {}
    for f in files:
        sub = tempfile.mkdtemp(dir=tmp)
        objs = isa_lint.code_objects(os.path.join(path, f) if f else path, sub)
        for i, o in enumerate(objs):
            found[f if f and len(objs) == 1 else "%s#%d" % (f or "code object", i)] = o
    return found


def first_difference(a, b):
    """a, b: describe() of the two code objects; None when they are the same"""
    (ka, da, na), (kb, db, nb) = a, b
    if ka != kb:
        return "kernel symbols: only in A %s, only in B %s" % (sorted(set(ka) - set(kb)), sorted(set(kb) - set(ka)))
    for what, xa, xb in (("disassembly", da, db), ("notes", na, nb)):
        for i, (la, lb) in enumerate(zip(xa, xb)):
            if la != lb:
                return "%s line %d:\n    A: %s\n    B: %s" % (what, i + 1, la.strip(), lb.strip())
        if len(xa) != len(xb):
            return "%s: %d lines in A, %d in B" % (what, len(xa), len(xb))
    return None


def main(argv):
    if len(argv) != 2:
        sys.stderr.write(__doc__)
        return 2
    if not isa_lint.available() or not os.path.exists(READELF):
        sys.stderr.write("codeobj_diff: llvm-objdump / llvm-readelf not found\n")
        return 2
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        A, B = bundles(argv[0], tmp), bundles(argv[1], tmp)
        for label in sorted(set(A) | set(B)):
            if label not in A or label not in B:
                print("%s: DIFFERENT - only in %s" % (label, "A" if label in A else "B"))
                bad += 1
                continue
            a, b = describe(A[label]), describe(B[label])
            diff = first_difference(a, b)
            print("%s: %s" % (label, "identical (%d kernels, %d lines of disassembly)" % (len(a[0]), len(a[1])) if diff is None else "DIFFERENT - " + diff))
            bad += diff is not None
    print("%d code object(s) differ" % bad if bad else "no difference")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
