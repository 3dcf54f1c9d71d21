#!/usr/bin/env python3
"""Is the device code of two builds of one source the same?  usage: cmp_kernel_asm.py old.s new.s

Both files come from the csrc Makefile's build/%.s rule.  For every kernel of new.s the instruction stream between its label and its
.Lfunc_end, and its .amdhsa_ resource block (registers, LDS, scratch), must equal the old ones -- after dropping `;` comments and
trailing blanks and renumbering local labels (.LBB<function>_<block>) by first appearance.  Kernels only old.s has are listed as removed.
Exit status 1 if a kernel of new.s differs or is new."""
import re
import shutil
import subprocess
import sys


def kernels(path):
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^\t\.amdhsa_kernel (\S+)\n(.*?)^\t\.end_amdhsa_kernel", text, re.M | re.S):
        name = m.group(1)
        body = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end\d+:" % re.escape(name), text, re.M | re.S).group(1)
        lines = [l.split(";")[0].rstrip() for l in body.split("\n")]
        body = "\n".join(l for l in lines if l)
        labels = {}
        body = re.sub(r"\.L\w+", lambda l: labels.setdefault(l.group(0), ".L%d" % len(labels)), body)
        out[name] = (body, m.group(2))
    return out


def pretty(names):
    tool = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    if not tool:
        return dict(zip(names, names))
    res = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return {n: r.replace("(anonymous namespace)::", "").split("(")[0] for n, r in zip(names, res)}


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    show = pretty(sorted(set(old) | set(new)))
    bad = 0
    for name in sorted(new, key=show.get):
        if name not in old:
            verdict = "NEW"
        else:
            diffs = [what for what, a, b in zip(("instructions", "resources"), old[name], new[name]) if a != b]
            verdict = "DIFFERENT " + " + ".join(diffs) if diffs else "identical"
        bad += verdict != "identical"
        ninstr = sum(1 for l in new[name][0].split("\n") if l.startswith("\t") and not l.startswith("\t."))
        print("%-46s %6d instructions  %s" % (show[name], ninstr, verdict))
    for name in sorted(set(old) - set(new), key=show.get):
        print("%-46s removed" % show[name])
    print("%d kernels compared, %d not identical" % (len(new), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
