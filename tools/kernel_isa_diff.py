#!/usr/bin/env python3
"""Are the kernels of two builds the same instructions?

    hipcc <the Makefile's HIPFLAGS> --cuda-device-only -S old.hip -o old.s        (and the same for the new sources)
    tools/kernel_isa_diff.py --before old.s [more.s ...] --after new_a.s new_b.s [...]

Every kernel (a symbol with an .amdhsa_kernel descriptor) of the files on each side is reduced to its instruction text --
comments and assembler directives dropped, local labels renamed in order of appearance, white space squeezed -- and to
the lines of its descriptor block.  Printed per kernel: instruction count and a digest of each side, the descriptor's
register / LDS / scratch figures, and whether both the instructions and the whole descriptor are equal.  Exit status 1
if any kernel differs or exists on one side only.

The tool normalises and hashes; it knows nothing about particular instructions.
"""
import argparse
import hashlib
import re
import sys

LABEL = re.compile(r"\.L[A-Za-z0-9_$.]+")
SHOWN = ("next_free_vgpr", "next_free_sgpr", "accum_offset", "group_segment_fixed_size", "private_segment_fixed_size")


def strip_comment(line):
    for mark in (";", "//"):
        at = line.find(mark)
        if at >= 0:
            line = line[:at]
    return " ".join(line.split())


def kernels_of(path):
    """{kernel symbol: (instruction lines, descriptor lines)} of one .s file"""
    lines = open(path, errors="replace").read().splitlines()
    desc = {}
    for i, raw in enumerate(lines):
        t = raw.split()
        if len(t) == 2 and t[0] == ".amdhsa_kernel":
            body = []
            for d in lines[i + 1:]:
                d = strip_comment(d)
                if d == ".end_amdhsa_kernel":
                    break
                if d:
                    body.append(d)
            desc[t[1]] = body
    out = {}
    for name in desc:
        start = next(i for i, raw in enumerate(lines) if raw.startswith(name + ":"))
        text, names = [], {}
        for raw in lines[start + 1:]:
            if raw.startswith(".Lfunc_end"):
                break
            s = strip_comment(raw)
            if not s:
                continue
            is_label = s.endswith(":") and " " not in s
            if s.startswith(".") and not is_label:
                continue                                  # an assembler directive
            s = LABEL.sub(lambda m: names.setdefault(m.group(0), "L%d" % len(names)), s)
            text.append(s)
        out[name] = (text, desc[name])
    return out


def digest(lines):
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()[:16]


def figures(desc):
    got = dict(d.split(None, 1) for d in desc if " " in d)
    return " ".join("%s=%s" % (k, got.get(".amdhsa_" + k, "-")) for k in SHOWN)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--before", nargs="+", required=True, metavar="FILE.s")
    ap.add_argument("--after", nargs="+", required=True, metavar="FILE.s")
    ap.add_argument("--dump", metavar="DIR", help="also write each kernel's normalised text to DIR/<kernel>.before / .after, for diff(1)")
    args = ap.parse_args()
    sides = []
    for files in (args.before, args.after):
        side = {}
        for f in files:
            for name, k in kernels_of(f).items():
                if name in side:
                    sys.exit("%s: kernel %s is in more than one file of this side" % (f, name))
                side[name] = k + (f,)
        sides.append(side)
    before, after = sides
    bad = 0
    for name in sorted(set(before) | set(after)):
        print(name)
        if name not in before or name not in after:
            print("    ONLY %s (%s)" % (("before", before[name][2]) if name in before else ("after", after[name][2])))
            bad += 1
            continue
        (tb, db, fb), (ta, da, fa) = before[name], after[name]
        if args.dump:
            for ext, t in ((".before", tb), (".after", ta)):
                open("%s/%s%s" % (args.dump, name, ext), "w").write("\n".join(t) + "\n")
        ninstr = [sum(1 for s in t if not s.endswith(":")) for t in (tb, ta)]
        same_text, same_desc = tb == ta, db == da
        print("    before  %-28s %6d instructions  %s  descriptor %s" % (fb.split("/")[-1], ninstr[0], digest(tb), digest(db)))
        print("    after   %-28s %6d instructions  %s  descriptor %s" % (fa.split("/")[-1], ninstr[1], digest(ta), digest(da)))
        print("    before  %s" % figures(db))
        print("    after   %s" % figures(da))
        print("    instructions %s, descriptor %s" % ("EQUAL" if same_text else "DIFFERENT", "EQUAL" if same_desc else "DIFFERENT"))
        if not same_text:
            at = next((i for i, (x, y) in enumerate(zip(tb, ta)) if x != y), min(len(tb), len(ta)))
            print("    first difference at normalised line %d:\n      before: %s\n      after:  %s" %
                  (at, tb[at] if at < len(tb) else "(end)", ta[at] if at < len(ta) else "(end)"))
        for x in sorted(set(db) ^ set(da)):
            print("    descriptor line on one side only: %s" % x)
        bad += not (same_text and same_desc)
    print("%d kernels, %d different" % (len(set(before) | set(after)), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
