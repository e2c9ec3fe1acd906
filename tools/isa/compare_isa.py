#!/usr/bin/env python3
"""Compare two gfx950 .s files (hipcc ... --cuda-device-only -S of the same source at two commits) kernel by kernel: the text of
every function from its `_Z...:` label to `.Lfunc_end`, comments and blank lines stripped, the function's ordinal in local labels
(.LBB<n>_<k>) dropped.  Prints one line per function -- identical / differs / only in A / only in B -- and the counts; exit
status 1 if any function differs or exists on one side only.
usage: compare_isa.py parent.s commit.s [--quiet]   (--quiet: list only what is not identical)"""
import re, sys


def functions(path):
    """{mangled name: [instruction and label lines]} of every function of the file, in file order"""
    lines = open(path).read().split("\n")
    names = {m.group(1) for m in (re.match(r"^\s*\.type\s+(_Z\w+),@function", l) for l in lines) if m}
    out, cur = {}, None
    for l in lines:
        m = re.match(r"^(_Z\w+):", l)
        if m and m.group(1) in names and cur is None:
            cur = m.group(1)
            out[cur] = []
            continue
        if cur is None:
            continue
        if l.startswith(".Lfunc_end"):
            cur = None
            continue
        s = re.sub(r"\s+", " ", re.sub(r"(;|//).*$", "", l)).strip()
        if s:
            out[cur].append(re.sub(r"\.L(BB|JTI|tmp)\d+_", r".L\1_", s))
    return out


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if len(args) != 2:
        sys.exit(__doc__)
    quiet = "--quiet" in sys.argv
    a, b = functions(args[0]), functions(args[1])
    same = bad = 0
    for name in list(a) + [n for n in b if n not in a]:
        if name not in b: verdict = "only in A"
        elif name not in a: verdict = "only in B"
        elif a[name] == b[name]: verdict = "identical"
        else: verdict = f"differs ({len(a[name])} -> {len(b[name])} lines)"
        same += verdict == "identical"
        bad += verdict != "identical"
        if not (quiet and verdict == "identical"):
            print(f"{verdict:<12} {name}")
    print(f"{same + bad} functions: {same} identical, {bad} not")
    sys.exit(1 if bad else 0)


main()
