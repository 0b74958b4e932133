#!/usr/bin/env python3
"""Do two device assembly files (hipcc --cuda-device-only -S) hold the same kernels?

    python3 tools/isa_same.py parent.s branch.s

Splits each file into kernels, normalises each kernel's body (comments and blank lines dropped, mangled names replaced by one
token, the function index taken out of local labels) and its .amdhsa_ resource block (the kernel's name dropped), and matches
the kernels of the two files by that text alone: names may differ.  Prints the kernel counts and, for every kernel of one file
without a twin in the other, its name and the unified diff against the nearest unmatched body of the other file.  Exit status 0
if every kernel has a twin.  Nothing else in the files is looked at.
"""
import collections
import difflib
import re
import sys

_NAME = re.compile(r"\b_Z\w+")
_LABEL = re.compile(r"\.L(BB|JTI|func_end|func_begin|tmp)\d+")


def _norm(line):
    line = line.split(";", 1)[0].rstrip()
    line = _NAME.sub("SYM", line)
    return _LABEL.sub(lambda m: ".L" + m.group(1), line).strip()


def kernels(path):
    """{name: (body lines, resource block lines)}"""
    out, body, res, name, state = {}, [], [], None, None
    for raw in open(path):
        s = raw.strip()
        if state is None:
            m = re.match(r"(_Z\w+):", s)
            if m:
                name, body, res, state = m.group(1), [], [], "body"
        elif state == "body":
            if s.startswith(".amdhsa_kernel "):
                state = "res"
            elif s.startswith(".section") or s.startswith(".p2align"):
                continue
            else:
                n = _norm(raw)
                if n:
                    body.append(n)
        elif state == "res":
            if s.startswith(".end_amdhsa_kernel"):
                out[name] = (tuple(body), tuple(res))
                state = None
            else:
                res.append(s)
    return out


def main(a_path, b_path):
    a, b = kernels(a_path), kernels(b_path)
    print(f"kernels: {len(a)} in {a_path}, {len(b)} in {b_path}")
    left = collections.defaultdict(list)
    for name, key in b.items():
        left[key].append(name)
    lone_a = []
    for name, key in a.items():
        if left[key]:
            left[key].pop()
        else:
            lone_a.append(name)
    lone_b = [n for names in left.values() for n in names]
    print(f"matched by body and resource block: {len(a) - len(lone_a)}; without a twin: {len(lone_a)} / {len(lone_b)}")
    for name in lone_a:
        print(f"\n--- {name}")
        if not lone_b:
            continue
        near = max(lone_b, key=lambda n: difflib.SequenceMatcher(None, a[name][0], b[n][0], autojunk=False).quick_ratio())
        print(f"+++ {near}")
        for side in (0, 1):
            diff = list(difflib.unified_diff(a[name][side], b[near][side], lineterm="", n=2))
            for line in diff[2:400]:
                print(line)
    for name in lone_b:
        print(f"\n+++ only in {b_path}: {name}")
    return 0 if len(a) == len(b) and not lone_a and not lone_b else 1


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
