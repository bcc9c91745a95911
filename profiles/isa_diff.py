#!/usr/bin/env python3
"""Hold the gfx950 code of every kernel of a change against the parent's, kernel by kernel.

    hipcc <the Makefile's CXXFLAGS> --save-temps -c <unit>.hip        (every unit, once on the parent, once on the change)
    python3 profiles/isa_diff.py [--symbols REGEX] PARENT.s... -- CHANGE.s...

Each side is any number of `*-hip-amdgcn-amd-amdhsa-gfx950.s` files: a kernel may move between units.  For every kernel whose symbol
matches REGEX (default `_ZN6legion`) two things are compared: the kernel descriptor's vgpr_count, sgpr_count, group_segment_fixed_size
(LDS bytes) and private_segment_fixed_size (scratch bytes), and the lines of the function body -- comments, blank lines and directives
dropped, and the local labels `.LBB<n>_<m>` rewritten to `.LBB_<m>`, since <n> is the function's index in its unit.  Text only: the
script knows no instruction.  Prints a markdown table; exit code 1 unless every kernel of the parent is in the change and identical."""
import argparse
import re
import subprocess
import sys

WORDS = ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")
LOCAL_LABEL = re.compile(r"\.L([A-Za-z_]+)\d+_(\d+)")


def kernels(paths, select):
    """symbol -> (the four words, [body lines]) of every selected kernel of the files"""
    out = {}
    for path in paths:
        bodies, words, name, block, functions = {}, {}, None, {}, set()
        for line in open(path):
            m = re.match(r"\s+\.type\s+(\w+),@function", line)
            if m:
                functions.add(m.group(1))
            m = re.match(r"(\w+):", line)
            if m and name is None and m.group(1) in functions:
                name, bodies[m.group(1)] = m.group(1), []
                continue
            if name is not None:
                if line.startswith(".Lfunc_end"):
                    name = None
                    continue
                text = re.sub(r"\s*;.*", "", line).strip()
                if text and (text.endswith(":") or not text.startswith(".")):
                    bodies[name].append(LOCAL_LABEL.sub(r".L\1_\2", text))
                continue
            m = re.match(r"\s+\.(name|%s):\s+(\S+)" % "|".join(WORDS), line)
            if m:
                block[m.group(1)] = m.group(2)
            elif line.strip().startswith(".wavefront_size"):   # the last word of a kernel's metadata entry
                words[block["name"]] = tuple(int(block[w]) for w in WORDS)
                block = {}
        for sym, w in words.items():
            if select.search(sym):
                if sym in out:
                    sys.exit("%s: kernel %s is in more than one file of this side" % (path, sym))
                out[sym] = (w, bodies[sym])
    return out


def demangled(symbols):
    try:
        r = subprocess.run(["c++filt"], input="\n".join(symbols), stdout=subprocess.PIPE, text=True, check=True)
        names = r.stdout.split("\n")[:len(symbols)]
    except (OSError, subprocess.CalledProcessError):
        names = symbols
    return {s: without_parameters(n) for s, n in zip(symbols, names)}


def without_parameters(name):
    """`void legion::k<float __vector(4), true>(legion::Args)` -> `legion::k<float __vector(4), true>`: the return type and the
    trailing parameter list go, parentheses inside the template arguments stay"""
    name = re.sub(r"^void ", "", name)
    if not name.endswith(")"):
        return name
    depth = 0
    for i in range(len(name) - 1, -1, -1):
        depth += (name[i] == ")") - (name[i] == "(")
        if depth == 0:
            return name[:i]
    return name


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--symbols", default="_ZN6legion", help="regex a kernel's symbol must match (default: %(default)s)")
    ap.add_argument("files", nargs="+", help="PARENT.s... -- CHANGE.s...")
    argv = sys.argv[1:]
    if "--" not in argv:
        ap.error("the parent's files and the change's are separated by --")
    cut = argv.index("--")
    a = ap.parse_args(argv[:cut])
    select = re.compile(a.symbols)
    P, C = kernels(a.files, select), kernels(argv[cut + 1:], select)
    if not P or not C:
        sys.exit("no kernel matches %r on one side" % a.symbols)
    names = demangled(sorted(set(P) | set(C)))
    count = lambda body: sum(1 for t in body if not t.endswith(":"))
    ok = True
    print("| kernel | VGPRs | SGPRs | LDS bytes | scratch bytes | instructions | against the parent |")
    print("|---|---|---|---|---|---|---|")
    for sym in sorted(names, key=names.get):
        words, body = C.get(sym) or P[sym]
        if sym not in C:
            verdict = "missing"
        elif sym not in P:
            verdict = "new"
        elif P[sym] == C[sym]:
            verdict = "identical"
        else:
            what = [w for w, p, c in zip(WORDS, P[sym][0], words) if p != c]
            if P[sym][1] != body:
                what.append("body (parent: %d instructions)" % count(P[sym][1]))
            verdict = "DIFFERENT: " + ", ".join(what)
        ok &= verdict in ("identical", "new")
        print("| `%s` | %d | %d | %d | %d | %d | %s |" % ((names[sym],) + words + (count(body), verdict)))
    same = sum(1 for s in P if s in C and P[s] == C[s])
    print("\n%d kernels in the parent, %d in the change, %d identical." % (len(P), len(C), same))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
