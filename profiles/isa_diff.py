#!/usr/bin/env python3
"""Hold the gfx950 code of every kernel of a change against the parent's, kernel by kernel.

    hipcc <the Makefile's CXXFLAGS> --save-temps -c <unit>.hip        (every unit, once on the parent, once on the change)
    python3 profiles/isa_diff.py [--symbols REGEX] [--rename REGEX=REPLACEMENT]... PARENT.s... -- CHANGE.s...

Each side is any number of `*-hip-amdgcn-amd-amdhsa-gfx950.s` files: a kernel may move between units.  For every kernel whose symbol
matches REGEX (default `_ZN6legion`) two things are compared: the kernel descriptor's vgpr_count, sgpr_count, group_segment_fixed_size
(LDS bytes) and private_segment_fixed_size (scratch bytes), and the lines of the function body -- comments, blank lines and directives
dropped, and the local labels `.LBB<n>_<m>` rewritten to `.LBB_<m>`, since <n> is the function's index in its unit.  Text only: the
script knows no instruction.  Prints a markdown table; exit code 1 unless every kernel of the parent is in the change and identical.

A change that renames kernels (other template parameters, another namespace) says so with --rename REGEX=REPLACEMENT, any number of times:
each is a `re.sub` over the PARENT's mangled symbols, applied in the order given before the two sides are matched, so the parent's kernel
is held against the change's kernel of the new name.  The REGEX ends at its first `=`; the REPLACEMENT may use `\\1`.  Bodies are compared
as they are: a kernel that names another kernel's symbol in its body differs under a rename.  Two parent kernels that end up under one name
are an error."""
import argparse
import re
import subprocess
import sys

WORDS = ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")
LOCAL_LABEL = re.compile(r"\.L([A-Za-z_]+)\d+_(\d+)")


def kernels(paths, select, renames=()):
    """symbol -> (the four words, [body lines]) of every selected kernel of the files, under its name after `renames`"""
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
                new = sym
                for pattern, replacement in renames:
                    new = pattern.sub(replacement, new)
                if new in out:
                    sys.exit("%s: kernel %s is in more than one file of this side, or two kernels were renamed to it" % (path, new))
                out[new] = (w, bodies[sym])
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
    ap.add_argument("--rename", action="append", default=[], metavar="REGEX=REPLACEMENT",
                    help="re.sub applied to the parent's symbols before matching; repeatable, applied in order")
    ap.add_argument("files", nargs="+", help="PARENT.s... -- CHANGE.s...")
    argv = sys.argv[1:]
    if "--" not in argv:
        ap.error("the parent's files and the change's are separated by --")
    cut = argv.index("--")
    a = ap.parse_args(argv[:cut])
    select = re.compile(a.symbols)
    if any("=" not in r for r in a.rename):
        ap.error("--rename takes REGEX=REPLACEMENT")
    renames = [(re.compile(r.split("=", 1)[0]), r.split("=", 1)[1]) for r in a.rename]
    P, C = kernels(a.files, select, renames), kernels(argv[cut + 1:], select)
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
