#!/usr/bin/env python3
"""Hold the gfx950 resources and instruction counts of the k_sample instantiations that existed before the WEIGHTED template parameter
against the same instantiations after it, and list the new ones.

    hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 --save-temps -c kernels.hip      (once on the parent, once on the change)
    python3 profiles/sample_weighted_isa.py <parent>/kernels-hip-amdgcn-amd-amdhsa-gfx950.s <change>/kernels-hip-amdgcn-amd-amdhsa-gfx950.s

A parent k_sample<TILE, PRESC, PART, DISTINCT> is the change's k_sample<TILE, PRESC, PART, DISTINCT, false>.  Compared per instantiation:
VGPRs, SGPRs, LDS bytes, scratch bytes (the kernel descriptor's words) and the number of instructions (lines of the function body that are
neither labels, directives nor comments).  Prints a markdown table; exit code 1 when an existing instantiation differs."""
import re
import sys

SYM = r"_ZN6legion8k_sampleILi(\d+)ELb([01])ELb([01])ELb([01])E(?:Lb([01])E)?EEvNS_10SampleArgsE"
WORDS = ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")


def instruction_counts(path):
    out, name, n = {}, None, 0
    for line in open(path):
        m = re.match("^(" + SYM + "):", line)
        if m:
            name, n = m.group(1), 0
            continue
        if name is not None:
            if line.startswith(".Lfunc_end") or line.startswith("\t.section"):
                out[name], name = n, None
                continue
            text = re.sub(r";.*", "", line).strip()
            if text and not text.endswith(":") and not text.startswith("."):
                n += 1
    return out


def resources(path):
    res, block = {}, {}
    for line in open(path):
        m = re.match(r"\s+\.(name|%s):\s+(\S+)" % "|".join(WORDS), line)
        if m:
            block[m.group(1)] = m.group(2)
        if line.strip().startswith(".wavefront_size"):
            if re.match(SYM + "$", block.get("name", "")):
                res[block["name"]] = tuple(int(block[w]) for w in WORDS)
            block = {}
    return res


def key(name):
    tile, presc, part, distinct, weighted = re.match(SYM, name).groups()
    return (int(tile), int(presc), int(part), int(distinct), int(weighted or 0))


def main(parent, change):
    P = {key(n): r + (instruction_counts(parent)[n],) for n, r in resources(parent).items()}
    C = {key(n): r + (instruction_counts(change)[n],) for n, r in resources(change).items()}
    same = True
    print("| k_sample<TILE, PRESC, PART, DISTINCT, WEIGHTED> | VGPRs | SGPRs | LDS bytes | scratch bytes | instructions | against the parent |")
    print("|---|---|---|---|---|---|---|")
    for k in sorted(C):
        verdict = "new"
        if k in P:
            verdict = "identical" if P[k] == C[k] else "DIFFERENT: parent %s" % (P[k],)
            same &= P[k] == C[k]
        print("| <%d, %d, %d, %d, %d> | %d | %d | %d | %d | %d | %s |" % (k + C[k] + (verdict,)))
    missing = sorted(set(P) - set(C))
    if missing:
        same = False
        print("missing from the change:", missing)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3]))
