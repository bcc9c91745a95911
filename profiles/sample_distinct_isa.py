#!/usr/bin/env python3
"""Compare the gfx950 ISA of the default-mode k_sample instantiations before and after the DISTINCT template parameter.

    hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 --save-temps -c kernels.hip      (once on the parent, once on the change)
    python3 profiles/sample_distinct_isa.py <parent>/kernels-hip-amdgcn-amd-amdhsa-gfx950.s <change>/kernels-hip-amdgcn-amd-amdhsa-gfx950.s

A parent instantiation k_sample<TILE, PRESC, PART> is held against the change's k_sample<TILE, PRESC, PART, false>: the instruction
streams with the symbol name, the block-label numbers and the comments taken out.  Prints one line per instantiation and the kernel
descriptors' resource words of every instantiation of the change."""
import difflib
import re
import sys

SYM = r"_ZN6legion8k_sampleILi(\d+)ELb([01])ELb([01])E(?:Lb([01])E)?EEvNS_10SampleArgsE"


def functions(path):
    out, name, cur = {}, None, None
    for line in open(path):
        m = re.match("^(" + SYM + "):", line)
        if m:
            name, cur = m.group(1), []
            continue
        if name is not None:
            if line.startswith(".Lfunc_end") or line.startswith("\t.section"):
                out[name], name = cur, None
            else:
                cur.append(line)
    return out


def resources(path):
    res, block = {}, {}
    for line in open(path):
        m = re.match(r"\s+\.(name|vgpr_count|sgpr_count|group_segment_fixed_size|private_segment_fixed_size):\s+(\S+)", line)
        if m:
            block[m.group(1)] = m.group(2)
        if line.strip().startswith(".wavefront_size"):
            if re.match(SYM + "$", block.get("name", "")):
                res[block["name"]] = dict(block)
            block = {}
    return res


def normalised(lines):
    body = "".join(lines)
    body = re.sub(SYM, "K_SAMPLE", body)
    body = re.sub(r"\.LBB\d+_", ".LBB_", body)
    return [l.rstrip() for l in re.sub(r";.*", "", body).splitlines() if l.strip()]


def main(parent, change):
    P, B = functions(parent), functions(change)
    same = True
    for name in sorted(P):
        tile, presc, part, _ = re.match(SYM, name).groups()
        twin = "_ZN6legion8k_sampleILi%sELb%sELb%sELb0EEEvNS_10SampleArgsE" % (tile, presc, part)
        a, b = normalised(P[name]), normalised(B[twin])
        print("k_sample<%s, %s, %s> -> <.., false>: %d instructions and labels, %s" % (tile, presc, part, len(a), "identical" if a == b else "DIFFERENT"))
        if a != b:
            same = False
            print("\n".join(list(difflib.unified_diff(a, b, lineterm="", n=1))[:80]))
    for name, r in sorted(resources(change).items()):
        tile, presc, part, distinct = re.match(SYM, name).groups()
        print("k_sample<%s, %s, %s, %s>: %s VGPRs, %s SGPRs, %s bytes LDS, %s bytes scratch" % (tile, presc, part, distinct, r["vgpr_count"], r["sgpr_count"], r["group_segment_fixed_size"], r["private_segment_fixed_size"]))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3]))
