"""Per-hop kernel times (us) of one `rocprofv3 --kernel-trace --output-format csv -d <dir> -- python3 profiles/weighted_shared.py <workload> <label>`
run, split by state: the dispatches between two k_seed launches are one batch, its k-th k_sample is hop k, and the k_sample instantiation
names the state (<.., true, true, true> = weighted shared-key, <.., true, true, false> = weighted without replacement).  Median [min, max]
over the timed batches of k_sample, k_mark, k_write and the gather.
Usage: python3 profiles/weighted_shared_trace.py <..._kernel_trace.csv> [warm-up batches per state = 3] [states = 2]"""
import csv, re, sys
import numpy as np
path = sys.argv[1]
skip = (int(sys.argv[2]) if len(sys.argv) > 2 else 3) * (int(sys.argv[3]) if len(sys.argv) > 3 else 2)
rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
per, batch, hop, state = {}, -1, 0, None
for r in rows:
    name, us = r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    if "k_seed" in name:
        batch, hop, state = batch + 1, 0, None
        continue
    m = re.search(r"k_(sample|mark|write|gather)", name)
    if batch < skip or not m:
        continue
    if m.group(1) == "sample":
        hop += 1
        state = "weighted_shared" if "true, true, true>" in name else "weighted_distinct" if "true, true, false>" in name else "other"
    per.setdefault((state, 0 if m.group(1) == "gather" else hop, "k_" + m.group(1)), []).append(us)
print("| state | hop | kernel | launches | median us | min | max |\n|---|---|---|---|---|---|---|")
for (state, hop, kernel), v in sorted(per.items(), key=lambda kv: (str(kv[0][0]), kv[0][1] or 9, kv[0][2])):
    print("| %s | %s | %s | %d | %.1f | %.1f | %.1f |" % (state, hop or "all", kernel, len(v), np.median(v), min(v), max(v)))
