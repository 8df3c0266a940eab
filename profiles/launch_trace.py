#!/usr/bin/env python3
"""kernel_trace.csv of `rocprofv3 --kernel-trace` -> the ORDERED list of the library's launches, in a form short enough to keep:

    python profiles/launch_trace.py <kernel_trace.csv> <out.txt>

First a table `k<i> <workgroup size> <kernel>` (parameter lists and the nig:: prefix dropped), then the launches in start order as
`k<i>@<grid size in threads>` tokens, a new line at every handle creation (init_ws_kernel).  Prints the number of launches and the
sha256 of the one-launch-per-line form.  Two such files are equal exactly when the two ordered launch lists are."""
import csv
import hashlib
import re
import sys


def main(trace, out):
    rows = list(csv.DictReader(open(trace)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    ids, lines, h, n = {}, [], hashlib.sha256(), 0
    for r in rows:
        name = r["Kernel_Name"]
        if "nig::" not in name and "mixed_rollout_kernel" not in name:
            continue
        name = re.sub(r"\((nig::|unsigned|float|long|int|double).*\)$", "", re.sub(r"^void ", "", name)).replace("nig::", "")
        grid, wg = r["Grid_Size_X"], r["Workgroup_Size_X"]
        h.update(f"{name}\t{grid}\t{wg}\n".encode())
        n += 1
        k = ids.setdefault((name, wg), len(ids))
        if name == "init_ws_kernel" or not lines:
            lines.append([])
        lines[-1].append(f"k{k}@{grid}")
    with open(out, "w") as f:
        for (name, wg), k in ids.items():
            f.write(f"k{k} {wg} {name}\n")
        f.write("\n")
        for l in lines:
            f.write(" ".join(l) + "\n")
    print(n, "launches,", len(ids), "kernels, sha256", h.hexdigest())


if __name__ == "__main__":
    main(*sys.argv[1:3])
