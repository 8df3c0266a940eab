#!/usr/bin/env python3
"""Do two builds hold the same instructions in the kernels they share?  No GPU needed.

    python profiles/isa_diff.py OLD_DIR NEW_DIR

OLD_DIR / NEW_DIR hold one device listing per translation unit (<tu>.s), made with the build's own flags:

    hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fno-slp-vectorize -std=c++17 -w -S --cuda-device-only \
          -Rpass-analysis=kernel-resource-usage -o DIR/<tu>.s csrc/<tu>.hip 2> DIR/<tu>.remarks

Every function symbol of OLD is looked up in NEW and the two bodies are compared instruction by instruction (comments,
directives and blank lines dropped; basic-block labels renumbered, because their numbers count the functions of the file).
Prints the symbols that differ or vanished, the symbols only NEW has, and exits 1 if a shared symbol differs.  With
--resources also prints VGPRs / scratch / occupancy of NEW's kernels whose name contains "sampled" next to their ring-fed
twins, from the .remarks files.
"""
import glob
import os
import re
import sys


def functions(path):
    """symbol -> list of normalised instruction lines"""
    out, name, body = {}, None, []
    for l in open(path):
        if name is None:
            m = re.match(r"^(_Z\w+|[A-Za-z_]\w*):\s*(;.*)?$", l)
            if m and not l.startswith(".L"):
                name, body = m.group(1), []
            continue
        if l.startswith(".Lfunc_end"):
            out[name] = body
            name = None
            continue
        t = l.split(";")[0].rstrip()
        if not t.strip():
            continue
        t = re.sub(r"\.LBB\d+_", ".LBB_", t)
        if t.startswith("\t."):             # directive
            continue
        body.append(t.strip())
    return out


def resources(path):
    """kernel name -> {VGPRs, ScratchSize, Occupancy, ...} from -Rpass-analysis=kernel-resource-usage remarks"""
    out, cur = {}, None
    for l in open(path):
        m = re.search(r"remark: .*Function Name: (\S+)", l)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+(\w[\w ]*?)(?: \[[^\]]*\])?: (\d+) \[", l)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return out


def main(argv):
    want_res = "--resources" in argv
    dirs = [a for a in argv if not a.startswith("--")]
    old_dir, new_dir = dirs
    bad = 0
    n_same = 0
    for old_s in sorted(glob.glob(os.path.join(old_dir, "*.s"))):
        tu = os.path.basename(old_s)
        new_s = os.path.join(new_dir, tu)
        if not os.path.exists(new_s):
            print(f"{tu}: missing in {new_dir}")
            bad += 1
            continue
        fo, fn = functions(old_s), functions(new_s)
        for sym, body in fo.items():
            if sym not in fn:
                print(f"{tu}: {sym} vanished")
                bad += 1
            elif fn[sym] != body:
                k = next((i for i, (a, b) in enumerate(zip(body, fn[sym])) if a != b), min(len(body), len(fn[sym])))
                print(f"{tu}: {sym} DIFFERS ({len(body)} -> {len(fn[sym])} instructions, first at #{k})")
                bad += 1
            else:
                n_same += 1
        added = sorted(set(fn) - set(fo))
        print(f"{tu}: {len(fo)} shared symbols compared, {len(added)} new")
    print(f"identical: {n_same}, differing or missing: {bad}")
    if want_res:
        import subprocess
        by_dem = {}
        for rem in sorted(glob.glob(os.path.join(new_dir, "*.remarks"))):      # (the twins live in different translation units)
            res = resources(rem)
            names = list(res)
            dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
            by_dem.update({re.sub(r"\(.*$", "", d).replace("void ", ""): res[n] for n, d in zip(names, dem)})
        if True:
            for d, r in sorted(by_dem.items()):
                if "sampled" not in d:
                    continue
                m = re.match(r"nig::(\w+)<(.*)>$", d)
                a = [x.strip() for x in m.group(2).split(",")]
                twin = {"rollout_sampled_kernel": lambda: "rollout_kernel<%s, false>" % ", ".join(a),
                        "rollout_sampled_wide_kernel": lambda: "rollout_wide_kernel<%s, false>" % ", ".join(a),
                        "split_sampled_kernel": lambda: "split_rollout_kernel<%s, false>" % ", ".join(a),
                        "pg_pair_sampled_kernel": lambda: "rollout_pg_pair_kernel<%s, false, %s>" % (a[0], a[1])}[m.group(1)]()
                t = by_dem.get("nig::" + twin, {})
                fmt = lambda q: f"VGPRs {q.get('VGPRs')} scratch {q.get('ScratchSize')} B occupancy {q.get('Occupancy')}"
                print(f"{d[5:]:62s} {fmt(r):44s} | ring-fed twin: {fmt(t)}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
