#!/usr/bin/env python3
"""Instructions per env-step, by class, of the step loops of the three-wave rollout kernels.  No GPU needed.

    python profiles/isa_loops.py LISTING.s 'split_rollout_kernelINS_15ChemicalReactorELi3ELi4ELb0E' [more name fragments ...]

LISTING.s is a device listing made with the build's own flags (see profiles/isa_diff.py).  The counting rule:

  * The kernel's instructions form a graph: every instruction leads to the next one, a branch to its label (a conditional
    branch to both).  A LOOP is a label that a later branch jumps back to.
  * For every loop the SHORTEST path from the label round to itself is taken, counted in instructions.  That is the
    iteration with every conditional side path NOT taken -- no spin on a ring counter, no re-read of a slot, no reset, no
    finished episode.  Loops whose shortest iteration has fewer than 30 instructions (the spin loops) are dropped.
  * The ring counters live at the DS offset of the store that zeroes them before the first barrier (+ 0, 4, 8: producer,
    integrator, recorder).  A step posts to its role's counter exactly once, so the number of counter stores on the path is
    the number of env-steps of the iteration, and the counter's index names the role.  Loops that post to no counter (the
    cooperative reset's inner loops) are dropped.
  * A forward s_cbranch_execz whose skipped block holds a counter store (the post's `if (lane == 0)`) is not a side path:
    lane 0 exists, the branch falls through.
  * Classes by mnemonic: s_nop | SALU = every other s_* (waits and branches included) | VALU = v_* | DS = ds_* |
    VMEM = global_* / flat_* / buffer_* / scratch_*.
  * Reported: the iteration's counts divided by its steps.
  * Second row per role, "restart side path": what the shortest path leaves out and a finishing lane pays.  A conditional
    branch ON the shortest path whose other way leads back to the path through a Philox block (v_mad_u64_u32) is a BALLOT
    BRANCH of the cooperative episode restart (coop_reset, csrc/nig_step.hpp); a spin or a slot re-read holds no Philox
    round.  The side path runs from the branch's other way to the first instruction back on the shortest path (the rejoin),
    again by the shortest way, with every forward s_cbranch_execz falling through: the lanes those blocks are for exist
    (a finishing lane, its item lanes), and the item loop runs once.  Where the side path itself forks on a scalar
    condition (one finisher / several), the other way is reported too.  Per way: instructions from the ballot branch to
    the rejoin, the s_waitcnt with an lgkmcnt field inside that span (and how many of them stand behind a ds_read issued since
    the wait before: the dependent LDS round trips; the others step through one batch of reads), the v_mad_u64_u32 inside
    it, the ds_* inside it; min-max over the unrolled copies of the step.
"""
import re
import sys
from collections import deque

ROLES = {0: "producer", 1: "integrator", 2: "recorder"}
CLASSES = ["VALU", "SALU", "DS", "VMEM", "s_nop"]


def kernel_body(lines, frag):
    start = [i for i, l in enumerate(lines) if l.startswith("_ZN3nig") and frag in l and not l.startswith("\t") and ":" in l]
    if not start:
        raise SystemExit(f"no kernel matching {frag}")
    i = j = start[0]
    while not lines[j].startswith(".Lfunc_end"):
        j += 1
    return lines[i].split(":")[0], lines[i + 1:j]


def klass(op):
    if op == "s_nop":
        return "s_nop"
    if op.startswith("s_"):
        return "SALU"
    if op.startswith("v_"):
        return "VALU"
    if op.startswith("ds_"):
        return "DS"
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "VMEM"
    return "other"


def program(body):
    ins, labels = [], {}
    for l in body:
        t = l.split(";")[0].strip()
        if not t:
            continue
        m = re.match(r"^(\.LBB\d+_\d+):", t)
        if m:
            labels[m.group(1)] = len(ins)
        elif l.startswith("\t") and not t.startswith("."):
            ins.append(t)
    succ = []
    for k, t in enumerate(ins):
        op = t.split()[0]
        if op == "s_branch":
            succ.append([labels[t.split()[-1]]])
        elif op.startswith("s_cbranch"):
            succ.append([labels[t.split()[-1]], k + 1])
        elif op == "s_endpgm":
            succ.append([])
        else:
            succ.append([k + 1] if k + 1 < len(ins) else [])
    return ins, succ


def shortest_cycle(succ, h):
    """instructions of the shortest path from h back to h (h included once)"""
    prev, todo = {}, deque()
    for s in succ[h]:
        if s not in prev:
            prev[s] = h
            todo.append(s)
    while todo:
        k = todo.popleft()
        if k == h:
            break
        for s in succ[k]:
            if s not in prev:
                prev[s] = k
                todo.append(s)
    if h not in prev:
        return None
    path, k = [], prev[h]
    while k != h:
        path.append(k)
        k = prev[k]
    path.append(h)
    return path[::-1]


def counter_offset(ins):
    first_barrier = next(k for k, t in enumerate(ins) if t.split()[0] == "s_barrier")
    init = [t for t in ins[:first_barrier] if t.split()[0] == "ds_write_b32"]
    m = re.search(r"offset:(\d+)", init[-1])
    return int(m.group(1)) if m else 0


def keep_posts(ins, succ, off):
    """A post is `if (lane == 0) store`: s_and_saveexec, the store, s_or exec.  When the compiler keeps an s_cbranch_execz
    round the store (it does when a wait lands in that block) the skip is never taken by a whole wave -- lane 0 exists --
    so it is not a side path: the branch falls through."""
    for k, t in enumerate(ins):
        if t.split()[0] == "s_cbranch_execz" and len(succ[k]) == 2 and succ[k][0] > k:
            for u in ins[k + 1:succ[k][0]]:
                m = re.search(r"offset:(\d+)", u)
                if u.split()[0] == "ds_write_b32" and m and int(m.group(1)) - off in (0, 4, 8):
                    succ[k] = [k + 1]
                    break


def report(path, frag):
    lines = open(path).read().split("\n")
    name, body = kernel_body(lines, frag)
    ins, succ = program(body)
    off = counter_offset(ins)
    keep_posts(ins, succ, off)
    print(f"{name}\n  {len(ins)} instructions in the kernel; ring counters at DS offset {off}")
    headers = sorted({t for k, ss in enumerate(succ) for t in ss if t <= k})
    for h in headers:
        cyc = shortest_cycle(succ, h)
        if cyc is None or len(cyc) < 30:
            continue
        posts = []
        for k in cyc:
            t = ins[k]
            m = re.search(r"offset:(\d+)", t)
            if t.split()[0] == "ds_write_b32" and m and int(m.group(1)) - off in (0, 4, 8):
                posts.append((int(m.group(1)) - off) // 4)
        if not posts or len(set(posts)) != 1:
            continue
        steps = len(posts)
        n = {c: 0 for c in CLASSES + ["other"]}
        for k in cyc:
            n[klass(ins[k].split()[0])] += 1
        per = "  ".join(f"{c} {n[c] / steps:6.1f}" for c in CLASSES)
        print(f"  {ROLES[posts[0]]:10s} {steps:2d} steps per iteration, {len(cyc):4d} instructions: per step {len(cyc) / steps:6.1f} = {per}"
              + (f"  other {n['other'] / steps:.1f}" if n["other"] else ""))


def side_path(ins, succ_ft, start, on_cycle):
    """shortest way from `start` to the first instruction on the loop's shortest path (exclusive); None if there is none"""
    if start in on_cycle:
        return []
    prev, todo, end = {start: None}, deque([start]), None
    while todo:
        k = todo.popleft()
        if k in on_cycle:
            end = k
            break
        for t in succ_ft[k]:
            if t not in prev:
                prev[t] = k
                todo.append(t)
    if end is None:
        return None
    path, k = [], prev[end]
    while k is not None:
        path.append(k)
        k = prev[k]
    return path[::-1]


def restart_rows(ins, succ, cyc):
    """[(label, [(instructions, lgkm waits, v_mad_u64_u32, ds), ...] per unrolled copy)] for the loop whose shortest path is cyc"""
    on_cycle = set(cyc)
    succ_ft = [([k + 1] if ins[k].split()[0] == "s_cbranch_execz" and len(ss) == 2 and ss[0] > k else ss) for k, ss in enumerate(succ)]

    def measure(path):
        ops = [ins[k].split()[0] for k in path]
        trips, fresh = 0, False          # waits with a ds_read issued since the wait before: dependent LDS round trips
        for k in path:
            if ins[k].split()[0].startswith("ds_read"):
                fresh = True
            elif ins[k].startswith("s_waitcnt") and "lgkmcnt" in ins[k] and fresh:
                trips, fresh = trips + 1, False
        return (len(path), sum(1 for k in path if ins[k].startswith("s_waitcnt") and "lgkmcnt" in ins[k]),
                ops.count("v_mad_u64_u32"), sum(1 for o in ops if o.startswith("ds_")), trips)

    first, other = [], []
    for k in cyc:
        if not ins[k].split()[0].startswith("s_cbranch") or len(succ[k]) != 2:
            continue
        for t in succ[k]:
            if t in on_cycle:
                continue
            path = side_path(ins, succ_ft, t, on_cycle)
            if not path or not any(ins[j].split()[0] == "v_mad_u64_u32" for j in path):
                continue
            first.append(measure(path))
            # a scalar fork inside the side path: the way not taken, if it is a restart as well
            for j in path:
                if ins[j].split()[0] in ("s_cbranch_scc0", "s_cbranch_scc1", "s_cbranch_vccz", "s_cbranch_vccnz") and len(succ_ft[j]) == 2:
                    alt = [u for u in succ_ft[j] if u not in path and u not in on_cycle]
                    for u in alt:
                        rest = side_path(ins, succ_ft, u, on_cycle)
                        if rest and any(ins[x].split()[0] == "v_mad_u64_u32" for x in rest):
                            other.append(measure(path[:path.index(j) + 1] + rest))
                    break
    rows = []
    if first:
        rows.append(("shortest way" if other else "only way", first))
    if other:
        rows.append(("other way of its first scalar fork", other))
    return rows


def report_restart(path, frag):
    lines = open(path).read().split("\n")
    name, body = kernel_body(lines, frag)
    ins, succ = program(body)
    off = counter_offset(ins)
    keep_posts(ins, succ, off)
    for h in sorted({t for k, ss in enumerate(succ) for t in ss if t <= k}):
        cyc = shortest_cycle(succ, h)
        if cyc is None or len(cyc) < 30:
            continue
        posts = [(int(re.search(r"offset:(\d+)", ins[k]).group(1)) - off) // 4 for k in cyc
                 if ins[k].split()[0] == "ds_write_b32" and re.search(r"offset:(\d+)", ins[k]) and int(re.search(r"offset:(\d+)", ins[k]).group(1)) - off in (0, 4, 8)]
        if not posts or len(set(posts)) != 1:
            continue
        for label, ms in restart_rows(ins, succ, cyc):
            rng = lambda i: ("%d" % min(m[i] for m in ms)) if min(m[i] for m in ms) == max(m[i] for m in ms) else "%d-%d" % (min(m[i] for m in ms), max(m[i] for m in ms))   # noqa: E731
            print(f"  {ROLES[posts[0]]:10s} restart side path, {label}: {len(ms)} copies; ballot branch to rejoin {rng(0)} instructions, "
                  f"s_waitcnt lgkmcnt {rng(1)} ({rng(4)} behind a fresh ds_read: dependent LDS round trips), v_mad_u64_u32 {rng(2)}, ds_* {rng(3)}")


if __name__ == "__main__":
    for frag in sys.argv[2:]:
        report(sys.argv[1], frag)
        report_restart(sys.argv[1], frag)
