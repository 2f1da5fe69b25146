#!/usr/bin/env python3
"""Scratch (private memory) instructions per loop of a kernel's gfx950 assembly.

    hipcc ... -save-temps=obj -c geom_kernels.hip -o /tmp/geom.o
    tools/scratch_per_loop.py /tmp/geom_kernels-hip-amdgcn-amd-amdhsa-gfx950.s k_ransac k_five_point_raw

A loop is a backward branch to a label of the same function; nested loops are listed on their own and inside their
parents.  Per loop: instructions, vector scratch loads / stores, LDS instructions and f64 instructions in its body."""
import re
import sys

INST = re.compile(r"^\s+([a-z]\w+)\s")
LABEL = re.compile(r"^(\.LBB\d+_\d+):")
BRANCH = re.compile(r"\s(s_cbranch\w+|s_branch)\s+(\.LBB\d+_\d+)")
SCRATCH = re.compile(r"^\s+scratch_(load|store)")


def functions(lines):
    out, name = {}, None
    for l in lines:
        m = re.match(r"^(_Z\w+):", l)
        if m:
            name = m.group(1); out[name] = []
        elif name and l.startswith(".Lfunc_end"):
            name = None
        if name:
            out[name].append(l)
    return out


def report(name, body):
    labels = {LABEL.match(l).group(1): k for k, l in enumerate(body) if LABEL.match(l)}
    loops = []
    for k, l in enumerate(body):
        m = BRANCH.search(l)
        if m and labels.get(m.group(2), k + 1) <= k:
            loops.append((labels[m.group(2)], k, m.group(2)))
    sc = [SCRATCH.match(l).group(1) for l in body if SCRATCH.match(l)]
    print(f"{name}: {sum(bool(INST.match(l)) for l in body)} instructions, scratch loads {sc.count('load')} stores {sc.count('store')}, {len(loops)} loops")
    for a, b, lab in sorted(loops):
        part = body[a:b + 1]
        ops = [INST.match(l).group(1) for l in part if INST.match(l)]
        s = [SCRATCH.match(l).group(1) for l in part if SCRATCH.match(l)]
        print(f"  loop {lab:<12} lines {a:>6}-{b:<6} instructions {len(ops):>5}  scratch loads {s.count('load'):>3} stores {s.count('store'):>3}"
              f"  lds {sum(o.startswith('ds_') for o in ops):>3}  f64 {sum('_f64' in o for o in ops):>5}  dpp {sum('dpp' in l for l in part):>4}")


def main():
    path, wanted = sys.argv[1], sys.argv[2:]
    fns = functions(open(path).read().split("\n"))
    for name, body in fns.items():
        if not wanted or any(w in name for w in wanted):
            report(name, body)


if __name__ == "__main__":
    main()
