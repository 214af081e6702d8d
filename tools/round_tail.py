#!/usr/bin/env python
"""The device window between two planning rounds, from a rocprofv3 rocpd sqlite database (kernel trace only, no counters):
for every round after the first, the time from the end of the last step kernel of the round before (unet_kernel, the
ddpm_* step kernels) to the start of the round's first unet_kernel, and the kernels dispatched in that window.  A round
is recognised by its init_kernel launch.
    rocprofv3 --kernel-trace -d DIR -o bench -- python bench.py --steps 5 --warmup 2
    python tools/round_tail.py DIR/bench_results.db [rounds to skip at the front] > profiles/round_tail_<tag>.txt"""
import bisect
import re
import sqlite3
import sys
from collections import Counter

STEP = re.compile(r"unet_kernel|unet_persist_kernel|ddpm_")


def short(name):
    name = re.sub(r"\(.*", "", name)
    name = re.sub(r"^void ", "", name)
    return name[:100]


def main(path, skip=0):
    c = sqlite3.connect(path)
    cols = [r[1] for r in c.execute("pragma table_info(kernels)")]
    name_col = "name" if "name" in cols else "kernel_name"
    rows = sorted(((s, e, short(n)) for n, s, e in c.execute(f"select {name_col}, start, end from kernels")), key=lambda r: r[0])
    starts = [r[0] for r in rows]
    inits = [i for i, r in enumerate(rows) if r[2].endswith("init_kernel") and "window" not in r[2]]
    windows = []
    for i in inits:
        before = [r for r in rows[max(0, i - 400):i] if STEP.search(r[2])]
        after = next((r for r in rows[i:i + 400] if "unet_kernel" in r[2]), None)
        if not before or after is None:
            continue                                  # the first round: nothing ran before it
        w0, w1 = max(r[1] for r in before), after[0]
        inside = rows[bisect.bisect_left(starts, w0):bisect.bisect_left(starts, w1)]
        windows.append((w0, w1, inside))
    windows = windows[skip:]
    print(f"# between-round device window ({path}; {len(windows)} rounds, the first {skip} windows skipped)")
    print("# window = end of the last step kernel of round k  ->  start of the first unet_kernel of round k + 1\n")
    print("| round | window us | kernels in it | their busy us |")
    print("|---:|---:|---:|---:|")
    tot, names = 0.0, Counter()
    for k, (w0, w1, inside) in enumerate(windows):
        busy = sum(r[1] - r[0] for r in inside)
        tot += w1 - w0
        names.update(r[2] for r in inside)
        print(f"| {k + skip + 1} | {(w1 - w0) / 1e3:.1f} | {len(inside)} | {busy / 1e3:.1f} |")
    if windows:
        print(f"\nmean window {tot / len(windows) / 1e3:.1f} us over {len(windows)} rounds\n")
        print("kernels dispatched inside the windows (dispatches per round):\n")
        for n, cnt in sorted(names.items(), key=lambda kv: -kv[1]):
            print(f"- {cnt / len(windows):.2f} x `{n}`")


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 0)
