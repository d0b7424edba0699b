#!/usr/bin/env python3
"""C3's preamble from a kernel trace: what runs between the signature and the scan.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o TAG -- python bench.py
    python tools/preamble_trace.py OUT/TAG_kernel_trace.csv > profiles/TAG_c3_preamble.txt

Per step (a k_sig_fast dispatch followed by a k_scan_r dispatch): every dispatch from the
signature's end to the scan's start with its start and end relative to the signature's end,
the intervals in which no kernel runs, and the time from the scan's end to the next
signature.  Times in microseconds.  Copies done by the DMA engines are not kernels and show
up here as idle time.
"""
import csv
import re
import sys


def short(name: str) -> str:
    name = re.sub(r"\(.*", "", name).replace("sydelta::", "")
    name = re.sub(r"^void ", "", name)
    return name if len(name) <= 60 else name[:57] + "..."


def main(path: str) -> None:
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"]),
                         r["Queue_Id"]))
    rows.sort()
    sigs = [i for i, r in enumerate(rows) if r[2].startswith("k_sig_fast")]
    steps = []
    for k, i in enumerate(sigs):
        j = next((j for j in range(i + 1, len(rows)) if rows[j][2].startswith("k_scan_r")), None)
        if j is None or (k + 1 < len(sigs) and sigs[k + 1] < j):
            continue
        nxt = rows[sigs[k + 1]][0] if k + 1 < len(sigs) else None
        steps.append((i, j, nxt))
    print(f"# {path.split('/')[-1]}: {len(steps)} steps (warm-up steps included)")
    tot_pre, tot_idle, tot_post = [], [], []
    for n, (i, j, nxt) in enumerate(steps):
        t0 = rows[i][1]
        pre = (rows[j][0] - t0) / 1e3
        print(f"\nstep {n}: k_sig_fast {((rows[i][1] - rows[i][0]) / 1e3):.1f} us; signature end -> scan start {pre:.1f} us; "
              f"k_scan_r {((rows[j][1] - rows[j][0]) / 1e3):.1f} us")
        inside = [r for r in rows if r[0] >= t0 and r[0] < rows[j][0]]
        busy_to = t0
        idle = 0.0
        for s, e, name, q in inside:
            if s > busy_to:
                print(f"    idle {((busy_to - t0) / 1e3):8.1f} .. {((s - t0) / 1e3):8.1f}  ({((s - busy_to) / 1e3):.1f})")
                idle += (s - busy_to) / 1e3
            print(f"  q{q:>2} {((s - t0) / 1e3):8.1f} .. {((e - t0) / 1e3):8.1f}  ({((e - s) / 1e3):6.1f})  {name}")
            busy_to = max(busy_to, e)
        if rows[j][0] > busy_to:
            print(f"    idle {((busy_to - t0) / 1e3):8.1f} .. {pre:8.1f}  ({((rows[j][0] - busy_to) / 1e3):.1f})")
            idle += (rows[j][0] - busy_to) / 1e3
        print(f"  idle inside the stretch: {idle:.1f} us")
        tot_pre.append(pre)
        tot_idle.append(idle)
        if nxt is not None:
            post = (nxt - rows[j][1]) / 1e3
            print(f"  scan end -> next signature start: {post:.1f} us")
            tot_post.append(post)

    def med(v):
        v = sorted(v)
        return v[len(v) // 2] if v else float("nan")

    print(f"\nmedians over {len(steps)} steps: signature end -> scan start {med(tot_pre):.1f} us, idle inside "
          f"{med(tot_idle):.1f} us, scan end -> next signature {med(tot_post):.1f} us")


if __name__ == "__main__":
    main(sys.argv[1])
