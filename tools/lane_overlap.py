"""Do consecutive launches of the run-to-completion kernel overlap?  Reads the kernel trace of a profiled run
(`rocprofv3 --kernel-trace --stats --output-format csv -- python bench.py --solve-only --steps 20`, the `*_kernel_trace.csv` it writes) and prints, for
the last launches of the solve kernel, the hardware queue of each launch and the start of launch k + 1 relative to the end of launch k (negative: it
started while its predecessor was still running -- the two lanes of a handle are on different hardware queues and share the chip).

    python tools/lane_overlap.py <kernel_trace.csv> [kernel name substring = lm_pass_kernel] [launches = 12]
"""
import csv
import sys


def main():
    path = sys.argv[1]
    name = sys.argv[2] if len(sys.argv) > 2 else "lm_pass_kernel"
    last = int(sys.argv[3]) if len(sys.argv) > 3 else 12
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            if name in r["Kernel_Name"]:
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r.get("Queue_Id", "?"), r.get("Stream_Id", "?")))
    rows.sort()
    print(f"{len(rows)} launches of *{name}*; the last {min(last, len(rows))}:")
    print("launch  queue  stream  duration_us  start - previous end [us]  busy with predecessor [us]")
    tail = rows[-last:]
    for i, (s, e, q, st) in enumerate(tail):
        if i == 0:
            print(f"{len(rows) - len(tail) + i:6d}  {q:>5}  {st:>6}  {(e - s) / 1e3:11.1f}")
            continue
        pe = tail[i - 1][1]
        print(f"{len(rows) - len(tail) + i:6d}  {q:>5}  {st:>6}  {(e - s) / 1e3:11.1f}  {(s - pe) / 1e3:25.1f}  {max(0, min(e, pe) - s) / 1e3:25.1f}")
    if len(tail) > 1:
        span = tail[-1][1] - tail[0][0]
        print(f"span of these launches {span / 1e3:.1f} us = {span / 1e3 / len(tail):.1f} us per launch; sum of their durations {sum(e - s for s, e, _, _ in tail) / 1e3:.1f} us")


if __name__ == "__main__":
    main()
