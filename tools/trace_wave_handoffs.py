#!/usr/bin/env python
"""The hand-offs of a free-running wave in a rocprofv3 --kernel-trace CSV of the headline (one slot group).

A wave is, on ONE queue: k_tree (the wave's launch), the tower, the heads; the move step and the background search (a second k_tree)
run on other queues under the tower, and the next wave's launch waits for them.  Over the LAST n tower dispatches of the process
(with `bench.py --gpus 1 --steps n` nothing is launched after the timed region but the step's epilogue):

    tower_end_to_wave_launch_us   tower end -> start of the next k_tree on the tower's queue (heads + every join in between)
    heads_end_to_wave_launch_us   heads end -> that start (the joins alone)
    wave_launch_us                duration of that k_tree
    tower_us                      duration of the tower
    background_end_to_tower_end_us  tower end - end of the background k_tree (another queue) that ran under it: > 0 = the search left early
    launches_per_wave             dispatches of the window on all queues / towers in it, and the count per kernel

    tools/trace_wave_handoffs.py <kernel_trace.csv> <n> [rows_out.csv]  ->  one JSON line (rows_out: the window's dispatches)
"""
import csv
import json
import statistics
import sys


def main():
    path, n = sys.argv[1], int(sys.argv[2])
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Queue_Id"], r["Kernel_Name"].replace("void ", "").split("<")[0].split("(")[0]))
    rows.sort()
    towers = [i for i, r in enumerate(rows) if r[3].startswith("k_tower")]
    win = towers[-n:]
    gaps, hgaps, launch, tower, bgend = [], [], [], [], []
    for i in win:
        s, e, q, _ = rows[i]
        tower.append((e - s) / 1e3)
        for r in rows[max(i - 4, 0):i + 5]:
            if r[2] != q and r[3] == "k_tree" and r[0] < e and r[1] > s:
                bgend.append((e - r[1]) / 1e3)
                break
        heads_end = None
        for r in rows[i + 1:i + 40]:
            if r[2] != q:
                continue
            if r[3].startswith("k_heads"):
                heads_end = r[1]
            if r[3] == "k_tree":
                gaps.append((r[0] - e) / 1e3)
                launch.append((r[1] - r[0]) / 1e3)
                if heads_end is not None:
                    hgaps.append((r[0] - heads_end) / 1e3)
                break
    lo, hi = rows[win[0]][0], rows[win[-1]][1]
    inside = [r for r in rows if lo <= r[0] <= hi]
    per = {}
    for r in inside:
        per[r[3]] = per.get(r[3], 0) + 1

    def st(v):
        return {"median": round(statistics.median(v), 2), "mean": round(sum(v) / len(v), 2), "p10": round(sorted(v)[len(v) // 10], 2),
                "p90": round(sorted(v)[len(v) * 9 // 10], 2)} if v else None
    print(json.dumps({"trace": path.split("/")[-1], "towers": len(win), "window_ms": round((hi - lo) / 1e6, 3),
                      "ms_per_wave": round((hi - lo) / 1e6 / max(len(win) - 1, 1), 4),
                      "tower_end_to_wave_launch_us": st(gaps), "heads_end_to_wave_launch_us": st(hgaps), "wave_launch_us": st(launch), "tower_us": st(tower),
                      "background_end_to_tower_end_us": st(bgend),
                      "launches_per_wave": round(len(inside) / len(win), 2), "launches_per_wave_by_kernel": {k: round(v / len(win), 2) for k, v in sorted(per.items())}}))
    if len(sys.argv) > 3:
        with open(sys.argv[3], "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(["start_us", "end_us", "queue", "kernel"])
            for r in inside:
                w.writerow([round((r[0] - lo) / 1e3, 2), round((r[1] - lo) / 1e3, 2), r[2], r[3]])


if __name__ == "__main__":
    main()
