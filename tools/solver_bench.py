#!/usr/bin/env python
"""What does the Connect Four solver (csrc/solver.hip, az_c4_solve) reach, and what does it cost, on the six Pons benchmark sets?

Per set (1000 positions, up to 7000 (state, action) queries) and per mode (strong = exact scores, weak = their sign), at the default
node budget or --budget: queries, share of queries solved, share of positions whose value is known, wall time of the call after a
warm-up (median of --reps) and nodes/s.  For comparison the CPU negamax of the test suite (azref.c4_solve, one core, 2 M nodes per
query) runs over the queries of the first --cpu-positions positions of each set: share solved, nodes/s.

    python tools/solver_bench.py [--dir tests/golden/pons] [--budget N] [--reps 3] [--cpu-positions 32] [--out profiles/solver/solver_sets.json]
                                 [--table-bits N] [--sets beginning/easy,middle/medium] [--modes strong,weak]

--table-bits N > 0: the same sets through az_c4_solve_table with one table of 2^N entries (0, the default, is the tableless run
above).  Per set and mode the table is cleared and the call is made twice: "cold" and, on what the first call left in the table,
"warm"; each row carries the shares, the wall time of that one call, nodes/s and the table's occupied entries after it.  A call
changes the table, so there are no repetitions and no CPU leg; --out defaults to profiles/solver/solver_sets_table.json.

Prints one JSON line per measurement and writes all of them to --out.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "alphazero.jl_amd"))
import numpy as np  # noqa: E402

import azhip  # noqa: E402
from azhip import Pons, Solver  # noqa: E402
from azhip import _lib as L  # noqa: E402


def cpu_leg(bench, npos, limit):
    """the test suite's CPU negamax over the same queries: the children of the first npos positions that do not end the game"""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import azref as R
    queries = solved = nodes = 0
    t0 = time.perf_counter()
    for s, _ in bench.entries[:npos]:
        g = R.Game(R.C4)
        for c in s:
            g.play(int(c) - 1)
        for a in g.available_actions():
            c = g.clone()
            c.play(a)
            if c.terminated():
                continue
            sc, n = R.c4_solve([int(x) - 1 for x in s] + [int(a)], limit)
            queries, solved, nodes = queries + 1, solved + (sc < 98), nodes + min(n, limit)
    sec = time.perf_counter() - t0
    return {"positions": min(npos, len(bench.entries)), "queries": queries, "solved_share": round(solved / max(queries, 1), 4),
            "node_limit": limit, "seconds": round(sec, 3), "nodes_per_s": round(nodes / max(sec, 1e-9))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", default=os.path.join(ROOT, "tests", "golden", "pons"))
    ap.add_argument("--budget", type=int, default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cpu-positions", type=int, default=32)
    ap.add_argument("--cpu-limit", type=int, default=2_000_000)
    ap.add_argument("--table-bits", type=int, default=0)
    ap.add_argument("--sets", default=None, help="stage/difficulty pairs, comma separated; default: all")
    ap.add_argument("--modes", default="strong,weak")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, "profiles", "solver", "solver_sets_table.json" if a.table_bits > 0 else "solver_sets.json")
    only = None if a.sets is None else {tuple(x.split("/")) for x in a.sets.split(",")}
    modes = [m == "weak" for m in a.modes.split(",")]
    table = Solver.Table(a.table_bits) if a.table_bits > 0 else None
    gspec = azhip.ConnectFourSpec()
    e = gspec._eng()
    budget = a.budget or L.SOLVER_DEFAULT_BUDGET
    rows = []
    for b in Pons.load_benchmarks(a.dir):
        if only is not None and (b.stage, b.difficulty) not in only:
            continue
        keys = Pons.states_of_strings([s for s, _ in b.entries], gspec)
        for weak in modes:
            e.c4_solve(keys[:16], weak=weak, node_budget=16, table=table)         # warm-up: code object, staging buffers
            if table is not None:
                table.clear()
                for state in ("cold", "warm"):
                    t0 = time.perf_counter()
                    value, q, nodes = e.c4_solve(keys, weak=weak, node_budget=budget, table=table)
                    sec = time.perf_counter() - t0
                    nq = int((q != Solver.NA).sum())
                    for (s, sc), v in zip(b.entries, value):                      # a solved value is the recorded one
                        assert v == Solver.UNSOLVED or int(v) == (int(np.sign(sc)) if weak else sc), (s, int(v), sc)
                    row = {"what": "az_c4_solve_table", "table_bits": a.table_bits, "table": state, "stage": b.stage, "difficulty": b.difficulty,
                           "mode": "weak" if weak else "strong", "node_budget": budget, "positions": len(b.entries), "queries": nq,
                           "queries_solved_share": round(float((q != Solver.UNSOLVED).sum() - (q == Solver.NA).sum()) / nq, 4),
                           "values_solved_share": round(float((value != Solver.UNSOLVED).mean()), 4),
                           "values_unknown": int((value == Solver.UNSOLVED).sum()), "wall_s": round(sec, 4), "nodes": int(nodes.sum()),
                           "nodes_per_s": round(int(nodes.sum()) / sec), "occupied": table.info()["occupied"]}
                    rows.append(row)
                    print(json.dumps(row), flush=True)
                continue
            secs = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                value, q, nodes = e.c4_solve(keys, weak=weak, node_budget=budget)
                secs.append(time.perf_counter() - t0)
            sec = sorted(secs)[len(secs) // 2]
            nq = int((q != Solver.NA).sum())
            for (s, sc), v in zip(b.entries, value):                              # a solved value is the recorded one
                assert v == Solver.UNSOLVED or int(v) == (int(np.sign(sc)) if weak else sc), (s, int(v), sc)
            row = {"what": "az_c4_solve", "stage": b.stage, "difficulty": b.difficulty, "mode": "weak" if weak else "strong",
                   "node_budget": budget, "positions": len(b.entries), "queries": nq,
                   "queries_solved_share": round(float((q != Solver.UNSOLVED).sum() - (q == Solver.NA).sum()) / nq, 4),
                   "values_solved_share": round(float((value != Solver.UNSOLVED).mean()), 4), "reps": a.reps,
                   "wall_s_median": round(sec, 4), "wall_s_min": round(min(secs), 4), "nodes": int(nodes.sum()),
                   "nodes_per_s": round(int(nodes.sum()) / sec)}
            rows.append(row)
            print(json.dumps(row), flush=True)
        if a.cpu_positions > 0 and table is None:
            row = dict({"what": "cpu negamax, one core", "stage": b.stage, "difficulty": b.difficulty}, **cpu_leg(b, a.cpu_positions, a.cpu_limit))
            rows.append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"device": e.device_info()[0], "rows": rows}, f, indent=1)
        f.write("\n")
    if table is not None:
        table.close()


if __name__ == "__main__":
    main()
