#!/usr/bin/env python
"""The Pons benchmark (games/connect-four/scripts/pons_benchmark.jl) on the device: the error rate of the MinMax baseline (depth 5,
amplified rewards, tau = 0), of the network alone and of the MCTS player on the six sets, judged by the device solver in weak mode.

Which network: --params FILE (a parameter file written by azhip.network.save_params), or by default the untrained network and
the best network after each of --iters iterations of examples/iteration.py's training loop (the learning curve of the
reference's documentation, in miniature).  Positions the solver cannot judge within its node budget are left out and counted.

    python tools/pons_benchmark.py [--dir tests/golden/pons] [--params FILE] [--iters 3] [--games 256] [--sims 100] [--workers 128]
                                   [--budget N] [--out profiles/solver/pons_benchmark.json] [--table-bits N] [--players minmax,network_only]

--table-bits N > 0: the solver judges with one transposition table of 2^N entries (azhip.Solver.Table) that serves all six sets
and every player of the run; --out defaults to profiles/solver/pons_benchmark_table.json then, and beside each row's `unsolved`
(the positions left out) stands `unsolved_tableless`, the same figure of the tableless run in profiles/solver/pons_benchmark.json.
--players: which kinds of player to test (default: minmax, network_only and alphazero).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "alphazero.jl_amd"))
import azhip  # noqa: E402
from azhip import MinMax, Pons  # noqa: E402
from azhip.network import load_params  # noqa: E402
from azhip.training import SelfPlayParams, train_iteration  # noqa: E402


def rows_of(res):
    return [{"stage": r["stage"], "difficulty": r["difficulty"], "error_rate": None if r["error_rate"] is None else round(r["error_rate"], 4),
             "solved": r["solved"], "unsolved": r["unsolved"], "seconds": round(r["seconds"], 3)} for r in res]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", default=os.path.join(ROOT, "tests", "golden", "pons"))
    ap.add_argument("--params", default=None)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--games", type=int, default=256)
    ap.add_argument("--sims", type=int, default=100)
    ap.add_argument("--workers", type=int, default=128)
    ap.add_argument("--budget", type=int, default=None)
    ap.add_argument("--table-bits", type=int, default=0)
    ap.add_argument("--players", default="minmax,network_only,alphazero")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    tableless = os.path.join(ROOT, "profiles", "solver", "pons_benchmark.json")
    a.out = a.out or (os.path.join(ROOT, "profiles", "solver", "pons_benchmark_table.json") if a.table_bits > 0 else tableless)
    players = set(a.players.split(","))
    table = azhip.Solver.Table(a.table_bits) if a.table_bits > 0 else None
    before = json.load(open(tableless)) if table is not None and os.path.exists(tableless) else {}
    gspec = azhip.ConnectFourSpec()
    benchmarks = Pons.load_benchmarks(a.dir)
    cache, kw = {}, dict(num_workers=a.workers, node_budget=a.budget, table=table)
    out = {"node_budget": a.budget or azhip._lib.SOLVER_DEFAULT_BUDGET, "sets": [[b.stage, b.difficulty, len(b.entries)] for b in benchmarks]}
    if table is not None:
        out["table_bits"] = a.table_bits

    def emit(name, res):
        out[name] = rows_of(res)
        if before.get("node_budget") == out["node_budget"]:
            for r, r0 in zip(out[name], before.get(name, [])):
                r["unsolved_tableless"] = r0["unsolved"]
        print(json.dumps({"player": name, "sets": out[name]}), flush=True)

    if "minmax" in players:
        emit("minmax", Pons.test_player(lambda _: MinMax.Player(depth=5, amplify_rewards=True, τ=0), gspec, benchmarks, cache=cache, **kw))
    arena_mcts = azhip.MctsParams(num_iters_per_turn=a.sims, cpuct=2.0, dirichlet_noise_ϵ=0.05, dirichlet_noise_α=1.0,
                                  temperature=azhip.ConstSchedule(0.2))                         # examples/iteration.py's arena.mcts

    def test_network(tag, nn):
        if "network_only" in players:
            emit("network_only" + tag, Pons.test_player(lambda net: azhip.NetworkPlayer(net), gspec, benchmarks, oracle=nn, cache=cache, **kw))
        if "alphazero" in players:
            emit("alphazero" + tag, Pons.test_alphazero(gspec, nn, arena_mcts, benchmarks, cache=cache, **kw))

    if a.params:
        test_network("", load_params(a.params, gspec))
    else:                                                                                      # examples/iteration.py's loop, tested between iterations
        hp = azhip.ResNetHP(num_blocks=5, num_filters=64, num_policy_head_filters=32, num_value_head_filters=32)
        bestnn = azhip.ResNet(gspec, hp, seed=1)
        curnn = bestnn.copy_()
        sp = SelfPlayParams(
            mcts=azhip.MctsParams(num_iters_per_turn=a.sims, cpuct=2.0, dirichlet_noise_ϵ=0.25, dirichlet_noise_α=1.0,
                                  temperature=azhip.PLSchedule([0, 20, 30], [1.0, 1.0, 0.3])),
            sim=azhip.SimParams(num_games=a.games, num_workers=a.workers, batch_size=max(1, a.workers // 2), use_gpu=True, reset_every=2,
                                lock_step=True))
        ng = max(2, a.games // 4)
        arena = azhip.ArenaParams(mcts=arena_mcts,
                                  sim=azhip.SimParams(num_games=ng, num_workers=max(2, min(a.workers, ng)), batch_size=max(2, min(a.workers, ng)),
                                                      use_gpu=True, reset_every=2, flip_probability=0.5, alternate_colors=True),
                                  update_threshold=0.05)
        lp = azhip.LearningParams(samples_weighing_policy=azhip.LOG_WEIGHT, l2_regularization=1e-4, loss_computation_batch_size=1024,
                                  batch_size=256, optimiser=azhip.Adam(lr=2e-3), min_checkpoints_per_epoch=1,
                                  max_batches_per_checkpoint=2000, num_checkpoints=1)
        memory = azhip.MemoryBuffer(gspec, 400_000)
        test_network("_iter0", bestnn)
        for it in range(a.iters):
            t0 = time.perf_counter()
            curnn, bestnn, rep, lr = train_iteration(gspec, curnn, bestnn, memory, sp, lp, arena, seed=1 + it)
            print(json.dumps({"iteration": it + 1, "seconds": round(time.perf_counter() - t0, 1), "memory": rep.memory_size,
                              "nn_replaced": bool(lr.checkpoints[-1].nn_replaced)}), flush=True)
            test_network("_iter%d" % (it + 1), bestnn)
        memory.close()
    if table is not None:
        out["table_occupied"] = table.info()["occupied"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    if table is not None:
        table.close()
    azhip.clear_engine_cache()


if __name__ == "__main__":
    main()
