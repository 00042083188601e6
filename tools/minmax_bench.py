#!/usr/bin/env python
"""What does the MinMax baseline player (Benchmark.MinMaxTS, csrc/minmax.hip) cost on the device?

1. az_minmax_qvalues after a warm-up, timed with a HIP event pair on the legacy default stream around the call (the engine's
   stream is a blocking stream, so the pair brackets its copies and the kernel): Connect Four depth 5 at n = 128 and n = 4096,
   Tic-tac-toe depth 6 at n = 128, on positions reached by random play.  Reports positions/s and leaves/s (leaves = the paths of
   the exhaustive walk: those that reach the depth limit or end in a terminal state before it, counted with az_game_play in
   batches on the first 128 positions and scaled to n).
2. One 128-game Connect-Four duel Full (5 x 128 ResNet, 600 simulations) against MinMaxTS(depth = 5, tau = 0.2) through
   az_arena_run: wall time, the MCTS player's device time (az_prof: HIP events around every kernel of its engine) and the
   MinMax player's think -- its records replayed ply by ply through az_minmax_qvalues under the same event pair.  The yardstick
   is the other player of the same run: the MinMax side should be a small fraction of the MCTS side (above one tenth the kernel
   leaves the chip idle).

    python tools/minmax_bench.py [--reps 5] [--games 128] [--sims 600] [--skip-duel]

Prints one JSON line per measurement.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "alphazero.jl_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import azhip  # noqa: E402
from azhip import arena, minmax as MM  # noqa: E402
from azhip import _lib as L  # noqa: E402


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return out, a.elapsed_time(b), (time.perf_counter() - t0) * 1e3


def random_positions(e, n, max_plies, seed):
    """n non-terminal states reached by 0..max_plies uniformly random moves (rules on the device: az_game_play / az_game_encode)"""
    rng = np.random.default_rng(seed)
    keys = np.tile(np.array(e.init_key(), dtype=np.uint64), (n, 1))
    plies = rng.integers(0, max_plies + 1, n)
    for k in range(max_plies):
        _, A = e.encode(keys)
        acts = np.array([rng.choice(np.flatnonzero(A[i] > 0)) for i in range(n)], dtype=np.int32)
        acts[plies <= k] = -1
        nxt, term, _ = e.play(keys, acts)
        keep = ~term                                     # a move that would end the game is not played: the state stays
        keys[keep] = nxt[keep]
    return keys


def count_leaves(e, keys, depth):
    """leaves of the exhaustive walk: paths that reach depth `depth` or end in a terminal state before it"""
    leaves, frontier = 0, np.ascontiguousarray(keys)
    for d in range(depth):
        _, A = e.encode(frontier)
        idx, act = np.nonzero(A > 0)
        nxt, term, _ = e.play(frontier[idx], act.astype(np.int32))
        leaves += int(term.sum())
        frontier = nxt[~term]
        if not len(frontier):
            break
    return leaves + len(frontier)


def bench_qvalues(game, name, depth, n, reps, max_plies):
    with azhip.Engine(game=game, oracle=azhip.ORACLE_UNIFORM, num_workers=8, batch_size=8, num_iters_per_turn=2) as e:
        keys = random_positions(e, n, max_plies, seed=n + depth)
        cfg = MM.Player(depth, True, τ=0.2).cfg()
        leaves = count_leaves(e, keys[:128], depth) * (n // 128)       # the first 128 stand for the set (n is a multiple)
        e.minmax_qvalues(cfg, keys)                                    # warm-up: code object load, staging buffers
        ms = sorted(event_ms(lambda: e.minmax_qvalues(cfg, keys))[1:] for _ in range(reps))
        dev, wall = ms[len(ms) // 2]
        print(json.dumps({"what": "az_minmax_qvalues", "game": name, "depth": depth, "n": n, "reps": reps, "event_ms_median": round(dev, 4),
                          "event_ms_min": round(ms[0][0], 4), "wall_ms_median": round(wall, 4), "positions_per_s": round(n / dev * 1e3),
                          "leaves": leaves, "leaves_per_s": round(leaves / dev * 1e3)}), flush=True)


def bench_duel(games, sims, depth):
    gspec = azhip.ConnectFourSpec()
    hp = azhip.ResNetHP(num_blocks=5, num_filters=128, num_policy_head_filters=32, num_value_head_filters=32)
    nn = azhip.ResNet(gspec, hp, seed=7)
    mp = azhip.MctsParams(num_iters_per_turn=sims, cpuct=2.0, dirichlet_noise_ϵ=0.05, dirichlet_noise_α=1.0, temperature=azhip.ConstSchedule(0.2))
    sim = azhip.SimParams(num_games=games, num_workers=games, batch_size=games, use_gpu=True, reset_every=2, flip_probability=0.5,
                          alternate_colors=True, lock_step=True)
    player = MM.Player(depth, False, τ=0.2)
    ec = arena._engine(gspec, azhip.MctsPlayer(gspec, nn, mp), sim, 0, 1, "arena-white")
    eb = arena._engine(gspec, player, sim, 0, 1, "arena-black")
    ec.arena_run(eb, min(games, 8), alternate_colors=True)              # warm-up
    ec.prof_reset()
    ec.prof_enable(True)
    t0 = time.perf_counter()
    g, m, ng, nm, rew, red = ec.arena_run(eb, games, alternate_colors=True)
    wall = time.perf_counter() - t0
    prof = ec.prof_get()
    ec.prof_enable(False)
    mcts_ms = sum(v["ms"] for v in prof.values())
    # the MinMax player's think, ply by ply: with as many workers as games every game is at the same ply in every round
    by_ply = {}
    for i in range(ng):
        for k in range(g[i].num_moves):
            r = m[g[i].first_move + k]
            if r.N[L.MAX_ACTIONS] & 0x200:
                by_ply.setdefault(k, []).append((int(r.key[0]), int(r.key[1])))
    cfg, mm_ms, mm_wall, nthink = player.cfg(), 0.0, 0.0, 0
    for k in sorted(by_ply):
        keys = np.array(by_ply[k], dtype=np.uint64)
        _, dev, w = event_ms(lambda: eb.minmax_qvalues(cfg, keys))
        mm_ms, mm_wall, nthink = mm_ms + dev, mm_wall + w, nthink + len(keys)
    print(json.dumps({"what": "duel Full 5x128 vs MinMaxTS", "games": ng, "simulations": sims, "minmax_depth": depth, "wall_s": round(wall, 3),
                      "moves": nm, "minmax_moves": nthink, "mcts_device_ms": round(mcts_ms, 2), "minmax_think_event_ms": round(mm_ms, 3),
                      "minmax_think_wall_ms": round(mm_wall, 3), "minmax_over_mcts": round(mm_ms / mcts_ms, 5),
                      "avg_reward_of_full": float(np.mean(rew)), "redundancy": round(red, 4),
                      "note": "records of flipped turns are replayed on the un-flipped state: the mirror image costs the same walk"}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--games", type=int, default=128)
    ap.add_argument("--sims", type=int, default=600)
    ap.add_argument("--depth", type=int, default=5)
    ap.add_argument("--skip-duel", action="store_true")
    a = ap.parse_args()
    bench_qvalues(azhip.GAME_CONNECT_FOUR, "connect-four", 5, 128, a.reps, 20)
    bench_qvalues(azhip.GAME_CONNECT_FOUR, "connect-four", 5, 4096, a.reps, 20)
    bench_qvalues(azhip.GAME_TICTACTOE, "tictactoe", 6, 128, a.reps, 3)
    if not a.skip_duel:
        bench_duel(a.games, a.sims, a.depth)
    azhip.clear_engine_cache()


if __name__ == "__main__":
    main()
