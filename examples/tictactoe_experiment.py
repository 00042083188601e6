"""The reference's Tic-tac-toe experiment (games/tictactoe/params.jl) as shipped, entirely on the MI355X engine:

  network     NetLib.SimpleNet(width 200, depth_common 6, batch norm with momentum 1.0)
  self-play   1000 games x 400 simulations on 128 workers, reset_every 4, cpuct 1, noise 0.2, temperature 1
  learning    symmetries, LOG_WEIGHT, L2 1e-4, CyclicNesterov(1e-3, 1e-2, 1e-3; momentum 0.9 / 0.8) at batch 32, one checkpoint of up to
              5000 batches, loss computed in batches of 2048, nonvalidity penalty 1
  arena       100 games on 100 workers, flip_probability 0.5, alternating colours, temperature 0.3, noise 0.1, update threshold 0
  benchmark   400 games each: AlphaZero against MCTS rollouts, and the network alone against MinMax(depth 6, amplified rewards, tau 1)
  memory      80 000 samples, analysis in 4 game stages

It prints the reports of two iterations (train!, src/training.jl:321-333) and returns them.

    python examples/tictactoe_experiment.py [--iters 2] [--games 1000] [--sims 400] [--bench-games 400] [--max-batches 5000]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "alphazero.jl_amd"))
import azhip  # noqa: E402
from azhip import Benchmark  # noqa: E402
from azhip.learning import memory_report  # noqa: E402
from azhip.training import SelfPlayParams, train_iteration  # noqa: E402


def main(iters=2, games=1000, sims=400, bench_games=400, max_batches=5000, seed=1, quiet=False):
    gspec = azhip.TicTacToeSpec()
    hp = azhip.SimpleNetHP(width=200, depth_common=6, use_batch_norm=True, batch_norm_momentum=1.0)
    bestnn = azhip.SimpleNet(gspec, hp, seed=seed)
    curnn = bestnn.copy_()
    mcts = azhip.MctsParams(num_iters_per_turn=sims, cpuct=1.0, temperature=azhip.ConstSchedule(1.0), dirichlet_noise_ϵ=0.2, dirichlet_noise_α=1.0)
    sp = SelfPlayParams(mcts=mcts, sim=azhip.SimParams(num_games=games, num_workers=128, batch_size=128, reset_every=4, flip_probability=0.0,
                                                       alternate_colors=False))
    arena_mcts = azhip.MctsParams(num_iters_per_turn=sims, cpuct=1.0, temperature=azhip.ConstSchedule(0.3), dirichlet_noise_ϵ=0.1, dirichlet_noise_α=1.0)
    arena_sim = azhip.SimParams(num_games=100, num_workers=100, batch_size=100, reset_every=1, flip_probability=0.5, alternate_colors=True)
    arena = azhip.ArenaParams(mcts=arena_mcts, sim=arena_sim, update_threshold=0.0)
    lp = azhip.LearningParams(samples_weighing_policy=azhip.LOG_WEIGHT, l2_regularization=1e-4, batch_size=32, loss_computation_batch_size=2048,
                              nonvalidity_penalty=1.0, min_checkpoints_per_epoch=0, max_batches_per_checkpoint=max_batches, num_checkpoints=1,
                              optimiser=azhip.CyclicNesterov(lr_base=1e-3, lr_high=1e-2, lr_low=1e-3, momentum_high=0.9, momentum_low=0.8))
    bench_sim = azhip.SimParams(num_games=bench_games, num_workers=100, batch_size=100, reset_every=1, flip_probability=0.5, alternate_colors=True)
    duels = [Benchmark.Duel(Benchmark.Full(mcts), Benchmark.MctsRollouts(mcts), bench_sim),
             Benchmark.Duel(Benchmark.NetworkOnly(), Benchmark.MinMaxTS(depth=6, amplify_rewards=True, τ=1.0), bench_sim)]
    memory = azhip.MemoryBuffer(gspec, 80_000)
    say = (lambda *a: None) if quiet else print
    out = []
    for it in range(iters):
        t0 = time.perf_counter()
        curnn, bestnn, rep, lr = train_iteration(gspec, curnn, bestnn, memory, sp, lp, arena, use_symmetries=True, seed=seed + it)
        t_iter = time.perf_counter() - t0
        mr = memory_report(memory, bestnn, lp, num_game_stages=4)
        evals = [Benchmark.run(gspec, bestnn, d, gamma=mcts.gamma, seed=seed + it) for d in duels]
        ck = lr.checkpoints[-1]
        say("iteration %d (%.1f s + %.1f s of benchmarks and memory analysis)" % (it + 1, t_iter, time.perf_counter() - t0 - t_iter))
        say("  self-play: %d samples in memory (%d distinct boards), %.0f samples/s" % (rep.memory_size, rep.memory_num_distinct_boards, rep.samples_gen_speed))
        say("  learning:  %d batch updates, step loss %.4f -> %.4f, status L %.4f -> %.4f (Lp %.4f Lv %.4f Lreg %.4f Linv %.4f)"
            % (len(lr.losses), lr.losses[0], lr.losses[-1], lr.initial_status.loss.L, ck.status_after.loss.L, ck.status_after.loss.Lp,
               ck.status_after.loss.Lv, ck.status_after.loss.Lreg, ck.status_after.loss.Linv))
        say("  arena:     average reward %+.3f (redundancy %.2f) -> %s" % (ck.evaluation.avgr, ck.evaluation.redundancy,
                                                                          "new best network" if ck.nn_replaced else "best network kept"))
        say("  memory:    %d samples, %d boards; by game stage: %s" % (mr.all_samples.num_samples, mr.all_samples.num_boards,
                                                                      ", ".join("L %.3f" % s.samples_stats.status.loss.L for s in mr.per_game_stage)))
        for ev in evals:
            t = Benchmark.TernaryOutcomeStatistics.of(ev.rewards)
            say("  benchmark: %-45s average reward %+.3f (%d won, %d drawn, %d lost; %.1f s)" % (ev.legend, ev.avgr, t.num_won, t.num_draw, t.num_lost, ev.time))
        out.append(dict(self_play=rep, learning=lr, memory=mr, benchmark=evals, seconds=t_iter))
    memory.close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--games", type=int, default=1000)
    ap.add_argument("--sims", type=int, default=400)
    ap.add_argument("--bench-games", type=int, default=400)
    ap.add_argument("--max-batches", type=int, default=5000)
    a = ap.parse_args()
    main(a.iters, a.games, a.sims, a.bench_games, a.max_batches)
