"""The testing half of games/connect-four/scripts/pons_benchmark.jl: the mistake rate of a Connect-Four player on Pascal Pons'
benchmark positions (http://blog.gamesolver.org/solving-connect-four/02-test-protocol/), judged by the device solver.

A benchmark file `Test_L<stage>_R<difficulty>` holds one position per line: the moves from the empty board as a string of
1-based columns, and the position's exact score.  For each position the player thinks and takes argmax(π), the first maximum;
the move is a mistake unless sign(q[move]) == maximum(sign, q) with q from the solver (pons_benchmark.jl:101-107).

What differs from the script, all of it about how the work is laid out and none about what is computed:
  * positions are thought about in batches of up to `num_workers`, one device call per batch (az_mcts_explore with one root per
    slot, az_minmax_qvalues, az_net_evaluate_keys), not one position per call, and the solver judges a whole set in one call
    (az_c4_solve in weak mode); every MCTS slot starts from an empty tree (the script's workers keep theirs across the few
    positions of their share);
  * the solver has a node budget (include/azhip.h "Connect Four solver").  A position with a move it could not score is left out
    and counted as `unsolved`; the error rate is over the others;
  * wherever the solver does know a position's value, its sign is compared with the recorded score, and a difference raises
    SolverMismatch: that is a disagreement between the solver and the data, not a mistake of the player."""
import os
import re
import time
from dataclasses import dataclass, replace

import numpy as np

from . import _lib as L
from . import minmax as MinMax
from . import solver as Solver
from .engine import Engine
from .mcts import oracle_kind
from .params import ConstSchedule
from .play import MctsPlayer, NetworkPlayer, PlayerWithTemperature
from .trace import policy_from_visits

# `ne` elapsed moves: beginning ne <= 14, middle 14 < ne <= 28, end ne > 28 (pons_benchmark.jl:22-24)
STAGES = ["beginning", "middle", "end"]
# `nr` remaining moves: easy nr < 14, medium 14 <= nr < 28, hard nr > 28 (pons_benchmark.jl:26-28)
DIFFICULTIES = ["easy", "medium", "hard"]
NUM_WORKERS = 128


class SolverMismatch(RuntimeError):
    """the solver's value of a benchmark position does not have the sign of the recorded score"""


@dataclass
class Bench:
    stage: str
    difficulty: str
    entries: list          # [(moves string, score)]


def parse_test_filename(name):
    """(stage, difficulty) of a file named Test_L<1-3>_R<1-3>, else None (pons_benchmark.jl:31-41)"""
    m = re.fullmatch(r"Test_L(\d)_R(\d)", name)
    if not m or not (1 <= int(m.group(1)) <= 3 and 1 <= int(m.group(2)) <= 3):
        return None
    return STAGES[int(m.group(1)) - 1], DIFFICULTIES[int(m.group(2)) - 1]


def load_benchmarks(dir):
    """pons_benchmark.jl:49-75: every Test_L*_R* file of `dir`, sorted by (difficulty, stage)"""
    if not os.path.isdir(dir):
        raise FileNotFoundError("no benchmark directory %r" % (dir,))
    benchmarks = []
    for bf in sorted(os.listdir(dir)):
        meta, f = parse_test_filename(bf), os.path.join(dir, bf)
        if meta is None or not os.path.isfile(f):
            continue
        entries = []
        with open(f) as fh:
            for line in fh:
                w = line.split()
                if w:
                    entries.append((w[0], int(w[1])))
        benchmarks.append(Bench(meta[0], meta[1], entries))
    benchmarks.sort(key=lambda b: (DIFFICULTIES.index(b.difficulty), STAGES.index(b.stage)))
    return benchmarks


def state_of_string(s, gspec):
    """pons_benchmark.jl:92-99: the game after the moves of `s` (1-based columns) from the empty board"""
    g = gspec.init()
    for c in s:
        g.play(int(c))
    return g


def states_of_strings(strs, gspec):
    """current_state(state_of_string(s)) for many strings at once -> (n, 2) uint64 keys; one az_game_play per ply, not per move"""
    e = gspec._eng()
    keys = np.tile(np.array(e.init_key(), dtype=np.uint64), (len(strs), 1))
    for t in range(max((len(s) for s in strs), default=0)):
        idx = np.array([i for i, s in enumerate(strs) if len(s) > t], dtype=np.int64)
        keys[idx], _, _ = e.play(keys[idx], [int(strs[i][t]) - 1 for i in idx])
    return keys


def optimal_on(q, api):
    """pons_benchmark.jl:101-107: is the api-th available action optimal, given the solver's q-values of the available actions"""
    q = np.asarray(q, dtype=np.int64)
    return int(np.sign(q[api])) == int(np.sign(q).max())


def _first_argmax(pi, avail):
    """argmax(π) over the available actions (first maximum), as a FULL action index"""
    idx = np.flatnonzero(avail)
    return int(idx[int(np.argmax(np.asarray(pi)[idx]))])


class _Thinker:
    """think + argmax(π) for a batch of states, by the kind of player: the chosen FULL action index per state (-1: no answer)"""

    def __init__(self, player, gspec, num_workers, table=None):
        self.player, self.gspec, self.W, self.engine, self.done, self.table = player, gspec, num_workers, None, 0, table
        p = player.player if isinstance(player, PlayerWithTemperature) else player
        self.core = p
        if isinstance(p, MctsPlayer):
            mp, kind = p.params, oracle_kind(p.oracle)
            kw = p.oracle.engine_options() if kind in L.NET_ORACLES else {}
            self.engine = Engine(game=gspec.game_id, oracle=kind, num_workers=num_workers, batch_size=num_workers,
                                 num_iters_per_turn=mp.num_iters_per_turn, gamma=mp.gamma, cpuct=mp.cpuct,
                                 dirichlet_noise_eps=mp.dirichlet_noise_ϵ, dirichlet_noise_alpha=mp.dirichlet_noise_α,
                                 prior_temperature=mp.prior_temperature, seed=p.seed, reset_every=0, lock_step=1, **kw)
            if kind in L.NET_ORACLES:
                self.engine.net_set_params(p.oracle.params())

    def close(self):
        if self.engine is not None:
            self.engine.close()

    def __call__(self, keys, avail):
        p, n = self.core, keys.shape[0]
        first = self.done
        self.done += n
        if isinstance(p, MctsPlayer):
            e = self.engine
            e.mcts_reset()
            e.mcts_explore(keys, p.niters, game_ids=np.arange(first, first + n), moves=np.zeros(n))
            out = []
            for i in range(n):
                N, _, _, _, mask = e.mcts_node_stats(i, keys[i])
                m = [(mask >> a) & 1 for a in range(7)]
                pi = np.zeros(7)
                pi[np.flatnonzero(m)] = policy_from_visits(N, m)
                out.append(_first_argmax(pi, avail[i]))
            return out
        if isinstance(p, MinMax.Player):
            _, pi = self.gspec._eng().minmax_qvalues(p.cfg(), keys)
            return [_first_argmax(pi[i], avail[i]) for i in range(n)]
        if isinstance(p, NetworkPlayer):
            P, _ = p.network._eng().net_evaluate_keys(keys)
            return [_first_argmax(P[i], avail[i]) for i in range(n)]
        if isinstance(p, Solver.Player):
            _, q, _ = self.gspec._eng().c4_solve(keys, node_budget=p.node_budget, table=self.table if self.table is not None else p.table)
            return [-1 if (q[i] == Solver.UNSOLVED).any() else _first_argmax(Solver.policy(q[i]), avail[i]) for i in range(n)]
        out = []                                            # any other AbstractPlayer: its own think, a position at a time
        for i in range(n):
            actions, pi = self.player.think(self.gspec.init((int(keys[i][0]), int(keys[i][1]))))
            out.append(int(actions[int(np.argmax(pi))]) - 1)
        return out


def test_player_on(make_player, gspec, bench, oracle=None, num_workers=NUM_WORKERS, node_budget=None, progress=None, cache=None, table=None):
    """one benchmark set -> dict(stage, difficulty, error_rate over the solved entries (None without one), solved, unsolved, entries, seconds).
    cache: a dict that keeps the set's keys and solver answers for the next player tested on it with the same budget, apart for runs
    with and without a table.  table: a Solver.Table for the judging call (and for the thinking of a Solver.Player under test); it
    is meant to serve every set of a run"""
    t0 = time.perf_counter()
    ck = (bench.stage, bench.difficulty, len(bench.entries), node_budget)
    if table is not None:
        ck += ("table",)
    if cache is not None and ck in cache:
        keys, value, q = cache[ck]
    else:
        keys = states_of_strings([s for s, _ in bench.entries], gspec)
        value, q, _ = gspec._eng().c4_solve(keys, weak=True, node_budget=node_budget, table=table)   # the whole set in one launch
        if cache is not None:
            cache[ck] = keys, value, q
    if len(bench.entries) and (q == Solver.NA).all(axis=1).any():
        raise ValueError("a benchmark position is a finished game")
    for (s, score), v in zip(bench.entries, value):                  # the pin: wherever the value is known, it has the recorded sign
        if v != Solver.UNSOLVED and int(v) != int(np.sign(score)):
            raise SolverMismatch("position %s (%s, %s): the solver's value has sign %d, the recorded score is %d"
                                 % (s, bench.stage, bench.difficulty, int(v), score))
    thinker = _Thinker(make_player(oracle), gspec, num_workers, table)
    errs = unsolved = 0
    try:
        for off in range(0, len(bench.entries), num_workers):
            k, qb = keys[off:off + num_workers], q[off:off + num_workers]
            chosen = thinker(k, qb != Solver.NA)
            for i in range(k.shape[0]):
                avail = qb[i] != Solver.NA
                if chosen[i] < 0 or (qb[i][avail] == Solver.UNSOLVED).any():
                    unsolved += 1
                else:
                    idx = np.flatnonzero(avail)
                    errs += 0 if optimal_on(qb[i][idx], int(np.searchsorted(idx, chosen[i]))) else 1
                if progress is not None:
                    progress()
    finally:
        thinker.close()
    n = len(bench.entries)
    solved = n - unsolved
    return dict(stage=bench.stage, difficulty=bench.difficulty, error_rate=errs / solved if solved else None, solved=solved,
                unsolved=unsolved, entries=n, seconds=time.perf_counter() - t0)


def test_player(make_player, gspec, benchmarks, oracle=None, num_workers=NUM_WORKERS, node_budget=None, progress=None, cache=None, table=None):
    """pons_benchmark.jl:135-145: make_player(oracle) is tested on every set, in the order of `benchmarks`; one table serves them all"""
    return [test_player_on(make_player, gspec, b, oracle, num_workers, node_budget, progress, cache, table) for b in benchmarks]


def test_alphazero(gspec, nn, arena_mcts, benchmarks, **kw):
    """pons_benchmark.jl:160-168: MctsPlayer(gspec, nn, arena.mcts with temperature = ConstSchedule(0), dirichlet_noise_ϵ = 0)"""
    params = replace(arena_mcts, temperature=ConstSchedule(0.0), dirichlet_noise_ϵ=0.0)
    return test_player(lambda net: MctsPlayer(gspec, net, params), gspec, benchmarks, oracle=nn, **kw)
