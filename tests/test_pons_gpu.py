"""The Pons benchmark (azhip/pons.py, the testing half of games/connect-four/scripts/pons_benchmark.jl) on the first 128 entries
of Test_L3_R1 (end game) and of Test_L2_R1 (middle game): the error rate test_player reports for a player equals the one
recomputed here, position by position, from that player's CPU reference and reference q-values.

Reference q-values: on the end-game half -azref.c4_solve(moves + [a]) and the terminal formula, exact.  On the middle-game half
an exact q of a bad move can cost the CPU negamax tens of millions of nodes, so the signs come from the device's weak mode,
cross-checked here against the CPU negamax wherever that solves the child within 20 000 nodes; a position with an unsolved move
is left out on both sides, as test_player documents."""
import functools
import os
import shutil

import numpy as np
import pytest

import azref as R
import minmax_ref as M

pytestmark = pytest.mark.gpu
PONS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pons")
NA, UNSOLVED = -128, 127
K = 128


@functools.lru_cache(maxsize=None)
def benches():
    """the two halves as Pons.Bench records"""
    from azhip import Pons
    full = {(b.stage, b.difficulty): b for b in Pons.load_benchmarks(PONS)}
    return [Pons.Bench(b.stage, b.difficulty, b.entries[:K]) for b in (full["end", "easy"], full["middle", "easy"])]


def game_of(s):
    g = R.Game(R.C4)
    for c in s:
        g.play(int(c) - 1)
    return g


@functools.lru_cache(maxsize=None)
def ref_signs():
    """per half: (n, 7) signs of the q-values (NA: full column, UNSOLVED: the position is left out), computed once"""
    import azhip
    gspec = azhip.ConnectFourSpec()
    out = []
    for b in benches():
        S = np.full((K, 7), NA, dtype=np.int64)
        keys = np.array([game_of(s).key() for s, _ in b.entries], dtype=np.uint64)
        _, wq, _ = gspec._eng().c4_solve(keys, weak=True)
        checked = 0
        for i, (s, sc) in enumerate(b.entries):
            g, moves = game_of(s), [int(c) - 1 for c in s]
            for a in g.available_actions():
                c = g.clone()
                c.play(a)
                if c.terminated():
                    exact = 0 if c.white_reward() == 0 else 21 - len(s) // 2
                else:
                    r, _ = R.c4_solve(moves + [int(a)], 20_000_000 if b.stage == "end" else 20_000)
                    exact = -r if r < 98 else None
                if exact is not None and wq[i, a] != UNSOLVED:
                    assert int(wq[i, a]) == int(np.sign(exact)), (s, a)
                    checked += 1
                S[i, a] = int(np.sign(exact)) if b.stage == "end" else int(wq[i, a])
            assert b.stage != "end" or S[i][S[i] != NA].max() == np.sign(sc)
        print("%s half: %d of %d weak q-values cross-checked against the CPU negamax" % (b.stage, checked, (S != NA).sum()))
        assert checked == (S != NA).sum() if b.stage == "end" else checked > 0     # the end game is checked whole
        out.append(S)
    return out


def expected(choices, S):
    """(error rate over the solved entries, unsolved) from each position's chosen FULL action index and the reference signs"""
    errs = unsolved = 0
    for i, a in enumerate(choices):
        avail = S[i] != NA
        if (S[i][avail] == UNSOLVED).any():
            unsolved += 1
        else:
            assert avail[a]
            errs += int(S[i][a] != S[i][avail].max())
    return errs / (len(choices) - unsolved), unsolved


def test_solver_as_the_tested_player():
    import azhip
    from azhip import Pons, Solver
    gspec = azhip.ConnectFourSpec()
    res = Pons.test_player(lambda _: Solver.Player(), gspec, benches())
    assert [(r["stage"], r["difficulty"], r["entries"]) for r in res] == [("end", "easy", K), ("middle", "easy", K)]
    for r, b in zip(res, benches()):
        keys = np.array([game_of(s).key() for s, _ in b.entries], dtype=np.uint64)
        _, q, _ = gspec._eng().c4_solve(keys)
        _, wq, _ = gspec._eng().c4_solve(keys, weak=True)
        over = int(((q == UNSOLVED).any(axis=1) | (wq == UNSOLVED).any(axis=1)).sum())     # entries with a move the budget does not reach
        assert r["unsolved"] == over and r["solved"] == K - over and r["error_rate"] == 0.0, r
        assert r["seconds"] > 0
    assert res[0]["unsolved"] == 0
    small = Pons.test_player(lambda _: Solver.Player(node_budget=16), gspec, benches()[:1], node_budget=16)[0]
    assert 0 < small["unsolved"] < K and small["error_rate"] == 0.0, small


@pytest.mark.parametrize("half", [0, 1])
def test_minmax(half):
    """MinMax.Player(depth 5, amplified rewards, τ = 0): first arg-max of tests/minmax_ref.py's π"""
    import azhip
    from azhip import MinMax, Pons
    b, S = benches()[half], ref_signs()[half]
    ref = M.MinMax(R.C4, 5, True, tau=0.0)
    G = M.GAMES[R.C4]
    choices = []
    for s, _ in b.entries:
        g = G.init()
        for c in s:
            g = G.play(g, int(c) - 1)
        acts, _, pi = ref.think(g)
        choices.append(acts[int(np.argmax(pi))])
    want = expected(choices, S)
    r = Pons.test_player(lambda _: MinMax.Player(depth=5, amplify_rewards=True, τ=0), azhip.ConnectFourSpec(), [b])[0]
    print("minmax %s: error rate %.4f, unsolved %d" % (b.stage, r["error_rate"], r["unsolved"]))
    assert (r["error_rate"], r["unsolved"]) == want


def test_mcts():
    """MctsPlayer, uniform oracle, 64 simulations: the error rates are those of MCTS.Env.explore's visit counts root by root, and do
    not depend on how many roots go into a call"""
    import azhip
    from azhip import MCTS, Pons
    gspec = azhip.ConnectFourSpec()
    params = azhip.MctsParams(num_iters_per_turn=64, dirichlet_noise_ϵ=0.0, dirichlet_noise_α=1.0, cpuct=2.0)
    make = lambda oracle: azhip.MctsPlayer(gspec, oracle, params)
    res = {w: Pons.test_player(make, gspec, benches(), oracle=MCTS.RandomOracle(gspec), num_workers=w) for w in (128, 48)}
    env = MCTS.Env(gspec, MCTS.RandomOracle(gspec), cpuct=2.0, noise_ϵ=0.0, noise_α=1.0)
    for k, (b, S) in enumerate(zip(benches(), ref_signs())):
        choices = []
        for s, _ in b.entries:
            game = gspec.init(game_of(s).key())
            env.reset()
            env.explore(game, 64)
            actions, pi = env.policy(game)
            choices.append(actions[int(np.argmax(pi))] - 1)
        want = expected(choices, S)
        for w in (128, 48):
            r = res[w][k]
            assert (r["error_rate"], r["unsolved"]) == want, (w, b.stage, r, want)
    env._e.close()


def test_solver_and_data_disagree(tmp_path):
    """an entry whose recorded sign is wrong (in a copy of the data) raises; it is not counted as the player's mistake"""
    import azhip
    from azhip import Pons, Solver
    d = tmp_path / "pons"
    d.mkdir()
    lines = open(os.path.join(PONS, "Test_L3_R1")).read().splitlines()[:16]
    s, sc = lines[5].split()
    lines[5] = "%s %d" % (s, 3 if int(sc) <= 0 else -3)
    (d / "Test_L3_R1").write_text("\n".join(lines) + "\n")
    shutil.copy(os.path.join(PONS, "Test_L2_R1"), d / "notes.txt")                       # not a benchmark file name: ignored
    bs = Pons.load_benchmarks(str(d))
    assert len(bs) == 1 and len(bs[0].entries) == 16
    with pytest.raises(Pons.SolverMismatch, match=s):
        Pons.test_player(lambda _: Solver.Player(), azhip.ConnectFourSpec(), bs)
    lines[5] = "%s %s" % (s, sc)
    (d / "Test_L3_R1").write_text("\n".join(lines) + "\n")
    r = Pons.test_player(lambda _: Solver.Player(), azhip.ConnectFourSpec(), Pons.load_benchmarks(str(d)))[0]
    assert r["error_rate"] == 0.0 and r["entries"] == 16
