"""The Connect Four solver on the device (csrc/solver.hip; contract: include/azhip.h "Connect Four solver") against the scores
the reference ships (tests/golden/pons, the second column of games/connect-four/benchmark/Test_L*_R*) and against the CPU
negamax of the oracle (azref.c4_solve, used, not changed): reference q-values are -c4_solve(moves + [a]) for a child that goes
on and 0 / 21 - nstones // 2 for one that ends the game.

Budget rule asserted here (test_budget): a query is decided WITHOUT a node if the child is terminal or its mover wins with
his next stone; with ONE node if every move of the child's mover loses to the opponent's next stone, or two cells are left;
nothing else is solved at node_budget = 1."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import azref as R

pytestmark = pytest.mark.gpu
PONS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pons")
NA, UNSOLVED = -128, 127
_engines = {}


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for e in _engines.values():
        e.close()
    _engines.clear()


def eng(game=0):
    import azhip
    if game not in _engines:
        _engines[game] = azhip.Engine(game=game, oracle=azhip.ORACLE_UNIFORM, num_workers=8, batch_size=8, num_iters_per_turn=2)
    return _engines[game]


def entries(name, k=None):
    out = [(l.split()[0], int(l.split()[1])) for l in open(os.path.join(PONS, name)) if l.strip()]
    return out[:k]


def game_of(s):
    g = R.Game(R.C4)
    for c in s:
        g.play(int(c) - 1)
    return g


def keys_of(strs):
    return np.array([game_of(s).key() for s in strs], dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def end_set():
    """Test_L3_R1 (29-41 stones): entries, keys, and per entry the reference q by full action index (NA: full column)"""
    ents = entries("Test_L3_R1")
    keys, Q = keys_of([s for s, _ in ents]), np.full((len(ents), 7), NA, dtype=np.int64)
    nterminal = 0
    for i, (s, _) in enumerate(ents):
        g, moves = game_of(s), [int(c) - 1 for c in s]
        for a in g.available_actions():
            c = g.clone()
            c.play(a)
            if c.terminated():
                nterminal += 1
                Q[i, a] = 0 if c.white_reward() == 0 else 21 - len(s) // 2
            else:
                sc, _ = R.c4_solve(moves + [int(a)])
                assert sc < 98
                Q[i, a] = -sc
    assert (Q != NA).sum() == 3217 and nterminal == 65           # the figures of the issue: the reference side is what it was
    return ents, keys, Q


@functools.lru_cache(maxsize=None)
def end_strong():
    ents, keys, Q = end_set()
    return eng().c4_solve(keys)


def test_end_game_complete():
    """all 1000 end-game positions, strong mode, default budget: value = recorded score, every q = reference, nothing unsolved"""
    ents, keys, Q = end_set()
    value, q, nodes = end_strong()
    assert q.dtype == np.int8 and q.shape == (1000, 7) and value.shape == (1000,) and nodes.shape == (1000,)
    assert not (q == UNSOLVED).any() and not (value == UNSOLVED).any()
    assert np.array_equal(q.astype(np.int64), Q)                 # includes NA exactly on the full columns
    assert np.array_equal(value.astype(np.int64), np.array([sc for _, sc in ents]))
    assert np.array_equal(value.astype(np.int64), np.where(Q == NA, -99, Q).max(axis=1))
    assert (nodes >= 0).all() and nodes.max() > 0


@pytest.mark.parametrize("weak", [False, True])
def test_batch_shape(weak):
    """n = 1, 63, 64, 65 (9 states fill a wavefront: also 8, 9, 10) and 1000 give the same rows; twice the same call, the same arrays"""
    ents, keys, _ = end_set()
    full = eng().c4_solve(keys, weak=weak)
    again = eng().c4_solve(keys, weak=weak)
    for x, y in zip(full, again):
        assert np.array_equal(x, y)
    for n in (1, 8, 9, 10, 63, 64, 65):
        part = eng().c4_solve(keys[:n], weak=weak)
        for x, y in zip(part, full):
            assert np.array_equal(x, y[:n]), n
    for i in (0, 9, 63, 64, 500, 999):                           # alone, and from another place in a batch
        one = eng().c4_solve(keys[i:i + 1], weak=weak)
        shifted = eng().c4_solve(keys[i - 3 if i >= 3 else 0:i + 5], weak=weak)
        j = 3 if i >= 3 else i
        for x, y, z in zip(one, full, shifted):
            assert np.array_equal(x[0], y[i]) and np.array_equal(z[j], y[i]), i


def test_weak_mode_is_the_sign_of_strong_mode():
    ents, keys, _ = end_set()
    value, q, _ = end_strong()
    wvalue, wq, _ = eng().c4_solve(keys, weak=True)
    sgn = lambda x: np.where(x == NA, NA, np.sign(x.astype(np.int64)))
    assert np.array_equal(wq.astype(np.int64), sgn(q)) and np.array_equal(wvalue.astype(np.int64), np.sign(value.astype(np.int64)))


def test_middle_game():
    """the first 300 of Test_L2_R1 (15-28 stones; the 300 tests/golden/c4_scores.txt holds): a solved value is the recorded score
    and the maximum of the solved q; every position the CPU negamax solves within 20 000 nodes is solved at the default budget"""
    ents = entries("Test_L2_R1", 300)
    recorded = [l.split() for l in open(os.path.join(PONS, "..", "c4_scores.txt")) if l.startswith("Test_L2_R1 ")]
    assert [(s, int(sc)) for _, s, sc in recorded] == ents
    assert all(15 <= len(s) <= 28 for s, _ in ents)
    value, q, nodes = eng().c4_solve(keys_of([s for s, _ in ents]))
    cpu_solved = [R.c4_solve([int(c) - 1 for c in s], 20_000)[0] < 98 for s, _ in ents]
    assert sum(cpu_solved) == 236
    print("middle game: %d of 300 values solved, %d of %d q unsolved, %d nodes" % ((value != UNSOLVED).sum(), (q == UNSOLVED).sum(), (q != NA).sum(), nodes.sum()))
    for i, (s, sc) in enumerate(ents):
        g = game_of(s)
        assert np.array_equal(q[i] != NA, g.actions_mask()), s
        solved = q[i][(q[i] != NA) & (q[i] != UNSOLVED)]
        if value[i] != UNSOLVED:
            assert int(value[i]) == sc and int(solved.max()) == sc, (s, q[i], value[i], sc)
        else:
            assert not cpu_solved[i], "the CPU negamax solves %s within 20 000 nodes, the device does not: q = %s" % (s, q[i])
        assert (solved <= sc).all(), (s, q[i], sc)                # an exact q never exceeds the position's value


def _one_node_decides(child, stones):
    """every move of the child's mover is answered by a winning stone, or at most two cells are left (`stones` on its board)"""
    if stones >= 40:
        return True
    for m in child.available_actions():
        c2 = child.clone()
        c2.play(m)
        assert not c2.terminated()                                # the child's mover has no winning move, and more than two cells are left
        wins = False
        for w in c2.available_actions():
            c3 = c2.clone()
            c3.play(w)
            wins = wins or (c3.terminated() and c3.white_reward() != 0)
        if not wins:
            return False
    return True


def test_budget():
    """node_budget 1, 16, 256, 4096 on the end-game set: every entry is UNSOLVED or the reference; the solved set only grows; at
    budget 1 exactly the queries of the rule in this module's docstring are solved"""
    ents, keys, Q = end_set()
    prev = None
    for budget in (1, 16, 256, 4096):
        value, q, _ = eng().c4_solve(keys, node_budget=budget)
        q = q.astype(np.int64)
        solved = q != UNSOLVED
        assert np.array_equal(q[solved], Q[solved]), budget
        assert np.array_equal(q == NA, Q == NA)
        v = value.astype(np.int64)
        want = np.array([sc for _, sc in ents])
        assert ((v == UNSOLVED) | (v == want)).all(), budget
        assert (v[solved.all(axis=1)] != UNSOLVED).all()
        if prev is not None:
            assert (solved | ~prev).all(), budget
        if budget == 1:
            for i, (s, _) in enumerate(ents):
                g = game_of(s)
                for a in g.available_actions():
                    c = g.clone()
                    c.play(a)
                    free = c.terminated() or R.c4_solve([int(x) - 1 for x in s] + [int(a)], 1)[0] < 98   # the CPU negamax's first node sees a winning move
                    assert solved[i, a] == (free or _one_node_decides(c, len(s) + 1)), (s, a, q[i])
        prev = solved
    assert prev.all()                                            # 4096 nodes cover the end-game set (the largest CPU search is 8267 nodes, without the pruning)


def test_terminal_roots_and_errors():
    import azhip
    from azhip import _lib as L
    ents, _, _ = end_set()
    won = game_of("1212121")                                     # WHITE's fourth stone in column 1, his 4th of 21: BLACK to move has lost
    assert won.terminated() and won.white_reward() == 1
    s41 = next(s for s, sc in ents if len(s) == 41 and sc == 0)
    full = game_of(s41)
    full.play(int(full.available_actions()[0]))
    assert full.terminated() and full.white_reward() == 0
    for weak in (False, True):
        value, q, nodes = eng().c4_solve(np.array([won.key(), full.key()], dtype=np.uint64), weak=weak)
        assert (q == NA).all() and list(value) == [-18, 0] and list(nodes) == [0, 0]
    value, q, nodes = eng().c4_solve(np.zeros((0, 2), dtype=np.uint64))
    assert value.shape == (0,) and q.shape == (0, 7)

    lib = L.lib()
    keys = np.array([game_of("4").key()], dtype=np.uint64)
    v, q, nd = np.zeros(1, np.int8), np.zeros(7, np.int8), np.zeros(1, np.int64)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    cfg = L.SolverCfg()
    assert lib.az_solver_cfg_init(C.byref(cfg)) == 0
    assert (cfg.struct_size, cfg.weak, cfg.node_budget) == (C.sizeof(L.SolverCfg), 0, L.SOLVER_DEFAULT_BUDGET)
    assert lib.az_c4_solve(eng()._h, C.byref(cfg), vp(keys), 1, vp(v), vp(q), None) == 0           # nodes may be NULL
    assert lib.az_c4_solve(eng()._h, C.byref(cfg), None, 0, None, None, None) == 0                # n = 0

    def bad(status, *needles):
        assert status == L.AZ_ERR_BAD_ARG
        msg = lib.az_last_error().decode()
        assert msg and all(n in msg for n in needles), msg
    bad(lib.az_solver_cfg_init(None))
    bad(lib.az_c4_solve(eng()._h, None, vp(keys), 1, vp(v), vp(q), vp(nd)), "NULL")
    bad(lib.az_c4_solve(None, C.byref(cfg), vp(keys), 1, vp(v), vp(q), vp(nd)), "NULL")
    for args in ((None, 1, vp(v), vp(q)), (vp(keys), 1, None, vp(q)), (vp(keys), 1, vp(v), None)):
        bad(lib.az_c4_solve(eng()._h, C.byref(cfg), args[0], args[1], args[2], args[3], vp(nd)), "NULL")
    bad(lib.az_c4_solve(eng()._h, C.byref(cfg), vp(keys), -1, vp(v), vp(q), vp(nd)), "-1")
    wrong = L.SolverCfg(struct_size=8, weak=0, node_budget=100)
    bad(lib.az_c4_solve(eng()._h, C.byref(wrong), vp(keys), 1, vp(v), vp(q), vp(nd)), "struct_size")
    for b in (0, -5):
        zero = L.SolverCfg(struct_size=C.sizeof(L.SolverCfg), weak=0, node_budget=b)
        bad(lib.az_c4_solve(eng()._h, C.byref(zero), vp(keys), 1, vp(v), vp(q), vp(nd)), "node_budget")
    bad(lib.az_c4_solve(eng(azhip.GAME_TICTACTOE)._h, C.byref(cfg), vp(keys), 1, vp(v), vp(q), vp(nd)), "Tic-tac-toe")
    with pytest.raises(azhip.AzError):
        eng(azhip.GAME_TICTACTOE).c4_solve(keys)
    pi = np.zeros(7)
    bad(lib.az_solver_policy(None, 7, vp(pi)), "NULL")
    bad(lib.az_solver_policy(vp(q), 0, vp(pi)))


def test_player():
    """Solver.Player on 20 end-game positions spread over 29..41 stones: think is uniform over the reference's arg-max set; two
    such players playing on from there end with sign(recorded score) for the side to move; az_solver_policy rejects UNSOLVED"""
    import azhip
    from azhip import Solver
    ents, keys, Q = end_set()
    order = sorted(range(len(ents)), key=lambda i: (len(ents[i][0]), i))
    picks = [order[k * (len(order) - 1) // 19] for k in range(20)]
    assert {len(ents[i][0]) for i in picks} >= {29, 41} and len(set(picks)) == 20
    gspec, player = azhip.ConnectFourSpec(), Solver.Player()
    bench = azhip.Benchmark.Solver().instantiate(gspec, None)
    assert isinstance(bench, Solver.Player) and bench.node_budget is None
    for i in picks:
        s, sc = ents[i]
        game = gspec.init(tuple(int(x) for x in keys[i]))
        actions, pi = player.think(game)
        avail = np.flatnonzero(Q[i] != NA)
        assert actions == [int(a) + 1 for a in avail] == game.available_actions()
        best = Q[i][avail] == Q[i][avail].max()
        assert np.array_equal(pi, best / best.sum()), (s, pi, Q[i])
        acts2, qs = player.qvalues(game)
        assert acts2 == actions and list(qs) == list(Q[i][avail]) and player.value(game) == sc
        white_first = game.white_playing()
        while not game.game_terminated():
            actions, pi = player.think(game)
            game.play(actions[int(np.argmax(pi))])
        assert np.sign(game.white_reward() if white_first else -game.white_reward()) == np.sign(sc), s
        player.reset_player()
    assert np.array_equal(Solver.policy([NA, 2, -1, 2, NA, 0, 2]), [0, 1 / 3, 0, 1 / 3, 0, 0, 1 / 3])
    with pytest.raises(azhip.AzError):
        Solver.policy([NA, 2, UNSOLVED, 2, NA, 0, 2])
    hard = gspec.init(tuple(int(x) for x in keys_of(["44"])[0]))                # two stones on the board: far beyond any budget
    with pytest.raises(azhip.AzError):
        Solver.Player(node_budget=64).think(hard)
    with pytest.raises(azhip.AzError):
        Solver.Player(node_budget=64).value(hard)
