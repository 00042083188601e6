"""The Connect Four solver with a transposition table on the device (az_c4_solve_table, csrc/solver.h k_c4_solve_table; contract:
include/azhip.h "Connect Four solver", "table"): exact or unsolved whatever the table holds, and many more positions solved.

References: the recorded scores of tests/golden/pons, the tableless az_c4_solve, and on the end-game set the q-values of the CPU
negamax as test_solver_gpu.end_set builds them (computed once per session, shared with that module).  Budgets are 2^18 nodes or
less: the budget is what bounds a call's time.  Which positions finish under a budget is NOT asserted anywhere except as the
coverage condition of test_coverage, which the issue sets: at most half as many positions left without a value as without a table."""
import ctypes as C
import functools

import numpy as np
import pytest

from test_solver_gpu import NA, UNSOLVED, _engines, end_set, eng, entries, game_of, keys_of

pytestmark = pytest.mark.gpu
BUDGET = 1 << 18


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for e in _engines.values():
        e.close()
    _engines.clear()


@functools.lru_cache(maxsize=None)
def middle_set():
    """the first 200 of Test_L2_R2 (middle / medium): entries, keys, recorded scores, availability masks"""
    ents = entries("Test_L2_R2", 200)
    keys = keys_of([s for s, _ in ents])
    mask = np.array([game_of(s).actions_mask() for s, _ in ents], dtype=bool)
    return ents, keys, np.array([sc for _, sc in ents], dtype=np.int64), mask


def check_exact(value, q, score, mask, weak=False):
    """a solved value is the recorded score, a solved q is no more than it, NA sits exactly on the full columns"""
    value, q = value.astype(np.int64), q.astype(np.int64)
    want = np.sign(score) if weak else score
    assert np.array_equal(q != NA, mask)
    known = value != UNSOLVED
    assert np.array_equal(value[known], want[known])
    solved = (q != NA) & (q != UNSOLVED)
    assert (q <= want[:, None])[solved].all()
    full = known & ~(q == UNSOLVED).any(axis=1)                  # every q solved: the value is their maximum
    assert np.array_equal(np.where(q == NA, -99, q).max(axis=1)[full], want[full])
    return known


@pytest.mark.parametrize("weak", [False, True])
def test_exact_on_the_end_set(weak):
    """1000 end-game positions, table of 2^16 entries: the arrays of az_c4_solve and of the reference"""
    import azhip
    ents, keys, Q = end_set()
    plain = eng().c4_solve(keys, weak=weak, node_budget=BUDGET)
    with azhip.Solver.Table(16) as t:
        value, q, nodes = eng().c4_solve(keys, weak=weak, node_budget=BUDGET, table=t)
        assert np.array_equal(value, plain[0]) and np.array_equal(q, plain[1])
        want = np.where(Q == NA, NA, np.sign(Q)) if weak else Q
        assert np.array_equal(q.astype(np.int64), want)          # includes NA exactly on the full columns
        score = np.array([sc for _, sc in ents])
        assert np.array_equal(value.astype(np.int64), np.sign(score) if weak else score)
        assert (nodes >= 0).all() and nodes.max() > 0
        won, s41 = game_of("1212121"), next(s for s, sc in ents if len(s) == 41 and sc == 0)
        full = game_of(s41)
        full.play(int(full.available_actions()[0]))
        assert won.terminated() and full.terminated() and full.white_reward() == 0
        value, q, nodes = eng().c4_solve(np.array([won.key(), full.key()], dtype=np.uint64), weak=weak, table=t)
        assert (q == NA).all() and list(value) == [-18, 0] and list(nodes) == [0, 0]


@pytest.mark.parametrize("log2_entries", [0, 4, 20])
def test_exact_under_replacement(log2_entries):
    """a table of one entry replaces on every store, one of 16 nearly so: what is solved is still exact"""
    import azhip
    ents, keys, score, mask = middle_set()
    with azhip.Solver.Table(log2_entries) as t:
        value, q, nodes = eng().c4_solve(keys, node_budget=BUDGET, table=t)
        known = check_exact(value, q, score, mask)
        print("2^%d entries: %d of 200 values known, %d nodes, %d entries occupied" % (log2_entries, known.sum(), nodes.sum(), t.info()["occupied"]))
        assert t.info() == dict(log2_entries=log2_entries, bytes=8 << log2_entries, occupied=t.info()["occupied"])
        assert 0 < t.info()["occupied"] <= 1 << log2_entries


@functools.lru_cache(maxsize=None)
def cold_call():
    """the 200 middle / medium positions without a table and with a cold one of 2^23 entries, which stays open for test_warm_table"""
    import azhip
    ents, keys, score, mask = middle_set()
    plain = eng().c4_solve(keys, node_budget=BUDGET)
    t = azhip.Solver.Table(23)
    return plain, eng().c4_solve(keys, node_budget=BUDGET, table=t), t


def test_coverage():
    """the table call leaves at most half as many positions without a value as the tableless call, and knows every value that one knows"""
    ents, keys, score, mask = middle_set()
    plain, cold, _ = cold_call()
    check_exact(plain[0], plain[1], score, mask)
    check_exact(cold[0], cold[1], score, mask)
    left_plain, left_table = int((plain[0] == UNSOLVED).sum()), int((cold[0] == UNSOLVED).sum())
    print("values unknown of 200 at 2^18 nodes: %d without a table, %d with one of 2^23 entries; nodes %d and %d"
          % (left_plain, left_table, plain[2].sum(), cold[2].sum()))
    assert left_plain > 0
    assert 2 * left_table <= left_plain
    known = plain[0] != UNSOLVED
    assert np.array_equal(cold[0][known], plain[0][known])


def test_warm_table():
    """the same call again: a superset solved, equal values, strictly fewer nodes; cleared, the table is empty and the call a cold one"""
    ents, keys, score, mask = middle_set()
    _, cold, t = cold_call()
    try:
        assert t.info()["occupied"] > 0
        warm = eng().c4_solve(keys, node_budget=BUDGET, table=t)
        check_exact(warm[0], warm[1], score, mask)
        assert ((warm[0] != UNSOLVED) | (cold[0] == UNSOLVED)).all()
        known = cold[0] != UNSOLVED
        assert np.array_equal(warm[0][known], cold[0][known])
        print("nodes: cold %d, warm %d" % (cold[2].sum(), warm[2].sum()))
        assert warm[2].sum() < cold[2].sum()
        t.clear()
        assert t.info()["occupied"] == 0
        again = eng().c4_solve(keys, node_budget=BUDGET, table=t)
        check_exact(again[0], again[1], score, mask)
        both = (again[0] != UNSOLVED) & known
        assert np.array_equal(again[0][both], cold[0][both])
    finally:
        t.close()
        cold_call.cache_clear()


def test_shared_and_mixed():
    """one table under two engines and under weak and strong calls in turn; batch shapes"""
    import azhip
    ents, keys, score, mask = middle_set()
    keys, score, mask = keys[:65], score[:65], mask[:65]
    other = azhip.Engine(game=0, oracle=azhip.ORACLE_UNIFORM, num_workers=8, batch_size=8, num_iters_per_turn=2)
    try:
        with azhip.Solver.Table(18) as t:
            runs = []
            for engine, weak in ((eng(), False), (other, True), (eng(), True), (other, False), (eng(), False)):
                value, q, _ = engine.c4_solve(keys, weak=weak, node_budget=1 << 14, table=t)
                check_exact(value, q, score, mask, weak)
                runs.append((weak, value.astype(np.int64)))
            for weak, v in runs:                                 # weak is the sign of strong wherever both are solved
                for weak2, v2 in runs:
                    both = (v != UNSOLVED) & (v2 != UNSOLVED)
                    a, b = (v if weak else np.sign(v)), (v2 if weak2 else np.sign(v2))
                    assert np.array_equal(a[both], b[both])
            full = runs[-1][1]
            for n in (1, 8, 9, 10, 63, 64, 65):
                value, q, _ = (other if n % 2 else eng()).c4_solve(keys[:n], node_budget=1 << 14, table=t)
                check_exact(value, q, score[:n], mask[:n])
                both = (value != UNSOLVED) & (full[:n] != UNSOLVED)
                assert np.array_equal(value.astype(np.int64)[both], full[:n][both]), n
    finally:
        other.close()


def test_errors():
    import azhip
    from azhip import _lib as L
    lib = L.lib()
    keys = np.array([game_of("4").key()], dtype=np.uint64)
    v, q, nd = np.zeros(1, np.int8), np.zeros(7, np.int8), np.zeros(1, np.int64)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    cfg = L.SolverCfg()
    assert lib.az_solver_cfg_init(C.byref(cfg)) == 0
    cfg.node_budget = 256

    def bad(status, *needles):
        assert status == L.AZ_ERR_BAD_ARG
        msg = lib.az_last_error().decode()
        assert msg and all(n in msg for n in needles), msg
    h = C.c_void_p()
    bad(lib.az_solver_table_create(0, 4, None), "NULL")
    for lg in (-1, 31):
        bad(lib.az_solver_table_create(0, lg, C.byref(h)), "log2_entries", str(lg))
        assert not h.value
    bad(lib.az_solver_table_create(-1, 4, C.byref(h)), "device")
    bad(lib.az_solver_table_clear(None), "NULL")
    bad(lib.az_solver_table_info(None, None, None, None), "NULL")
    assert lib.az_solver_table_destroy(None) == 0
    assert lib.az_solver_table_create(0, 4, C.byref(h)) == 0 and h.value
    assert lib.az_solver_table_destroy(h) == 0
    assert lib.az_solver_table_create(0, 4, C.byref(h)) == 0 and h.value          # destroy, then create again
    try:
        assert lib.az_solver_table_info(h, None, None, None) == 0
        lg, nbytes, occ = C.c_int32(), C.c_int64(), C.c_int64()
        assert lib.az_solver_table_info(h, C.byref(lg), C.byref(nbytes), C.byref(occ)) == 0 and (lg.value, nbytes.value, occ.value) == (4, 128, 0)
        assert lib.az_c4_solve_table(eng()._h, C.byref(cfg), h, vp(keys), 1, vp(v), vp(q), None) == 0          # nodes may be NULL
        assert lib.az_c4_solve_table(eng()._h, C.byref(cfg), h, None, 0, None, None, None) == 0               # n = 0
        bad(lib.az_c4_solve_table(eng()._h, C.byref(cfg), None, vp(keys), 1, vp(v), vp(q), vp(nd)), "table", "NULL")
        bad(lib.az_c4_solve_table(eng()._h, None, h, vp(keys), 1, vp(v), vp(q), vp(nd)), "NULL")
        bad(lib.az_c4_solve_table(None, C.byref(cfg), h, vp(keys), 1, vp(v), vp(q), vp(nd)), "NULL")
        for args in ((None, vp(v), vp(q)), (vp(keys), None, vp(q)), (vp(keys), vp(v), None)):
            bad(lib.az_c4_solve_table(eng()._h, C.byref(cfg), h, args[0], 1, args[1], args[2], vp(nd)), "NULL")
        bad(lib.az_c4_solve_table(eng()._h, C.byref(cfg), h, vp(keys), -1, vp(v), vp(q), vp(nd)), "-1")
        wrong = L.SolverCfg(struct_size=8, weak=0, node_budget=100)
        bad(lib.az_c4_solve_table(eng()._h, C.byref(wrong), h, vp(keys), 1, vp(v), vp(q), vp(nd)), "struct_size")
        zero = L.SolverCfg(struct_size=C.sizeof(L.SolverCfg), weak=0, node_budget=0)
        bad(lib.az_c4_solve_table(eng()._h, C.byref(zero), h, vp(keys), 1, vp(v), vp(q), vp(nd)), "node_budget")
        bad(lib.az_c4_solve_table(eng(azhip.GAME_TICTACTOE)._h, C.byref(cfg), h, vp(keys), 1, vp(v), vp(q), vp(nd)), "Tic-tac-toe")
        bad(lib.az_c4_solve_table(eng(azhip.GAME_TICTACTOE)._h, C.byref(cfg), None, vp(keys), 1, vp(v), vp(q), vp(nd)), "Tic-tac-toe")   # the game comes first
    finally:
        assert lib.az_solver_table_destroy(h) == 0
    with pytest.raises(azhip.AzError):
        azhip.Solver.Table(31)


def test_table_of_another_device():
    import azhip
    import torch
    from azhip import _lib as L
    if torch.cuda.device_count() < 2:
        pytest.skip("a table of another device needs two devices")
    lib = L.lib()
    keys = np.array([game_of("4").key()], dtype=np.uint64)
    v, q, nd = np.zeros(1, np.int8), np.zeros(7, np.int8), np.zeros(1, np.int64)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    cfg = L.SolverCfg()
    assert lib.az_solver_cfg_init(C.byref(cfg)) == 0
    with azhip.Solver.Table(4, device=1) as far:
        assert lib.az_c4_solve_table(eng()._h, C.byref(cfg), far._h, vp(keys), 1, vp(v), vp(q), vp(nd)) == L.AZ_ERR_BAD_ARG
        msg = lib.az_last_error().decode()
        assert "device 1" in msg and "device 0" in msg, msg


def test_player_with_a_table():
    """Solver.Player(table=t) thinks about five end-game positions and plays them out, as test_solver_gpu.test_player does"""
    import azhip
    from azhip import Solver
    ents, keys, Q = end_set()
    order = sorted(range(len(ents)), key=lambda i: (len(ents[i][0]), i))
    picks = [order[k * (len(order) - 1) // 4] for k in range(5)]
    gspec = azhip.ConnectFourSpec()
    with Solver.Table(16) as t:
        player = Solver.Player(node_budget=BUDGET, table=t)
        bench = azhip.Benchmark.Solver(table=t).instantiate(gspec, None)
        assert isinstance(bench, Solver.Player) and bench.table is t and bench.node_budget is None
        assert Solver.Player().table is None and azhip.Benchmark.Solver().instantiate(gspec, None).table is None
        for i in picks:
            s, sc = ents[i]
            game = gspec.init(tuple(int(x) for x in keys[i]))
            actions, pi = player.think(game)
            avail = np.flatnonzero(Q[i] != NA)
            assert actions == [int(a) + 1 for a in avail]
            best = Q[i][avail] == Q[i][avail].max()
            assert np.array_equal(pi, best / best.sum()), (s, pi, Q[i])
            acts2, qs = player.qvalues(game)
            assert acts2 == actions and list(qs) == list(Q[i][avail]) and player.value(game) == sc
            white_first = game.white_playing()
            while not game.game_terminated():
                actions, pi = player.think(game)
                game.play(actions[int(np.argmax(pi))])
            assert np.sign(game.white_reward() if white_first else -game.white_reward()) == np.sign(sc), s
        assert t.info()["occupied"] > 0


def test_pons_with_a_table():
    """Pons.test_player_on over the first 64 of middle / medium: with a table no more positions are left out, no SolverMismatch,
    and the result cache keeps the judgements with and without a table apart"""
    import azhip
    from azhip import Pons, Solver
    gspec = azhip.ConnectFourSpec()
    bench = Pons.Bench("middle", "medium", entries("Test_L2_R2", 64))
    cache = {}
    plain = Pons.test_player_on(lambda _: Solver.Player(node_budget=1 << 14), gspec, bench, node_budget=1 << 16, cache=cache)
    assert len(cache) == 1
    with Solver.Table(20) as t:
        res = Pons.test_player_on(lambda _: Solver.Player(node_budget=1 << 14), gspec, bench, node_budget=1 << 16, cache=cache, table=t)
        assert len(cache) == 2                                   # the tableless judgement was not handed to the run with a table
        (res2,) = Pons.test_player(lambda _: Solver.Player(node_budget=1 << 14, table=t), gspec, [bench], node_budget=1 << 16, table=t)
    print("left out of 64: %d without a table, %d with one, %d on the warm table" % (plain["unsolved"], res["unsolved"], res2["unsolved"]))
    assert res["entries"] == 64 and res["unsolved"] <= plain["unsolved"] and res2["unsolved"] <= plain["unsolved"]
    for r in (plain, res, res2):
        assert r["error_rate"] is None or r["error_rate"] == 0.0  # a perfect player makes no mistake where it answers
