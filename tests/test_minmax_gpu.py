"""The MinMax baseline player on the device (csrc/minmax.hip; contract: include/azhip.h "MinMax player") against the CPU
reference tests/minmax_ref.py: heuristics, q-values and think()'s π bit for bit (-0.0 and 0.0 told apart), the arena with
MinMax players on either side replayed whole on the CPU, the engine states, and Benchmark.run's shipped Tic-tac-toe duel.
The position sets are those tests/test_minmax_cpu.py holds to the classes of think()."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import azref as R
import minmax_ref as M
import pyref

pytestmark = pytest.mark.gpu
GAME_IDS = (R.C4, R.TTT, R.MANCALA)          # = az_game_id
_engines = {}


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for e in _engines.values():
        e.close()
    _engines.clear()


def eng(game):
    import azhip
    if game not in _engines:
        _engines[game] = azhip.Engine(game=game, oracle=azhip.ORACLE_UNIFORM, num_workers=8, batch_size=8, num_iters_per_turn=2)
    return _engines[game]


def cfg(depth, amplify, tau=0.0, gamma=1.0):
    from azhip import minmax as MM
    return MM.Player(depth, amplify, τ=tau, γ=gamma).cfg()


@functools.lru_cache(maxsize=None)
def player(game, depth, amplify, gamma=1.0):
    return M.MinMax(game, depth, amplify, gamma=gamma)


@functools.lru_cache(maxsize=None)
def ref_q(game, depth, amplify, gamma, idx):
    """the reference's (actions, q-values) of position `idx` of the game's set, computed once for all tests"""
    return player(game, depth, amplify, gamma).qvalues(M.positions(game)[idx])


def check(game, idxs, depth, amplify, gamma=1.0, tau=1.0):
    """az_minmax_qvalues on the positions idxs: Q bit-equal on the available actions, NaN elsewhere; π bit-equal, 0 elsewhere"""
    A = M.GAMES[game].A
    ps = M.positions(game)
    Q, pi = eng(game).minmax_qvalues(cfg(depth, amplify, tau, gamma), M.keys_of(game, [ps[i] for i in idxs]))
    assert Q.shape == pi.shape == (len(idxs), A)
    for row, i in enumerate(idxs):
        acts, qs = ref_q(game, depth, amplify, gamma, i)
        want_pi = M.think_policy(qs, tau)
        for a in range(A):
            if a in acts:
                k = acts.index(a)
                assert M.bits(Q[row, a]) == M.bits(qs[k]), (game, depth, i, a, Q[row, a], qs[k])
                assert M.bits(pi[row, a]) == M.bits(want_pi[k]), (game, depth, i, a, pi[row, a], want_pi[k])
            else:
                assert math.isnan(Q[row, a]) and M.bits(pi[row, a]) == M.bits(0.0), (game, depth, i, a)


@pytest.mark.parametrize("game", GAME_IDS)
def test_heuristic_is_bit_equal(game):
    ps = M.positions(game)
    h = eng(game).heuristic(M.keys_of(game, ps))
    assert [M.bits(x) for x in h] == [M.bits(M.heuristic(M.GAMES[game], g)) for g in ps]
    assert eng(game).heuristic(np.zeros((0, 2), np.uint64)).shape == (0,)


@pytest.mark.parametrize("depth", [1, 2, 3, 4])
@pytest.mark.parametrize("game", GAME_IDS)
def test_qvalues_depth_1_to_4_on_all_positions(game, depth):
    """depths 1 and 2 are shallower than any frontier split; 3 and 4 meet terminal states inside the frontier"""
    check(game, range(64), depth, True)


@pytest.mark.parametrize("amplify,gamma,tau", [(False, 1.0, 0.2), (False, 0.9, 0.0), (True, 0.9, 2.5)])
@pytest.mark.parametrize("game", GAME_IDS)
def test_qvalues_amplify_and_gamma(game, amplify, gamma, tau):
    check(game, range(64), 3, amplify, gamma, tau)


def test_connect_four_depth_5():
    """8 positions, the opening among them (its q-values are the contract's landmark)"""
    check(R.C4, range(8), 5, False, 1.0, 0.0)
    Q, pi = eng(R.C4).minmax_qvalues(cfg(5, False), M.keys_of(R.C4, [M.positions(R.C4)[0]]))
    assert list(Q[0, 2:5]) == [0.27000000000000013, 0.27000000000000013, 0.27] and list(pi[0]) == [0, 0, 0.5, 0.5, 0, 0, 0]


def test_tictactoe_depth_6_and_solved():
    check(R.TTT, range(64), 6, True, 1.0, 1.0)
    ps = M.positions(R.TTT)
    fewest = sorted(range(64), key=lambda i: (sum(c != 0 for c in ps[i][0]), i))[:8]
    assert 0 in fewest
    check(R.TTT, fewest, 9, True, 1.0, 0.0)
    check(R.TTT, fewest, 9, False, 0.9, 0.5)


def test_mancala_depth_5_with_extra_turn_chains():
    G, ps = M.GAMES[R.MANCALA], M.positions(R.MANCALA)

    def chain(g):                              # some move keeps the turn and some move after it keeps it again
        for _, nx, sw, _ in M.children(G, g):
            if not sw and not pyref.finished(G, nx) and any(not sw2 and not pyref.finished(G, n2) for _, n2, sw2, _ in M.children(G, nx)):
                return True
        return False
    chains = [i for i in range(64) if chain(ps[i])]
    assert len(chains) >= 3
    idxs = (chains + [i for i in range(64) if i not in chains])[:8]
    check(R.MANCALA, idxs, 5, True, 1.0, 1.0)
    check(R.MANCALA, idxs, 5, False, 0.9, 0.2)


@pytest.mark.parametrize("n", [1, 3, 64, 257])
def test_batch_sizes(n):
    """257 = the set cycled: it crosses any grid rounding"""
    for game in GAME_IDS:
        check(game, [i % 64 for i in range(n)], 2, True)


def test_terminated_key_and_empty_batch():
    import azhip
    from azhip import _lib as L
    for game in GAME_IDS:
        G, ps = M.GAMES[game], M.positions(game)
        g, rng = G.init(), np.random.default_rng(3)
        while not pyref.finished(G, g):
            g = G.play(g, int(rng.choice([a for a, ok in enumerate(G.mask(g)) if ok])))
        keys = M.keys_of(game, [ps[0], ps[1], g, ps[2]])
        Q = np.full((4, G.A), 7.0)
        c = cfg(3, True)
        st = L.lib().az_minmax_qvalues(eng(game)._h, C.byref(c), keys.ctypes.data_as(C.c_void_p), 4, Q.ctypes.data_as(C.c_void_p), None)
        assert st == L.AZ_ERR_BAD_ARG and b"state 2 " in L.lib().az_last_error()
        assert (Q == 7.0).all()                                                  # nothing was launched or written
        assert L.lib().az_minmax_qvalues(eng(game)._h, C.byref(c), None, 0, None, None) == L.AZ_OK
    with azhip.Engine(game=azhip.GAME_GO9_PLANES, oracle=azhip.ORACLE_RESNET, num_workers=1, batch_size=1, num_iters_per_turn=2) as e:
        for call in (lambda: e.set_minmax(cfg(3, True)), lambda: e.minmax_qvalues(cfg(3, True), [(0, 0)])):
            with pytest.raises(azhip.AzError) as ei:
                call()
            assert ei.value.status == L.AZ_ERR_BAD_ARG


# ---------------------------------------------------------------------------------------------- arena
def _arena_engine(game, workers, flip, seed, **kw):
    import azhip
    kw.setdefault("oracle", azhip.ORACLE_UNIFORM)
    kw.setdefault("num_iters_per_turn", 2)
    return azhip.Engine(game=game, num_workers=workers, batch_size=workers, flip_probability=flip, seed=seed, reset_every=1, **kw)


@pytest.mark.parametrize("game,ngames,pa,pb", [(R.TTT, 32, (2, 1.0), (6, 0.5)), (R.C4, 16, (1, 1.0), (3, 0.5))])
@pytest.mark.parametrize("flip", [0.0, 0.5])
def test_arena_minmax_against_minmax_replays_on_the_cpu(game, ngames, pa, pb, flip):
    """every record -- key, π's Float32 bits, flags 0x300 | symmetry, action, reward -- the rewards and the redundancy"""
    seed = 11
    with _arena_engine(game, 8, flip, seed) as ec, _arena_engine(game, 8, flip, seed) as eb:
        ec.set_minmax(cfg(pa[0], True, pa[1]))
        eb.set_minmax(cfg(pb[0], True, pb[1]))
        games, moves, ng, nm, rew, red = ec.arena_run(eb, ngames, alternate_colors=True)
    ref = [M.MinMax(game, pa[0], True, tau=pa[1]), M.MinMax(game, pb[0], True, tau=pb[1])]
    g_ref, rew_ref, red_ref = M.arena(game, ref, ngames, seed, True, flip)
    assert ng == ngames and nm == sum(len(r) for r, _ in g_ref)
    for i in range(ngames):
        recs, final = g_ref[i]
        g = games[i]
        assert (g.game_id, g.num_moves) == (i, len(recs)) and (g.final_key[0], g.final_key[1]) == final, i
        for k, (key, N, act, r) in enumerate(recs):
            m = moves[g.first_move + k]
            assert (m.key[0], m.key[1]) == key and list(m.N) == N and m.action == act and m.reward == r, (i, k, list(m.N), N)
    assert list(rew) == rew_ref and red == red_ref
    if flip:
        flags = {moves[i].N[R.AMAX] for i in range(nm)}
        assert 0x300 in flags and len(flags) > 1


def _verify_mixed(game, games, moves, ng, rew, seed, mm, mm_is_contender, gamma=1.0):
    """MinMax records on their own (q and π from the key, the action from the draw of game id and move index); the other
    side's records are legal moves; results follow from the moves"""
    G = M.GAMES[game]
    nmm = nother = 0
    for i in range(ng):
        gr = games[i]
        flipped = (i + 1) % 2 == 1
        g, wr, gp = G.init(), 0.0, 1.0
        for k in range(gr.num_moves):
            m = moves[gr.first_move + k]
            assert G.key(g) == (m.key[0], m.key[1]), (i, k)
            sym = m.N[R.AMAX] & 0xff
            if sym:
                g = G.symmetries(g)[sym - 1]
            contender_moves = pyref.white_playing(G, g) != flipped
            if m.N[R.AMAX] & 0x200:
                assert contender_moves == mm_is_contender and m.N[R.AMAX] & 0x100
                acts, qs, pi = mm.think(g)
                want = [0] * R.AMAX
                for a, p in zip(acts, pi):
                    want[a] = M.f32_bits(p)
                assert list(m.N)[:R.AMAX] == want, (i, k)
                assert m.action == acts[M.select_move(pi, seed, i, k)], (i, k)
                nmm += 1
            else:
                assert contender_moves != mm_is_contender and not (m.N[R.AMAX] & 0x300)
                assert G.mask(g)[m.action] and sum(m.N[:G.A]) > 0
                nother += 1
            g = G.play(g, m.action)
            assert m.reward == G.reward(g)
            wr += gp * m.reward
            gp *= gamma
        assert pyref.finished(G, g) and G.key(g) == (gr.final_key[0], gr.final_key[1])
        assert rew[i] == (-wr if flipped else wr)
    assert nmm > 0 and nother > 0


def test_arena_minmax_against_mcts_and_back():
    import azhip
    seed, flip = 5, 0.5
    mcts = dict(oracle=azhip.ORACLE_HASH, num_iters_per_turn=64, cpuct=2.0, dirichlet_noise_eps=0.05, dirichlet_noise_alpha=1.0,
                temperature=([0], [0.2]))
    mm = M.MinMax(R.C4, 3, True, tau=0.2)
    with _arena_engine(R.C4, 8, flip, seed, **mcts) as e1, _arena_engine(R.C4, 8, flip, seed) as e2:
        e2.set_minmax(cfg(3, True, 0.2))
        games, moves, ng, nm, rew, red = e1.arena_run(e2, 16, alternate_colors=True)          # MinMax as the baseline
        _verify_mixed(R.C4, games, moves, ng, rew, seed, mm, False)
        games, moves, ng, nm, rew, red = e2.arena_run(e1, 16, alternate_colors=True)          # ... and as the contender
        _verify_mixed(R.C4, games, moves, ng, rew, seed, mm, True)
        for call in (lambda: e2.selfplay_begin(4), lambda: e2.mcts_explore([e2.init_key()], 2),
                     lambda: e2.selfplay_run(2)):                                               # no search while it is a MinMax player
            with pytest.raises(azhip.AzError) as ei:
                call()
            assert ei.value.status == azhip._lib.AZ_ERR_STATE
        e2.set_minmax(None)
        e2.mcts_explore([e2.init_key()], 2)                                                     # an MCTS player again
    # the engine that was a MinMax player plays tests/test_arena_oracle.py's smallest duel like one that never was
    pl = dict(oracle=R.ORACLE_HASH, nsims=25, cpuct=1.5, noise_eps=0.25, noise_alpha=1.0)
    kw = dict(game=R.C4, oracle=azhip.ORACLE_HASH, cpuct=1.5, dirichlet_noise_eps=0.25, dirichlet_noise_alpha=1.0,
              temperature=([0], [1.0]), num_workers=3, batch_size=3, reset_every=1, seed=9)
    with azhip.Engine(num_iters_per_turn=25, **kw) as ec, azhip.Engine(num_iters_per_turn=10, **kw) as eb:
        ec.set_minmax(cfg(2, False))
        eb.set_minmax(cfg(4, True, 0.3))
        ec.arena_run(eb, 3)
        ec.set_minmax(None)
        eb.set_minmax(None)
        games, moves, ng, nm, rew, red = ec.arena_run(eb, 3)
        g_ref, m_ref, nm_ref, rew_ref, red_ref = R.arena(R.C4, 3, 3, pl, dict(pl, nsims=10), seed=9,
                                                         assignment=R.assignment_of(games, 3))
        assert ng == 3 and nm == nm_ref and np.array_equal(rew, rew_ref) and red == red_ref
        for i in range(3):
            a, b = games[i], g_ref[i]
            assert (a.game_id, a.num_moves, tuple(a.final_key)) == (b.game_id, b.num_moves, tuple(b.final_key))
            for k in range(a.num_moves):
                x, y = moves[a.first_move + k], m_ref[b.first_move + k]
                assert tuple(x.key) == tuple(y.key) and list(x.N) == list(y.N) and (x.action, x.reward) == (y.action, y.reward), (i, k)


def test_benchmark_run_of_the_shipped_tictactoe_duel(monkeypatch):
    """games/tictactoe/params.jl:79-82: Duel(NetworkOnly(), MinMaxTS(depth=6, amplify_rewards=true, τ=1.)) end to end"""
    import azhip
    from azhip import benchmark as B
    from azhip.engine import Engine
    gspec = azhip.TicTacToeSpec()
    nn = azhip.ResNet(gspec, azhip.ResNetHP(num_blocks=1, num_filters=64, num_policy_head_filters=32, num_value_head_filters=32), seed=4)
    kept, run = [], Engine.arena_run

    def spy(self, *a, **kw):
        kept.append(run(self, *a, **kw))
        return kept[-1]
    monkeypatch.setattr(Engine, "arena_run", spy)
    sim = azhip.SimParams(num_games=32, num_workers=8, batch_size=8, use_gpu=True, reset_every=1, flip_probability=0.0, alternate_colors=True)
    duel = B.Duel(B.NetworkOnly(), B.MinMaxTS(depth=6, amplify_rewards=True, τ=1.0), sim)
    ev = B.run(gspec, nn, duel, seed=3)
    assert isinstance(ev, azhip.Evaluation) and ev.legend == "Network Only / MinMax (depth 6)"
    assert len(ev.rewards) == 32 and ev.avgr == float(np.mean(ev.rewards)) and set(ev.rewards) <= {-1.0, 0.0, 1.0}
    games, moves, ng, nm, rew, red = kept[0]
    mm = M.MinMax(R.TTT, 6, True, tau=1.0)
    G = M.GAMES[R.TTT]
    nmm = 0
    for i in range(ng):
        g = G.init()
        for k in range(games[i].num_moves):
            m = moves[games[i].first_move + k]
            assert G.key(g) == tuple(m.key) and m.N[R.AMAX] & 0x100
            if m.N[R.AMAX] & 0x200:
                acts, qs, pi = mm.think(g)
                want = [0] * R.AMAX
                for a, p in zip(acts, pi):
                    want[a] = M.f32_bits(p)
                assert list(m.N)[:R.AMAX] == want and m.action == acts[M.select_move(pi, 3, i, k)], (i, k)
                nmm += 1
            g = G.play(g, m.action)
        assert pyref.finished(G, g)
    assert nmm > 32 and ev.avgr <= 0.0                        # a depth-6 search does not lose Tic-tac-toe to an untrained policy
    # host-stepped: think() through az_minmax_qvalues (play.play_game)
    p = B.MinMaxTS(depth=6, amplify_rewards=True, τ=1.0).instantiate(gspec, nn)
    actions, pi = p.think(gspec.init())
    acts, qs, want = mm.think(G.init())
    assert actions == [a + 1 for a in acts] and [M.bits(x) for x in pi] == [M.bits(x) for x in want]
    trace = azhip.play_game(gspec, azhip.TwoPlayers(p, p))
    assert len(trace) >= 5
