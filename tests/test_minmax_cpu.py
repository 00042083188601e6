"""The MinMax baseline player (Benchmark.MinMaxTS, src/minmax.jl) without a device: the five entry points of
include/azhip.h "MinMax player" are exported and bound, think()'s π (az_minmax_policy, pure host) is bit-equal to the CPU
reference tests/minmax_ref.py on every branch, the configuration is validated with statuses and messages, the position
sets the GPU tests use cover every class of think(), and the Python hosts accept the player up to engine creation."""
import ctypes as C
import math

import numpy as np
import pytest

import azref as R
import minmax_ref as M
from azhip import _lib as L

INF = float("inf")
MINMAX_SYMBOLS = ("az_minmax_cfg_init", "az_game_heuristic", "az_minmax_qvalues", "az_minmax_policy", "az_engine_set_minmax")


def _policy(qs, tau):
    q = np.array(qs, dtype=np.float64)
    pi = np.full(len(qs), -1.0)
    L.check(L.lib().az_minmax_policy(q.ctypes.data_as(C.c_void_p), len(qs), tau, pi.ctypes.data_as(C.c_void_p)))
    return pi


def _same_bits(got, want):
    return [M.bits(x) for x in got] == [M.bits(x) for x in want]


def test_symbols_and_struct_size():
    lib = L.lib()
    for name in MINMAX_SYMBOLS:
        assert name in L.SYMBOLS and hasattr(lib, name), name
    assert L.STRUCTS[11][0] == "az_minmax_cfg"
    assert lib.az_abi_struct_size(11) == C.sizeof(L.MinMaxCfg) == 32
    assert lib.az_abi_version() == 4 and lib.az_abi_struct_size(0) == 224          # a host detects the feature by the symbols
    cfg = L.MinMaxCfg()
    L.check(lib.az_minmax_cfg_init(C.byref(cfg)))
    assert (cfg.struct_size, cfg.depth, cfg.amplify_rewards, cfg.reserved, cfg.tau, cfg.gamma) == (32, 5, 0, 0, 0.0, 1.0)
    assert L.MINMAX_MAX_DEPTH == 9


HAND_MADE = [
    [INF, 0.5, -INF], [0.1, INF, INF, -0.3],                                   # a +Inf present
    [-INF, -INF, -INF], [-INF],                                                # all -Inf
    [0.27000000000000013, 0.27000000000000013, 0.27, -1.0], [0.0, -0.0, -0.5], # ties for the maximum (and 0.0 == -0.0)
    [0.3, -0.7, 0.1, 0.3, 2.5e-3, -1.25, 0.29999999999999993],
    [-INF, 0.3, -0.7, -INF, 0.1], [-INF, -3.0],                                # some but not all -Inf
    [0.0, 0.0, 0.0], [-0.0, 0.0], [0.0],                                       # all-zero q: C = eps
    [-2.0, -5.0, -2.0000000000000004], [1e-300, -1e-300, 0.0], [12.0, -40.0, 3.0, 11.999999999999998],
]


@pytest.mark.parametrize("tau", [0.0, 0.2, 1.0, 2.5])
def test_policy_is_bit_equal_on_every_branch(tau):
    for qs in HAND_MADE:
        got, want = _policy(qs, tau), M.think_policy(qs, tau)
        assert _same_bits(got, want), (qs, tau, list(got), want)
        assert abs(sum(got) - 1.0) < 1e-12 and min(got) >= 0.0
    # the branches do what minmax.jl:91-111 says
    assert list(_policy([INF, 0.5, INF], tau)) == [0.5, 0.0, 0.5]
    assert list(_policy([-INF, -INF], tau)) == [0.5, 0.5]
    if tau == 0.0:
        assert list(_policy([0.27000000000000013, 0.27000000000000013, 0.27], tau)) == [0.5, 0.5, 0.0]
    else:
        p = _policy([-INF, 0.3, -0.7], tau)
        assert p[0] == 0.0 and p[1] > p[2] > 0.0


@pytest.fixture(scope="module")
def qsets():
    """per game: the q-vectors of the 64 positions at the depth the classes are counted at, amplify_rewards = true"""
    out = {}
    for game in (R.C4, R.TTT, R.MANCALA):
        p = M.MinMax(game, M.POSITION_SETS[game][2], True)
        out[game] = [p.qvalues(g) for g in M.positions(game)]
    return out


def test_position_sets_cover_every_class(qsets):
    """a condition on the reference alone: 64 non-terminal positions per game, at least 3 of every class of think() and
    at least 3 with fewer than A available actions"""
    for game, qv in qsets.items():
        G = M.GAMES[game]
        ps = M.positions(game)
        assert len(ps) == 64 and ps[0] == G.init() and not any(M.pyref.finished(G, g) for g in ps)
        cnt = dict(win=0, lost=0, partly_lost=0, tie=0)
        for acts, qs in qv:
            for k, v in M.classify(qs).items():
                cnt[k] += bool(v)
        few = sum(len(acts) < G.A for acts, _ in qv)
        assert all(v >= 3 for v in cnt.values()) and few >= 3, (game, cnt, few)


def test_policy_is_bit_equal_on_the_position_sets(qsets):
    for game, qv in qsets.items():
        for tau in (0.0, 0.2, 1.0, 2.5):
            for _, qs in qv:
                assert _same_bits(_policy(qs, tau), M.think_policy(qs, tau)), (game, tau, qs)


def test_reference_heuristics():
    """the reference's own two forms agree (packed Connect-Four form == cell by cell), the contract's landmark values hold"""
    for game in (R.C4, R.TTT, R.MANCALA):
        G = M.GAMES[game]
        for g in M.positions(game):
            assert M.bits(M.heuristic(G, g)) == M.bits(M.heuristic_cells(G, g))
    acts, qs = M.MinMax(R.C4, 5, False).qvalues(M.GAMES[R.C4].init())             # include/azhip.h: the opening at depth 5
    assert qs[2:5] == [0.27000000000000013, 0.27000000000000013, 0.27]        # columns 3, 4, 5 counted from 1
    assert M.heuristic(M.GAMES[R.TTT], M.GAMES[R.TTT].init()) == 0.0
    g = M.GAMES[R.TTT].play(M.GAMES[R.TTT].init(), 4)                            # centre taken: 4 of the mover's 8 alignments blocked
    assert M.heuristic(M.GAMES[R.TTT], g) == (0.09 + 0.09 + 0.09 + 0.09) - (0.09 + 0.3 + 0.09 + 0.09 + 0.3 + 0.09 + 0.3 + 0.3)
    # a drawn last move: r = 0. for the WHITE mover, the terminal child's 0. is negated, 0. + 1. * (-0.) = +0.
    p = M.MinMax(R.TTT, 1, True)
    g = M.GAMES[R.TTT].init()
    for a in (0, 1, 2, 4, 3, 5, 7, 6):
        g = M.GAMES[R.TTT].play(g, a)
    acts, qs = p.qvalues(g)
    assert acts == [8] and M.bits(qs[0]) == M.bits(0.0)
    # a BLACK mover's zero reward is -0.0: with a zero heuristic below it the q-value is -0.0 + (-0.0) = -0.0
    assert any(M.bits(q) == M.bits(-0.0) for game in (R.C4, R.TTT, R.MANCALA) for g in M.positions(game)
               for d in (1, 2) for q in M.MinMax(game, d, True).qvalues(g)[1])


def test_cfg_validation_returns_statuses_with_messages():
    """checked before the engine, so a host learns about a bad configuration without a device"""
    lib = L.lib()
    k = (C.c_uint64 * 2)(0, 0)
    q = (C.c_double * 9)()

    def cfg(**kw):
        c = L.MinMaxCfg()
        L.check(lib.az_minmax_cfg_init(C.byref(c)))
        for a, b in kw.items():
            setattr(c, a, b)
        return c
    bad = [(dict(depth=0), b"depth"), (dict(depth=L.MINMAX_MAX_DEPTH + 1), b"depth"), (dict(tau=-0.5), b"tau"),
           (dict(tau=INF), b"tau"), (dict(tau=math.nan), b"tau"), (dict(gamma=0.0), b"gamma"), (dict(gamma=-1.0), b"gamma"),
           (dict(gamma=math.nan), b"gamma"), (dict(gamma=INF), b"gamma"), (dict(struct_size=24), b"struct_size")]
    for kw, frag in bad:
        c = cfg(**kw)
        assert lib.az_engine_set_minmax(None, C.byref(c)) == L.AZ_ERR_BAD_ARG and frag in lib.az_last_error(), kw
        assert lib.az_minmax_qvalues(None, C.byref(c), k, 1, q, None) == L.AZ_ERR_BAD_ARG and frag in lib.az_last_error(), kw
    for depth in (1, L.MINMAX_MAX_DEPTH):                                        # a good one gets as far as the engine
        assert lib.az_engine_set_minmax(None, C.byref(cfg(depth=depth))) == L.AZ_ERR_BAD_ARG and b"engine" in lib.az_last_error()
    assert lib.az_minmax_qvalues(None, None, k, 1, q, None) == L.AZ_ERR_BAD_ARG and b"NULL" in lib.az_last_error()
    assert lib.az_minmax_cfg_init(None) == L.AZ_ERR_BAD_ARG
    assert lib.az_game_heuristic(None, k, 1, q) == L.AZ_ERR_BAD_ARG and b"engine" in lib.az_last_error()
    assert lib.az_minmax_policy(q, 0, 0.0, q) == L.AZ_ERR_BAD_ARG and lib.az_minmax_policy(q, 10, 0.0, q) == L.AZ_ERR_BAD_ARG
    assert lib.az_minmax_policy(q, 3, -1.0, q) == L.AZ_ERR_BAD_ARG and b"tau" in lib.az_last_error()
    assert lib.az_minmax_policy(None, 3, 0.0, q) == L.AZ_ERR_BAD_ARG
    nan = (C.c_double * 2)(0.5, math.nan)
    assert lib.az_minmax_policy(nan, 2, 0.0, q) == L.AZ_ERR_BAD_ARG and b"NaN" in lib.az_last_error()


def test_benchmark_minmaxts_instantiates_a_minmax_player():
    import azhip
    from azhip import benchmark as B, minmax as MM
    b = B.MinMaxTS(depth=6, amplify_rewards=True, τ=1.0)
    p = b.instantiate(azhip.TicTacToeSpec(), None)
    assert isinstance(p, MM.Player) and (p.depth, p.amplify_rewards, p.τ, p.gamma) == (6, True, 1.0, 1.0)
    assert b.name == "MinMax (depth 6)" and B.MinMaxTS(depth=5, amplify_rewards=False).τ == 0.0
    assert p.player_temperature(None, 3) == 1.0
    c = p.cfg()
    assert (c.struct_size, c.depth, c.amplify_rewards, c.tau, c.gamma) == (32, 6, 1, 1.0, 1.0)
    assert B.Duel(B.NetworkOnly(), b, azhip.SimParams(num_games=4, num_workers=4, batch_size=4)).name == "Network Only / MinMax (depth 6)"
    assert list(MM.policy([INF, 0.0], 0.3)) == [1.0, 0.0]


def test_arena_engine_accepts_the_minmax_player(monkeypatch):
    """arena._engine: a uniform-oracle engine with the smallest search, then set_minmax -- checked up to engine creation
    (which needs a device); every other player clears the state; Human-style players are still a TypeError"""
    import azhip
    from azhip import arena, minmax as MM
    made = []

    class FakeEngine:
        def __init__(self, role, kw):
            self.role, self.kw, self.mm = role, kw, "untouched"

        def set_minmax(self, cfg):
            self.mm = cfg

        def net_set_params(self, blob):
            pass

    def fake_cached_engine(role="", **kw):
        azhip.default_cfg(**kw)                                  # the options are real az_engine_cfg fields
        made.append(FakeEngine(role, kw))
        return made[-1]
    monkeypatch.setattr(arena, "cached_engine", fake_cached_engine)
    gspec = azhip.TicTacToeSpec()
    sim = azhip.SimParams(num_games=8, num_workers=8, batch_size=8, flip_probability=0.5)
    e = arena._engine(gspec, MM.Player(depth=6, amplify_rewards=True, τ=0.5), sim, 0, 7, "arena-black")
    assert e.kw["oracle"] == L.ORACLE_UNIFORM and e.kw["num_iters_per_turn"] == 2 and e.kw["num_workers"] == 8 and e.kw["seed"] == 7
    assert isinstance(e.mm, L.MinMaxCfg) and (e.mm.depth, e.mm.amplify_rewards, e.mm.tau, e.mm.gamma) == (6, 1, 0.5, 1.0)
    mp = azhip.MctsPlayer(gspec, azhip.MCTS.RolloutOracle(gspec), azhip.MctsParams(num_iters_per_turn=4, dirichlet_noise_ϵ=0.0, dirichlet_noise_α=1.0))
    assert arena._engine(gspec, mp, sim, 0, 7, "arena-white").mm is None          # cleared explicitly: engines are reused by role
    with pytest.raises(TypeError, match="Human"):
        arena._engine(gspec, object(), sim, 0, 7, "arena-white")
    import torch
    if not torch.cuda.is_available():                                           # the real path stops at engine creation
        monkeypatch.undo()
        with pytest.raises(L.AzError):
            arena._engine(gspec, MM.Player(depth=2, amplify_rewards=False), sim, 0, 7, "arena-black")
