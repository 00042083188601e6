"""The chance mode of the device search trees (AZ_HOST_TREE_CHANCE, csrc/host_tree.hip) against mdp_ref.RefSearch: run_simulation!
with a play! that is random, restated in Python Float64.  The device's rules and the reference's draw from identical per-worker
Philox streams, so every comparison is exact: after every explore N equal, W as Float64 bits, P, Vest and the counters
(simulations, nodes_traversed, evaluations, transposition_hits, sims_without_host and the high-water marks)."""
import numpy as np
import pytest

import mdp_ref as M
import pyref
from azhip import GridWorldRules, HostSteppedEnv, HostTree
from azhip.host_tree import DEPTH, FULL, PLAY, ROOT
from test_host_tree_gpu import Rules, eta_for, full_oracle

pytestmark = pytest.mark.gpu


def per_worker(make, W):
    """the rules of the tree under test and their twin for the reference: make(w) is called twice per worker, with equal streams"""
    return M.PerWorker([make(w) for w in range(W)]), M.PerWorker([make(w) for w in range(W)])


def explore_both(env, refs, games, nsims, nA, etas=None, **kw):
    assert env.explore(games, nsims, **kw) == {}
    for w, g in enumerate(games):
        assert refs[w].explore(g, nsims, None if etas is None else etas[w]) is None
    return M.assert_same(env.tree, refs, nA)


# W = 65 bounds its episodes at 10 moves (episode_length_bound 9) and plays them to their end (at most 12 real moves, the reset after the fifth): once a worker
# knows its part of the world a simulation only ends on a reward cell or at the time bound, and with the bound of 200 the 65 x 50
# simulations of ONE real move walk some 10^5 plies through the Python rules.  W = 2 keeps the reference's bound and plays the 12 moves
@pytest.mark.parametrize("W,gamma,max_moves,reset_after,bound", [(2, 1.0, 12, 6, 200), (2, 0.9, 12, 6, 200), (65, 1.0, 12, 4, 9), (65, 0.9, 12, 4, 9)])
def test_grid_world_episodes_with_advance_and_reset(W, gamma, max_moves, reset_after, bound):
    """games/grid-world 10 x 10, 50 simulations per move: whole episodes of at most 12 real moves.  After every real move the root is
    unknown to the device; the next explore finds it again by key and goes on from its earlier visits"""
    nA = 4
    rules, twin = per_worker(lambda w: GridWorldRules(episode_length_bound=bound, rng=M.philox(21, w)), W)
    starts = np.random.default_rng(8).integers(1, 11, size=(W, 2))
    games = [(w, (int(x), int(y), 0)) for w, (x, y) in enumerate(starts)]
    games = [g if not rules.terminal(g) else (g[0], (1, 1, 0)) for g in games]
    with HostTree(nA, W, 2048, max_depth=256, gamma=gamma, chance=True) as tree:   # time > 200 ends every path
        env = HostSteppedEnv(rules, tree, M.key_oracle(rules, nA))
        refs = [M.RefSearch(twin, M.key_oracle(twin, nA), gamma=gamma, max_depth=256, max_nodes=2048, max_edges=2048 * nA) for _ in range(W)]
        assert M.play_episodes(env, refs, twin, games, 50, nA, max_moves, reset_after=reset_after) > 0
        st = tree.stats()
        assert st["sims_without_host"] == 0 and st["transposition_hits"] > 0


def test_one_edge_stands_many_times_on_a_path_with_different_rewards():
    """one state, one action: it stays with +1, stays with -1, or ends.  Every path is that edge again and again; the backup of a
    repeated edge goes one entry at a time with the entry's own reward.  max_depth 64; with these streams the reference alone
    never comes near it (its longest path is asserted), so no worker is cut short"""
    W, nsims = 3, 60
    rules, twin = per_worker(lambda w: M.OneState(M.philox(3, w)), W)
    oracle = lambda s: (np.ones(1, np.float32), np.float32(0.25))
    games = [(w, (True, 0.0)) for w in range(W)]
    with HostTree(1, W, 8, max_depth=64, gamma=0.9, chance=True) as tree:
        refs = [M.RefSearch(twin, oracle, gamma=0.9, max_depth=64, max_nodes=8, max_edges=8) for _ in range(W)]
        st = explore_both(HostSteppedEnv(rules, tree, oracle), refs, games, nsims, 1)
        longest = max(r.max_path for r in refs)
        assert 16 <= longest < 64 and st["max_path"] == longest and st["max_nodes"] == 1
        assert st["nodes_traversed"] > 4 * W * nsims


def test_paths_longer_than_one_chunk_of_the_unwind():
    """a corridor of 80 cells, no slip, the prior all on "right" (action index 0), V = 0: simulation k walks k - 1 cells, so 75
    simulations pass 64 path entries and the backup reads the entries' side arrays in two chunks"""
    W, nA = 2, 4
    rules, twin = per_worker(lambda w: GridWorldRules(size=(80, 1), rewards={(80, 1): 1.0}, slip=0.0, rng=M.philox(1, w)), W)
    oracle = lambda s: (np.array([1, 0, 0, 0], np.float32), np.float32(0.0))
    games = [(w, (1, 1, 0)) for w in range(W)]
    with HostTree(nA, W, 128, max_depth=128, gamma=0.9, chance=True) as tree:
        refs = [M.RefSearch(twin, oracle, gamma=0.9, max_depth=128, max_nodes=128, max_edges=128 * nA) for _ in range(W)]
        st = explore_both(HostSteppedEnv(rules, tree, oracle), refs, games, 75, nA)
        assert st["max_path"] == 74 and st["max_nodes"] == 75


def test_wide_nodes_with_random_outcomes_and_noise_at_the_root():
    """100 actions, all legal at the root: two ranks per lane.  Dirichlet noise at the root by the contract of the deterministic mode"""
    ns, nA, eps, alpha, seed = (1, 2, 3), 100, 0.25, 0.5, 11
    W = len(ns)
    rules, twin = per_worker(lambda w: M.WideChance(M.philox(9, w)), W)
    games = [(w, M.WideChance.root(n)) for w, n in enumerate(ns)]
    gids, moves = [7 + w for w in range(W)], [3 * w for w in range(W)]
    with HostTree(nA, W, 512, max_depth=8, dirichlet_noise_eps=eps, dirichlet_noise_alpha=alpha, seed=seed, chance=True) as tree:
        refs = [M.RefSearch(twin, M.key_oracle(twin, nA), eps=eps, max_depth=8, max_nodes=512, max_edges=512 * nA) for _ in range(W)]
        etas = [eta_for(seed, gids[w], moves[w], 100, alpha) for w in range(W)]
        st = explore_both(HostSteppedEnv(rules, tree, M.key_oracle(rules, nA)), refs, games, 300, nA, etas, game_ids=gids, moves=moves)
        assert st["transposition_hits"] > 0 and st["max_edge_slots"] > 200


def ttt_oracle(s):
    P, V = pyref.hash_oracle(pyref.TicTacToe, s[1])
    out = np.zeros(9, np.float32)
    out[[a for a, ok in enumerate(pyref.TicTacToe.mask(s[1])) if ok]] = P
    return out, np.float32(V)


def test_slippery_tictactoe_two_players():
    """with probability 0.3 the mark lands on another free cell: pswitch is true on every entry, and one (state, action) is followed
    by terminal and non-terminal states in turn"""
    G = pyref.TicTacToe
    g0 = G.init()
    W = 3
    rules, twin = per_worker(lambda w: M.Slippery(G, M.philox(17, w)), W)
    games = [(0, g0), (1, G.play(G.play(g0, 4), 0)), (2, G.play(G.play(G.play(G.play(g0, 0), 4), 8), 2))]
    with HostTree(9, W, 4096, max_depth=16, gamma=0.9, chance=True) as tree:
        refs = [M.RefSearch(twin, ttt_oracle, gamma=0.9, max_depth=16, max_nodes=4096, max_edges=4096 * 9) for _ in range(W)]
        env = HostSteppedEnv(rules, tree, ttt_oracle)
        for _ in range(2):                                              # the second explore goes on in the same trees
            st = explore_both(env, refs, games, 100, 9)
        assert st["transposition_hits"] > 0 and st["evaluations"] > st["transposition_hits"]


class ForwardTap:
    """a HostTree in engine mode, watched: before every step the rows of its non-terminal replies go through az_net_forward as well,
    in the same order and number, and what comes back is queued per worker for the reference's oracle"""

    def __init__(self, tree, engine):
        self.tree, self.engine, self.asked, self.queues = tree, engine, [], {}

    def __getattr__(self, name):
        return getattr(self.tree, name)

    def step(self, replies=None, X=None, A=None, P=None, V=None):
        if replies is not None and len(replies):
            rows = [i for i in range(len(replies)) if not replies["terminal"][i]]
            if rows:
                Pn, Vn, _ = self.engine.net_forward(np.ascontiguousarray(X[rows]), np.ascontiguousarray(A[rows]))
                for k, i in enumerate(rows):
                    self.queues.setdefault(self.asked[i], []).append((tuple(map(int, replies["key"][i])), Pn[k].copy(), np.float32(Vn[k])))
        reqs, new = self.tree.step(replies, X, A, P, V)
        self.asked = [int(q["worker"]) for q in reqs if q["kind"] in (PLAY, ROOT)]
        return reqs, new


@pytest.mark.parametrize("W", [2, 65])
def test_engine_mode_nodes_hold_what_az_net_forward_gives(W):
    """engine mode on the Tic-tac-toe geometry with the slippery rules: the reference is fed az_net_forward's outputs for the same
    planes (ForwardTap), and the device's nodes hold exactly those P / Vest -- and so the same N and W"""
    import azhip
    from azhip.network import ResNetHP, random_params
    G = pyref.TicTacToe
    g0 = G.init()
    hp = ResNetHP(num_blocks=1, num_filters=64, num_policy_head_filters=32, num_value_head_filters=32)
    rules, twin = per_worker(lambda w: M.Slippery(G, M.philox(29, w)), W)
    games = [(w, G.play(g0, w % 9) if w % 2 else g0) for w in range(W)]
    with azhip.Engine(game=azhip.GAME_TICTACTOE, oracle=azhip.ORACLE_RESNET, num_workers=1, batch_size=1, num_iters_per_turn=2, num_blocks=1,
                      num_filters=64, num_policy_head_filters=32, num_value_head_filters=32) as e:
        e.net_set_params(random_params(azhip.GAME_TICTACTOE, hp, seed=41))
        with HostTree(9, W, 256, max_depth=16, engine=e, chance=True) as tree:
            tap = ForwardTap(tree, e)
            env = HostSteppedEnv(rules, tap)
            assert env.explore(games, 24) == {}

            def oracle_of(w):
                def f(s):
                    key, P, V = tap.queues[w].pop(0)
                    assert key == tuple(map(int, twin.key(s)))
                    return P, V
                return f
            refs = [M.RefSearch(twin, oracle_of(w), max_depth=16, max_nodes=256, max_edges=256 * 9) for w in range(W)]
            for w, g in enumerate(games):
                assert refs[w].explore(g, 24) is None
            assert not any(tap.queues.values())
            st = M.assert_same(tree, refs, 9)
            assert st["evaluations"] > st["transposition_hits"] > 0


@pytest.mark.parametrize("kind", ["depth", "full"])
def test_a_starved_worker_is_disarmed_its_neighbour_is_not(kind):
    """AZ_HT_DEPTH with max_depth 4 on the one-state MDP, AZ_HT_FULL with 3 nodes on grid-world: worker 0 is stopped, nothing of
    the abandoned simulation is kept, worker 1 (whose game stays within the bounds) ends with the reference's results"""
    if kind == "depth":
        nA, nodes, depth = 1, 8, 4
        make = lambda w: M.OneState(M.philox(3, w), p_end=0.15 if w == 0 else 1.0)      # the neighbour's episodes end at once
        oracle = lambda rules: (lambda s: (np.ones(1, np.float32), np.float32(0.25)))
        games = [(0, (True, 0.0)), (1, (True, 0.0))]
    else:
        nA, nodes, depth = 4, 3, 256
        make = lambda w: GridWorldRules(rng=M.philox(5, w)) if w == 0 else GridWorldRules(size=(2, 1), rewards={(2, 1): 1.0}, rng=M.philox(5, w))
        oracle = lambda rules: M.key_oracle(rules, nA)
        games = [(0, (2, 2, 0)), (1, (1, 1, 0))]
    rules, twin = per_worker(make, 2)
    with HostTree(nA, 2, nodes, max_depth=depth, chance=True) as tree:
        env = HostSteppedEnv(rules, tree, oracle(rules))
        refs = [M.RefSearch(twin, oracle(twin), max_depth=depth, max_nodes=nodes, max_edges=nodes * nA) for _ in range(2)]
        want = DEPTH if kind == "depth" else FULL
        assert env.explore(games, 64) == {0: want}
        assert refs[0].explore(games[0], 64) == want and refs[1].explore(games[1], 64) is None
        st = M.assert_same(tree, refs, nA)
        assert 64 < st["simulations"] < 128
        # disarmed: it can be reset and armed again
        env.reset([0])
        refs[0].reset()
        again = refs[0].explore(games[0], 2)
        assert env.explore([games[0]], 2, workers=[0]) == ({} if again is None else {0: again})
        M.assert_same(tree, refs, nA)


class DepthLog:
    """a tree whose every step is followed by request_depths(): log = per step the (worker, kind, depth) of its questions"""

    def __init__(self, tree):
        self.tree, self.log = tree, []

    def __getattr__(self, name):
        return getattr(self.tree, name)

    def step(self, *a, **kw):
        reqs, new = self.tree.step(*a, **kw)
        ask = [q for q in reqs if q["kind"] in (PLAY, ROOT)]
        depths = self.tree.request_depths()
        assert len(depths) == len(ask)
        self.log.append([(int(q["worker"]), int(q["kind"]), int(d)) for q, d in zip(ask, depths)])
        return reqs, new


def test_request_depths_in_both_modes():
    """deterministic: the path length the reference tree has at each request.  Chance: that too, and 0 exactly at the first
    request of every simulation"""
    G = pyref.TicTacToe
    g0 = G.init()
    roots = [g0, G.play(G.play(g0, 4), 0)]
    with HostTree(9, 2, 4096, max_depth=16) as tree:
        dev, ref = DepthLog(tree), DepthLog(M.RefTree(9, 2, 4096, max_depth=16))
        for t in (dev, ref):
            assert HostSteppedEnv(Rules(G), t, full_oracle(G, pyref.hash_oracle)).explore(roots, 64) == {}
        assert dev.log == ref.log and max(d for step in dev.log for _, _, d in step) >= 3
        assert [d for _, k, d in dev.log[0]] == [0, 0] and all(k == ROOT for _, k, _ in dev.log[0])
    W, nsims = 3, 40
    with HostTree(4, W, 1024, max_depth=256, chance=True) as tree:
        dev, ref = DepthLog(tree), DepthLog(M.RefTree(4, W, 1024, max_depth=256, chance=True))
        for t in (dev, ref):
            rules = M.PerWorker([GridWorldRules(rng=M.philox(2, w)) for w in range(W)])
            env = HostSteppedEnv(rules, t, M.key_oracle(rules, 4))
            games = [(w, (2 + w, 5, 0)) for w in range(W)]
            assert env.explore(games, 1) == {}                          # the roots are created
            t.log.clear()
            before = t.stats()["simulations"]
            assert env.explore(games, nsims) == {} and t.stats()["simulations"] == before + W * nsims
        assert dev.log == ref.log
        for w in range(W):
            mine = [d for step in dev.log for ww, _, d in step if ww == w]
            assert mine.count(0) == nsims and mine[0] == 0 and max(mine) >= 2
            assert all(b == 0 or b == a + 1 for a, b in zip(mine, mine[1:]))


def test_the_deterministic_mode_of_a_chance_capable_build_is_the_oracle_s_twin():
    """flags = 0: the Tic-tac-toe case of tests/test_host_tree_gpu.py, root statistics bit-equal to oracle/pyref.Mcts"""
    from test_host_tree_gpu import run_case
    G = pyref.TicTacToe
    g0 = G.init()
    tree, _, _, st = run_case(G, [g0, G.play(G.play(g0, 4), 0), G.play(G.play(G.play(G.play(g0, 0), 4), 8), 2)], 64, gamma=0.9)
    assert tree.chance is False and len(tree.request_depths()) == 0
    assert st["transposition_hits"] > 0 and st["sims_without_host"] > 0
    tree.close()
