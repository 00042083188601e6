"""Device search trees for a host-stepped game (az_host_tree_*, csrc/host_tree.hip) against their CPU twin, oracle/pyref.Mcts.

The tree lives in HBM and asks the host one question per simulation at most; the rules here are pyref's games and one synthetic wide
game.  In host-oracle mode P / V are given and every Float64 step is specified (include/azhip.h), so every comparison is exact:
N equal, W / P / Vest bit for bit.  Engine mode is held to az_net_forward on the same rows."""
import copy
import ctypes as C

import numpy as np
import pytest

import azref as R
import pyref
from azhip import AzError, HostSteppedEnv, HostTree
from azhip.host_tree import DEPTH, FULL, PLAY, REPLY_DTYPE, ROOT

pytestmark = pytest.mark.gpu
M64 = pyref.M64


class Rules:
    """a pyref game behind the interface HostSteppedEnv drives"""

    def __init__(self, G):
        self.G = G

    def play(self, g, a):
        return self.G.play(g, a)

    def mask(self, g):
        return self.G.mask(g)

    def key(self, g):
        return self.G.key(g)

    def reward(self, g):
        return self.G.reward(g)

    def terminal(self, g):
        return pyref.finished(self.G, g)

    def white_playing(self, g):
        return pyref.white_playing(self.G, g)


class Wide:
    """Synthetic game for wide nodes: 128 actions, the legal set a function of the key, over after 3 plies (sometimes 2), rewards
    -1 / 0 / 1, the player to move does not always change, and many actions lead to one state (transpositions).
    state = ((h, ply, n), player, finished, white reward): the layout pyref.finished / white_playing / state_of read."""
    A = 128
    _masks = {}

    @staticmethod
    def root(n):
        return ((pyref.mix64(1000 + n), 0, n), 1, False, 0.0)

    @staticmethod
    def mask(g):
        h, _, n = g[0]
        if g[0] not in Wide._masks:
            order = sorted(range(128), key=lambda a: pyref.mix64((h ^ ((a + 1) * 0x9e3779b97f4a7c15)) & M64))
            legal = set(order[:n])
            Wide._masks[g[0]] = [a in legal for a in range(128)]
        return Wide._masks[g[0]]

    @staticmethod
    def play(g, a):
        (h, ply, _), player, _, _ = g
        h2 = pyref.mix64((h + (a % 7) * 0x9e37 + ply + 1) & M64)
        fin = ply + 1 >= 3 or h2 % 11 == 0
        return ((h2, ply + 1, 1 + pyref.mix64((h2 + 7) & M64) % 128), player if h2 & 3 == 0 else 3 - player, fin, float(h2 % 3 - 1) if fin else 0.0)

    @staticmethod
    def key(g):
        h, ply, n = g[0]
        return h, ply | (n << 8) | ((g[1] == 2) << 63)

    @staticmethod
    def reward(g):
        return g[3]


def full_oracle(G, oracle):
    """pyref's oracle (P by rank) as the device wants it: P by full action index"""
    def f(g):
        P, V = oracle(G, g)
        out = np.zeros(G.A, np.float32)
        out[[a for a, ok in enumerate(G.mask(g)) if ok]] = P
        return out, np.float32(V)
    return f


def eta_for(seed, game_id, move, n, alpha):
    eta = np.zeros(n)
    R.lib().azr_dirichlet(seed, game_id, move, n, alpha, eta.ctypes.data_as(C.c_void_p))
    return list(eta)


def assert_root_equal(tree, G, workers, roots, twins):
    N, W, P, Vest, root = tree.root_stats(workers)
    for i, (g, tw) in enumerate(zip(roots, twins)):
        acts = [a for a, ok in enumerate(G.mask(g)) if ok]
        rN, rW, rP, rV = tw.root_stats(g)
        assert root[i] >= 0
        assert list(N[i, acts]) == rN, (i, list(N[i, acts]), rN)
        assert np.array_equal(W[i, acts].view(np.uint64), np.array(rW, np.float64).view(np.uint64)), i
        assert np.array_equal(P[i, acts].view(np.uint32), np.array(rP, np.float32).view(np.uint32)), i
        assert np.float32(Vest[i]).view(np.uint32) == np.float32(rV).view(np.uint32), i
        rest = [a for a in range(G.A) if a not in acts]
        assert not N[i, rest].any() and not W[i, rest].any() and not P[i, rest].any()


def run_case(G, roots, nsims, oracle=pyref.hash_oracle, gamma=1.0, cpuct=1.0, eps=0.0, alpha=1.0, seed=11, nodes=4096, edges=None, depth=64):
    n = len(roots)
    tree = HostTree(G.A, n, nodes, edge_slots_per_worker=edges, max_depth=depth, gamma=gamma, cpuct=cpuct, dirichlet_noise_eps=eps,
                    dirichlet_noise_alpha=alpha, seed=seed)
    env = HostSteppedEnv(Rules(G), tree, full_oracle(G, oracle))
    gids, moves = [7 + i for i in range(n)], [3 * i for i in range(n)]
    assert env.explore(roots, nsims, game_ids=gids, moves=moves) == {}
    twins = []
    for i, g in enumerate(roots):
        tw = pyref.Mcts(G, oracle, gamma=gamma, cpuct=cpuct, eps=eps)
        tw.explore(g, nsims, eta_for(seed, gids[i], moves[i], sum(G.mask(g)), alpha) if eps else None)
        twins.append(tw)
    assert_root_equal(tree, G, list(range(n)), roots, twins)
    st = tree.stats()
    assert st["simulations"] == sum(t.total_simulations for t in twins) == n * nsims
    assert st["nodes_traversed"] == sum(t.total_nodes_traversed for t in twins)
    assert st["max_nodes"] == max(len(t.tree) for t in twins)
    return tree, env, twins, st


def test_tictactoe_terminals_and_transpositions():
    G = pyref.TicTacToe
    g0 = G.init()
    roots = [g0, G.play(G.play(g0, 4), 0), G.play(G.play(G.play(G.play(g0, 0), 4), 8), 2)]
    tree, _, _, st = run_case(G, roots, 64)
    assert st["transposition_hits"] > 0 and st["sims_without_host"] > 0
    assert st["evaluations"] > st["transposition_hits"]
    tree.close()


@pytest.mark.parametrize("gamma", [1.0, 0.9])
def test_mancala_extra_turns_and_discount(gamma):
    G = pyref.Mancala
    g0 = G.init()
    tree, _, _, _ = run_case(G, [g0, G.play(g0, 2)], 200, cpuct=2.0, gamma=gamma)   # house 3 of 3 seeds ends in the store: an extra turn
    tree.close()


def test_connect_four_dirichlet_noise_by_the_contract():
    G = pyref.ConnectFour
    g0 = G.init()
    tree, _, _, _ = run_case(G, [g0, G.play(G.play(g0, 3), 3)], 200, eps=0.25, alpha=1.0)
    tree.close()


def test_ties_take_the_first_maximum():
    G = pyref.ConnectFour
    g0 = G.init()
    tree, _, _, _ = run_case(G, [g0, G.play(g0, 0)], 100, oracle=pyref.uniform_oracle)
    tree.close()


def test_wide_nodes_lane_boundary_and_two_ranks_per_lane():
    ns = (1, 2, 63, 64, 65, 82, 128)
    roots = [Wide.root(n) for n in ns]
    assert [sum(Wide.mask(g)) for g in roots] == list(ns)
    tree, _, _, st = run_case(Wide, roots, 300, nodes=512, eps=0.25, alpha=0.5)
    assert st["transposition_hits"] > 0
    tree.close()


def test_a_game_s_worth_of_moves_then_reset():
    G = pyref.ConnectFour
    n, nsims, eps, alpha, seed = 2, 24, 0.25, 1.0, 5
    tree = HostTree(G.A, n, 2048, dirichlet_noise_eps=eps, dirichlet_noise_alpha=alpha, cpuct=1.5, seed=seed)
    env = HostSteppedEnv(Rules(G), tree, full_oracle(G, pyref.hash_oracle))
    twins = [pyref.Mcts(G, pyref.hash_oracle, cpuct=1.5, eps=eps) for _ in range(n)]
    games = [G.init(), G.play(G.init(), 6)]
    saw_root_request = False
    for move in range(5):
        assert env.explore(games, nsims, game_ids=[20, 21], moves=[move, move]) == {}
        for i in range(n):
            twins[i].explore(games[i], nsims, eta_for(seed, 20 + i, move, sum(G.mask(games[i])), alpha))
        assert_root_equal(tree, G, [0, 1], games, twins)
        pols = env.policy([0, 1])
        acts = []
        for i, (a, pi) in enumerate(pols):
            N = twins[i].root_stats(games[i])[0]
            assert np.array_equal(pi, np.array(N) / sum(N))
            acts.append(a[int(np.argmax(pi))])
        env.advance([0, 1], acts)
        games = [G.play(g, a) for g, a in zip(games, acts)]
        assert tree.root_stats([0])[4][0] >= 0
        if move == 2:                                               # worker 1 goes on along an edge nobody walked: its root becomes unknown
            N1 = tree.root_stats([1])[0][0]
            unwalked = [a for a, ok in enumerate(G.mask(games[1])) if ok and N1[a] == 0]
            assert unwalked
            env.advance([1], [unwalked[-1]])
            games[1] = G.play(games[1], unwalked[-1])
            saw_root_request = tree.root_stats([1])[4][0] == -1      # the next explore starts with a ROOT request
    assert saw_root_request
    before = tree.stats()
    env.reset([0, 1])
    assert list(tree.root_stats([0, 1])[4]) == [-1, -1]
    assert env.explore(games, nsims, game_ids=[30, 31], moves=[0, 0]) == {}
    fresh = []
    for i in range(n):
        tw = pyref.Mcts(G, pyref.hash_oracle, cpuct=1.5, eps=eps)
        tw.explore(games[i], nsims, eta_for(seed, 30 + i, 0, sum(G.mask(games[i])), alpha))
        fresh.append(tw)
    assert_root_equal(tree, G, [0, 1], games, fresh)
    assert list(tree.root_stats([0, 1])[4]) == [0, 0]                # node ids restart at 0
    assert tree.stats()["simulations"] == before["simulations"] + n * nsims
    tree.close()


def twin_until(G, g, nsims, stop):
    """the twin after the last simulation before the first one for which stop(twin before, twin after) holds, and how many that is"""
    tw = pyref.Mcts(G, pyref.hash_oracle)
    for k in range(nsims):
        prev = copy.deepcopy(tw)
        tw.explore(g, 1, None)
        if stop(prev, tw):
            return prev, k
    return tw, nsims


@pytest.mark.parametrize("kind", ["full", "depth"])
def test_capacity_starved_worker_is_disarmed_its_neighbour_is_not(kind):
    G = pyref.TicTacToe
    g0 = G.init()
    small = G.play(G.play(G.play(G.play(G.play(G.play(G.play(g0, 0), 1), 2), 4), 3), 5), 7)   # two empty squares, nobody has won
    assert not pyref.finished(G, small) and sum(G.mask(small)) == 2
    nodes, depth = (6, 64) if kind == "full" else (4096, 2)
    tree = HostTree(G.A, 2, nodes, edge_slots_per_worker=9 * 64, max_depth=depth)
    env = HostSteppedEnv(Rules(G), tree, full_oracle(G, pyref.hash_oracle))
    stopped = env.explore([g0, small], 64)
    assert stopped == {0: FULL if kind == "full" else DEPTH}
    if kind == "full":
        starved, k = twin_until(G, g0, 64, lambda a, b: len(b.tree) > nodes)
    else:
        starved, k = twin_until(G, g0, 64, lambda a, b: b.total_nodes_traversed - a.total_nodes_traversed > depth)
    assert 0 < k < 64
    neighbour = pyref.Mcts(G, pyref.hash_oracle)
    neighbour.explore(small, 64, None)
    assert_root_equal(tree, G, [0, 1], [g0, small], [starved, neighbour])
    assert tree.stats()["simulations"] == k + 64
    # the worker is disarmed: it can be reset and armed again, and the abandoned simulation left nothing behind
    env.reset([0])
    stopped = env.explore([g0], 3, workers=[0])
    again = pyref.Mcts(G, pyref.hash_oracle)
    again.explore(g0, 3, None)
    assert stopped == {} and tree.stats()["simulations"] == k + 64 + 3
    assert_root_equal(tree, G, [0], [g0], [again])
    tree.close()


def go_rows(n, seed):
    rng = np.random.default_rng(seed)
    X = rng.integers(0, 2, size=(n, 4, 9, 9)).astype(np.float32)
    A = (rng.random((n, 82)) < 0.7).astype(np.float32)
    A[:, 81] = 1.0
    return X, A


def ttt_rows(n, seed):
    rng = np.random.default_rng(seed)
    X = rng.integers(0, 2, size=(n, 3, 3, 3)).astype(np.float32)
    A = (rng.random((n, 9)) < 0.6).astype(np.float32)
    A[np.arange(n), rng.integers(0, 9, n)] = 1.0
    return X, A


def replies_for(keys, terminal=0, reward=0.0, wp=1):
    r = np.zeros(len(keys), dtype=REPLY_DTYPE)
    r["key"] = keys
    r["terminal"], r["white_reward"], r["white_playing"] = terminal, reward, wp
    return r


@pytest.mark.parametrize("W", [2, 65])
@pytest.mark.parametrize("game", ["ttt", "go9"])
def test_engine_mode_nodes_hold_what_az_net_forward_gives(game, W):
    import azhip
    from azhip.network import ResNetHP, random_params
    gid, rows, nA = (azhip.GAME_TICTACTOE, ttt_rows, 9) if game == "ttt" else (azhip.GAME_GO9_PLANES, go_rows, 82)
    hp = ResNetHP(num_blocks=1, num_filters=64, num_policy_head_filters=32, num_value_head_filters=32)
    blob = random_params(gid, hp, seed=41)
    with azhip.Engine(game=gid, oracle=azhip.ORACLE_RESNET, num_workers=1, batch_size=1, num_iters_per_turn=2, num_blocks=1, num_filters=64,
                      num_policy_head_filters=32, num_value_head_filters=32) as e:
        e.net_set_params(blob)
        tree = HostTree(nA, W, 64, engine=e)
        ws = list(range(W))
        tree.explore(ws, [0] * W, [0] * W, 2)
        reqs, _ = tree.step()
        assert list(reqs["worker"]) == ws and all(reqs["kind"] == ROOT)
        X0, A0 = rows(W, 1)
        keys0 = np.stack([np.arange(W, dtype=np.uint64) + 100, np.zeros(W, np.uint64)], 1)
        reqs, new = tree.step(replies_for(keys0), X0, A0)              # the roots are created; the second simulation asks for a move
        assert list(new) == [0] * W and all(reqs["kind"] == PLAY) and list(reqs["node"]) == [0] * W
        P0, V0, _ = e.net_forward(X0, A0)
        # second step: worker 0's move ends the game, the others reach new states: W - 1 rows, in reply order
        X1, A1 = rows(W, 2)
        keys1 = np.stack([np.arange(W, dtype=np.uint64) + 1000, np.ones(W, np.uint64)], 1)
        rep = replies_for(keys1, wp=0)
        rep["terminal"][0], rep["white_reward"][0] = 1, 1.0
        acts = list(reqs["action"])
        reqs, new = tree.step(rep, X1, A1)
        assert len(reqs) == 0 and list(new) == [-1] + [1] * (W - 1)
        P1, V1, _ = e.net_forward(X1[1:], A1[1:])
        N, Wt, P, Vest, root = tree.root_stats(ws)
        assert np.array_equal(P.view(np.uint32), P0.view(np.uint32)) and np.array_equal(Vest.view(np.uint32), V0.view(np.uint32))
        assert all(N[i, acts[i]] == 1 for i in ws) and Wt[0, acts[0]] == 1.0
        assert all(Wt[i, acts[i]] == -np.float64(V1[i - 1]) for i in ws[1:])
        # the children hold the rows of the second launch
        tree.advance(ws, acts)
        _, _, P, Vest, root = tree.root_stats(ws)
        assert list(root) == [-1] + [1] * (W - 1)
        assert np.array_equal(P[1:].view(np.uint32), P1.view(np.uint32)) and np.array_equal(Vest[1:].view(np.uint32), V1.view(np.uint32))
        # worker 0's root is unknown (the game ended there): describing it as a state the worker knows is a transposition,
        # whose row is evaluated, discarded and counted, and changes nothing
        tree.explore([0], [0], [1], 1)
        reqs, _ = tree.step()
        assert len(reqs) == 1 and reqs["kind"][0] == ROOT
        before = tree.stats()
        X2, A2 = rows(1, 3)
        reqs, new = tree.step(replies_for(keys0[:1]), X2, A2)
        assert list(new) == [0]
        st = tree.stats()
        assert st["transposition_hits"] == before["transposition_hits"] + 1 and st["evaluations"] == before["evaluations"] + 1
        while len(reqs):                                            # finish the explore: every further move ends the game
            rep = replies_for(keys1[:len(reqs)], terminal=1, reward=-1.0)
            reqs, _ = tree.step(rep)
        _, _, P, Vest, root = tree.root_stats([0])
        assert root[0] == 0 and np.array_equal(P[0].view(np.uint32), P0[0].view(np.uint32)) and Vest[0].view(np.uint32) == V0[0].view(np.uint32)
        tree.close()


MISUSES = ["reply_count", "reward", "no_legal", "mask_value", "negative_p", "p_on_illegal", "worker_range", "explore_armed"]


@pytest.mark.parametrize("misuse", MISUSES)
def test_refusals_name_the_offender_and_leave_the_tree_unchanged(misuse):
    G = pyref.TicTacToe
    g0 = G.init()
    tree = HostTree(G.A, 2, 256)
    rules, oracle = Rules(G), full_oracle(G, pyref.hash_oracle)
    env = HostSteppedEnv(rules, tree, oracle)
    tree.explore([0, 1], [0, 0], [0, 0], 24)
    reqs, _ = tree.step()
    assert len(reqs) == 2
    rows = []
    for _ in reqs:
        env._describe(g0, rows)
    rep = np.array([r[0] for r in rows], dtype=REPLY_DTYPE)
    A, P, V = np.stack([r[1] for r in rows]), np.stack([r[2] for r in rows]), np.array([r[3] for r in rows], np.float32)
    bad = dict(rep=rep.copy(), A=A.copy(), P=P.copy(), V=V.copy())
    if misuse == "reply_count":
        call, frag = lambda: tree.step(rep[:1], None, A[:1], P[:1], V[:1]), "1 replies for 2 outstanding"
    elif misuse == "reward":
        bad["rep"]["white_reward"][1] = np.inf
        call, frag = lambda: tree.step(bad["rep"], None, A, P, V), "reply 1 (worker 1): white_reward"
    elif misuse == "no_legal":
        bad["A"][1] = 0
        bad["P"][1] = 0
        call, frag = lambda: tree.step(rep, None, bad["A"], bad["P"], V), "reply 1 (worker 1): the A row has no legal action"
    elif misuse == "mask_value":
        bad["A"][0, 3] = 0.5
        call, frag = lambda: tree.step(rep, None, bad["A"], P, V), "reply 0 (worker 0): A[3]"
    elif misuse == "negative_p":
        bad["P"][1, 2] = -0.25
        call, frag = lambda: tree.step(rep, None, A, bad["P"], V), "reply 1 (worker 1): P[2]"
    elif misuse == "p_on_illegal":
        bad["A"][0, 5] = 0
        call, frag = lambda: tree.step(rep, None, bad["A"], P, V), "reply 0 (worker 0): P[5]"
    elif misuse == "worker_range":
        call, frag = lambda: tree.root_stats([0, 2]), "workers[1] = 2"
    else:
        call, frag = lambda: tree.explore([1], [0], [0], 4), "worker 1"
    with pytest.raises(AzError) as ei:
        call()
    assert frag in str(ei.value), str(ei.value)
    # nothing was stored: the correct step is still accepted and the search ends where the twin's does
    env.roots, env.states = {0: g0, 1: g0}, {0: {}, 1: {}}
    reqs, new = tree.step(rep, None, A, P, V)
    assert list(new) == [0, 0]
    for w in (0, 1):
        env.states[w][0] = g0
    while len(reqs):
        rows, asked = [], []
        for q in reqs:
            s = rules.play(env.states[int(q["worker"])][int(q["node"])], int(q["action"]))
            env._describe(s, rows)
            asked.append((int(q["worker"]), s))
        reqs, new = tree.step(np.array([r[0] for r in rows], dtype=REPLY_DTYPE), None, np.stack([r[1] for r in rows]), np.stack([r[2] for r in rows]),
                              np.array([r[3] for r in rows], np.float32))
        for (w, s), node in zip(asked, new):
            if node >= 0:
                env.states[w].setdefault(int(node), s)
    twins = []
    for _ in range(2):
        tw = pyref.Mcts(G, pyref.hash_oracle)
        tw.explore(g0, 24, None)
        twins.append(tw)
    assert_root_equal(tree, G, [0, 1], [g0, g0], twins)
    tree.close()


def test_prior_temperature_other_than_one_is_refused():
    with pytest.raises(AzError) as ei:
        HostTree(9, 1, 16, prior_temperature=0.5)
    assert "prior_temperature" in str(ei.value)
    with pytest.raises(AzError):
        HostTree(129, 1, 16)
