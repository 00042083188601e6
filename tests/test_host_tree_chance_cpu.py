"""The chance mode of the device search trees (AZ_HOST_TREE_CHANCE) without a GPU: the flag and the new entry point in the header,
the library, the mirror and the Julia glue; HostSteppedEnv's one-env-per-worker protocol over the reference trees of mdp_ref
against the direct recursion on the same generator streams; GridWorldRules against hand-written transitions."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mdp_ref as M
import pyref
from azhip import GridWorldRules, HostSteppedEnv
from azhip import _lib as L

ROOT_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flags_default_to_zero_and_unknown_bits_are_refused_by_name():
    lib = L.lib()
    cfg = L.HostTreeCfg()
    L.check(lib.az_host_tree_cfg_init(C.byref(cfg)))
    assert cfg.flags == 0 and L.HOST_TREE_CHANCE == 1
    h = C.c_void_p()
    for flags, bit in ((2, b"bit 0x2"), (3, b"bit 0x2"), (0x41, b"bit 0x40"), (-2147483648, b"bit 0x80000000")):
        cfg.flags = flags
        # device 99 does not exist: the refusal comes before a device is touched
        assert lib.az_host_tree_create(None, 99, 9, 2, 16, 144, 8, C.byref(cfg), C.byref(h)) == L.AZ_ERR_BAD_ARG
        err = lib.az_last_error()
        assert b"flags" in err and bit in err and b"AZ_HOST_TREE_CHANCE" in err and not h.value, err


def test_the_new_symbol_is_declared_exported_mirrored_and_named_in_the_glue():
    hdr = open(os.path.join(ROOT_DIR, "include", "azhip.h")).read()
    jl = open(os.path.join(ROOT_DIR, "julia", "AlphaZeroHIPExtras.jl")).read()
    name = "az_host_tree_request_depths"
    assert name in L.SYMBOLS and hasattr(L.lib(), name) and re.search(r"\bint %s\(az_host_tree\* t, int32_t\* depths, int32_t cap, int32_t\* n\);" % name, hdr)
    assert re.search(r":%s\b" % name, jl)
    assert "#define AZ_HOST_TREE_CHANCE 1" in hdr and re.search(r"int32_t flags;", hdr) and "#define AZ_ABI_VERSION 4" in hdr
    assert (C.sizeof(L.HostTreeReply), C.sizeof(L.HostTreeRequest), C.sizeof(L.HostTreeCfg), C.sizeof(L.HostTreeStats)) == (24, 16, 56, 72)
    assert L.HostTreeCfg.flags.offset == 4 and L.HostTreeCfg.gamma.offset == 8
    n = C.c_int32(5)
    assert L.lib().az_host_tree_request_depths(None, None, 0, C.byref(n)) == L.AZ_ERR_BAD_ARG
    assert len(re.findall(r"^int az_\w+\(", hdr, flags=re.M)) + len(re.findall(r"^const char\* az_\w+\(", hdr, flags=re.M)) == len(L.SYMBOLS) == 101


def grid_case(W, seed, size=(10, 10), **kw):
    """PerWorker grid-world rules for the tree under test and their twin for the reference, and one start state per worker"""
    def make():
        return M.PerWorker([GridWorldRules(size=size, rng=M.philox(seed, w), **kw) for w in range(W)])
    starts = np.random.default_rng(seed).integers(1, 11, size=(W, 2))
    rules, twin = make(), make()
    games = [(w, (min(int(x), size[0]), min(int(y), size[1]), 0)) for w, (x, y) in enumerate(starts)]
    games = [g if not rules.terminal(g) else (g[0], (1, 1, 0)) for g in games]
    return rules, twin, games


@pytest.mark.parametrize("gamma", [1.0, 0.9])
def test_host_stepped_env_over_the_reference_tree_equals_the_direct_recursion(gamma):
    """grid-world episodes with advance and one reset: HostSteppedEnv keeps one simulation env per worker, cloned from the root at
    depth 0, and every worker ends with the N, W and counters of run_simulation! called directly"""
    W, nA = 3, 4
    rules, twin, games = grid_case(W, 21)
    tree = M.RefTree(nA, W, 4096, max_depth=256, gamma=gamma, chance=True)     # a path ends when time passes the bound of 200 at the latest
    env = HostSteppedEnv(rules, tree, M.key_oracle(rules, nA))
    assert env.chance
    refs = [M.RefSearch(twin, M.key_oracle(twin, nA), gamma=gamma, max_depth=256, max_nodes=4096, max_edges=4096 * nA) for _ in range(W)]
    assert M.play_episodes(env, refs, twin, games, 50, nA, 10, reset_after=6) > 0
    st = tree.stats()
    assert st["sims_without_host"] == 0 and st["transposition_hits"] > 0 and st["steps"] > st["simulations"] / W


def test_one_edge_many_times_on_a_path_with_its_own_reward_each_time():
    W = 2
    mk = lambda: M.PerWorker([M.OneState(M.philox(3, w)) for w in range(W)])
    rules, twin = mk(), mk()
    oracle = lambda s: (np.ones(1, np.float32), np.float32(0.25))
    tree = M.RefTree(1, W, 8, max_depth=64, gamma=0.9, chance=True)
    env = HostSteppedEnv(rules, tree, oracle)
    refs = [M.RefSearch(twin, oracle, gamma=0.9, max_depth=64, max_nodes=8, max_edges=8) for _ in range(W)]
    games = [(w, (True, 0.0)) for w in range(W)]
    assert env.explore(games, 40) == {}
    for w in range(W):
        assert refs[w].explore(games[w], 40) is None
    st = M.assert_same(tree, refs, 1)
    assert 8 <= st["max_path"] < 64 and st["max_nodes"] == 1


def test_the_deterministic_reference_tree_is_the_oracle_s_twin():
    """RefTree(chance=False) remembers edges as the device does: pyref.Mcts's statistics, and simulations that never ask"""
    from test_host_tree_gpu import Rules, full_oracle
    G = pyref.TicTacToe
    g0 = G.init()
    roots = [g0, G.play(G.play(g0, 4), 0)]
    tree = M.RefTree(9, 2, 4096, max_depth=64, gamma=0.9)
    env = HostSteppedEnv(Rules(G), tree, full_oracle(G, pyref.hash_oracle))
    assert not env.chance and env.explore(roots, 64) == {}
    N, Wt, P, Vest, root = tree.root_stats([0, 1])
    for i, g in enumerate(roots):
        tw = pyref.Mcts(G, pyref.hash_oracle, gamma=0.9)
        tw.explore(g, 64, None)
        acts = [a for a, ok in enumerate(G.mask(g)) if ok]
        rN, rW, rP, rV = tw.root_stats(g)
        assert list(N[i, acts]) == rN and np.array_equal(Wt[i, acts].view(np.uint64), np.array(rW, np.float64).view(np.uint64))
    assert tree.stats()["sims_without_host"] > 0


def test_a_request_about_a_node_whose_key_the_env_does_not_stand_in_is_an_error():
    rules, _, games = grid_case(1, 5)
    tree = M.RefTree(4, 1, 64, chance=True)
    env = HostSteppedEnv(rules, tree, M.key_oracle(rules, 4))
    env.explore(games, 3)
    env.states[0][0] = (0, 0)
    with pytest.raises(RuntimeError, match="node 0"):
        env.explore(games, 3)


def test_grid_world_rules_against_hand_written_transitions():
    class Fixed:
        """random() = 1.0: never slips"""
        def random(self):
            return 1.0
    r = GridWorldRules(rng=Fixed())
    assert r.size == (10, 10) and r.rewards == {(9, 3): 10.0, (8, 8): 3.0, (4, 3): -10.0, (4, 6): -5.0} and r.slip == 0.4 and r.episode_length_bound == 200
    # r, l, u, d on the indices 0..3 (game.jl:37), time counts the moves
    assert [r.play((5, 5, 7), a) for a in range(4)] == [(6, 5, 8), (4, 5, 8), (5, 6, 8), (5, 4, 8)]
    # clamped at all four walls (game.jl:48)
    assert r.play((10, 4, 0), 0) == (10, 4, 1) and r.play((1, 4, 0), 1) == (1, 4, 1)
    assert r.play((3, 10, 0), 2) == (3, 10, 1) and r.play((3, 1, 0), 3) == (3, 1, 1)
    # the four reward cells are terminal and pay on arrival; nothing else pays
    for cell, rew in r.rewards.items():
        s = cell + (3,)
        assert r.terminal(s) and r.reward(s) == rew
    assert r.play((8, 3, 0), 0) == (9, 3, 1) and r.reward((9, 3, 1)) == 10.0
    assert not r.terminal((5, 5, 200)) and r.reward((5, 5, 200)) == 0.0
    # time > bound ends the episode (game.jl:40-41); time is not in the key
    assert r.terminal((5, 5, 201)) and r.key((5, 5, 201)) == r.key((5, 5, 0)) != r.key((5, 6, 0)) and r.key((6, 5, 0)) != r.key((5, 6, 0))
    assert list(r.mask((5, 5, 0))) == [True] * 4 and r.white_playing((5, 5, 0)) is True
    X = r.planes((2, 7, 0))
    assert X.shape == (1, 10, 10) and X.sum() == 1.0 and X[0, 6, 1] == 1.0
    # a slip draws the direction uniformly (game.jl:45-47): 0.4 * 3/4 = 30 % of the moves go wrong
    r = GridWorldRules(rng=np.random.default_rng(4))
    wrong = sum(r.play((5, 5, 0), 0) != (6, 5, 1) for _ in range(4000))
    assert 0.27 < wrong / 4000 < 0.33
    # on the 9 x 9 x 4 / 82-action geometry: the same cells, the moves on the first four action indices, plane 0
    import azhip
    g = GridWorldRules(size=(9, 9), gspec=azhip.Go9PlanesSpec(), rng=Fixed())
    assert g.rewards == r.rewards and g.play((9, 9, 0), 0) == (9, 9, 1)
    m = g.mask((1, 1, 0))
    assert m.shape == (82,) and m[:4].all() and not m[4:].any()
    X = g.planes((9, 1, 0))
    assert X.shape == (4, 9, 9) and X.sum() == 1.0 and X[0, 0, 8] == 1.0
    with pytest.raises(ValueError):
        GridWorldRules(size=(7, 7))                                     # a 7 x 7 world does not hold the default cells
