"""The static parts of the device search trees for a host-stepped game (az_host_tree_*), without a GPU: the entry points are
declared, exported, mirrored and accounted for in the Julia glue, and HostSteppedEnv keeps the host's states by (worker, node id)
as the protocol requires -- exercised against a fake tree that asks scripted questions."""
import ctypes as C
import os
import re

import numpy as np

from azhip import _lib as L
from azhip import HostSteppedEnv, HostTree
from azhip.host_tree import DEPTH, FULL, PLAY, REPLY_DTYPE, REQUEST_DTYPE, ROOT

ROOT_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("az_host_tree_cfg_init", "az_host_tree_create", "az_host_tree_destroy", "az_host_tree_explore", "az_host_tree_step",
           "az_host_tree_root_stats", "az_host_tree_advance", "az_host_tree_reset", "az_host_tree_get_stats")


def test_symbols_are_declared_exported_and_mirrored():
    hdr = open(os.path.join(ROOT_DIR, "include", "azhip.h")).read()
    lib = L.lib()
    for name in SYMBOLS:
        assert name in L.SYMBOLS and hasattr(lib, name) and re.search(r"\bint %s\(" % name, hdr), name
    assert "#define AZ_HOST_TREE_MAX_ACTIONS 128" in hdr and L.HOST_TREE_MAX_ACTIONS == 128
    assert "#define AZ_ABI_VERSION 4" in hdr and L.ABI_VERSION == 4
    assert (C.sizeof(L.HostTreeReply), C.sizeof(L.HostTreeRequest), C.sizeof(L.HostTreeCfg), C.sizeof(L.HostTreeStats)) == (24, 16, 56, 72)
    assert REPLY_DTYPE.itemsize == 24 and REQUEST_DTYPE.itemsize == 16
    assert (PLAY, ROOT, FULL, DEPTH) == (0, 1, 2, 3)
    for name, kind in zip(("AZ_HT_PLAY", "AZ_HT_ROOT", "AZ_HT_FULL", "AZ_HT_DEPTH"), (PLAY, ROOT, FULL, DEPTH)):
        assert re.search(r"\b%s = %d\b" % (name, kind), hdr)


def test_cfg_defaults_and_host_side_refusals():
    """what az_host_tree_create refuses before it touches a device"""
    lib = L.lib()
    cfg = L.HostTreeCfg()
    L.check(lib.az_host_tree_cfg_init(C.byref(cfg)))
    assert cfg.struct_size == C.sizeof(L.HostTreeCfg)
    assert (cfg.gamma, cfg.cpuct, cfg.dirichlet_noise_eps, cfg.dirichlet_noise_alpha, cfg.prior_temperature, cfg.seed) == (1.0, 1.0, 0.0, 1.0, 1.0, 0)
    assert lib.az_host_tree_cfg_init(None) == L.AZ_ERR_BAD_ARG
    h = C.c_void_p()

    def create(nA=9, W=2, nodes=16, edges=144, depth=8):
        return lib.az_host_tree_create(None, 0, nA, W, nodes, edges, depth, C.byref(cfg), C.byref(h))
    cfg.prior_temperature = 0.5
    assert create() == L.AZ_ERR_BAD_ARG and b"prior_temperature" in lib.az_last_error() and not h.value
    cfg.prior_temperature = 1.0
    for kw, frag in ((dict(nA=129), b"num_actions"), (dict(nA=0), b"num_actions"), (dict(W=0), b"num_workers"), (dict(nodes=0), b"nodes_per_worker"),
                     (dict(edges=8), b"edge_slots_per_worker"), (dict(depth=0), b"max_depth")):
        assert create(**kw) == L.AZ_ERR_BAD_ARG and frag in lib.az_last_error() and not h.value, kw
    cfg.struct_size = 8
    assert create() == L.AZ_ERR_BAD_ARG and b"struct_size" in lib.az_last_error()
    assert lib.az_host_tree_destroy(None) == 0
    assert lib.az_host_tree_step(None, 0, None, None, None, None, None, None, None, None) == L.AZ_ERR_BAD_ARG


def test_julia_glue_names_every_entry_point():
    jl = open(os.path.join(ROOT_DIR, "julia", "AlphaZeroHIPExtras.jl")).read()
    for name in SYMBOLS:
        assert re.search(r":%s\b" % name, jl) or ("(:%s, LIB)" % name) in jl, name


class Counting:
    """states are integers: play adds the action + 1, the game ends at 6 or above; every method counts its calls"""
    A = 3

    def __init__(self):
        self.plays = []

    def play(self, s, a):
        self.plays.append((s, a))
        return s + a + 1

    def mask(self, s):
        return [True, s % 2 == 0, True]

    def key(self, s):
        return (s, 1 << 63)

    def reward(self, s):
        return 1.0 if s >= 6 else 0.0

    def terminal(self, s):
        return s >= 6

    def white_playing(self, s):
        return s % 2 == 0


class FakeTree:
    """answers like az_host_tree_step from a script: per step the requests to hand out and the node ids the replies get"""
    num_actions = 3

    def __init__(self, script):
        self.script, self.calls, self.seen = list(script), [], []

    def explore(self, workers, game_ids, moves, nsims):
        self.calls.append(("explore", list(workers), list(game_ids), list(moves), nsims))

    def step(self, replies=None, X=None, A=None, P=None, V=None):
        self.seen.append(None if replies is None else (replies.copy(), A.copy(), P.copy(), V.copy()))
        reqs, new = self.script.pop(0)
        return np.array(reqs, dtype=REQUEST_DTYPE), np.array(new, dtype=np.int32)

    def advance(self, workers, actions):
        self.calls.append(("advance", list(workers), list(actions)))

    def reset(self, workers):
        self.calls.append(("reset", list(workers)))

    def root_stats(self, workers):
        n = len(workers)
        N = np.tile(np.array([[3, 0, 1]], np.int32), (n, 1))
        return N, None, None, None, np.zeros(n, np.int32)


def test_host_stepped_env_keeps_states_by_worker_and_node_id():
    rules = Counting()
    script = [
        ([(0, -1, -1, ROOT), (1, -1, -1, ROOT)], []),                 # both workers ask for their root
        ([(0, 0, 2, PLAY), (1, 0, 0, PLAY)], [0, 0]),                 # roots became node 0; each asks for a move from it
        ([(0, 1, 0, PLAY), (1, 0, 2, FULL)], [1, 1]),                 # the children became node 1; worker 1 ran out of nodes
        ([(0, 1, 2, PLAY)], [0]),                                     # worker 0's reply was a transposition to node 0
        ([], [-1]),                                                   # terminal reply: no node; nobody asks any more
    ]
    tree = FakeTree(script)
    env = HostSteppedEnv(rules, tree, oracle=lambda s: (np.array([0.5, 0.0 if s % 2 else 0.25, 0.5 if s % 2 else 0.25], np.float32), np.float32(s / 10)))
    stopped = env.explore([0, 1], 5, game_ids=[4, 5], moves=[2, 2])
    assert stopped == {1: FULL} and not tree.script
    assert tree.calls == [("explore", [0, 1], [4, 5], [2, 2], 5)]
    # the questions were answered from the states kept by (worker, node id): worker 0 node 0 = 0 -> +3 = 3; worker 1 node 0 = 1 -> +1 = 2;
    # worker 0 node 1 = 3 -> +1 = 4; then node 1 again (the transposition did not overwrite node 0) -> +3 = 6, terminal
    assert rules.plays == [(0, 2), (1, 0), (3, 0), (3, 2)]
    assert env.states == {0: {0: 0, 1: 3}, 1: {0: 1, 1: 2}}
    assert tree.seen[0] is None
    rep, A, P, V = tree.seen[1]
    assert [tuple(k) for k in rep["key"]] == [(0, 1 << 63), (1, 1 << 63)] and list(rep["white_playing"]) == [1, 0] and list(rep["terminal"]) == [0, 0]
    assert A.tolist() == [[1, 1, 1], [1, 0, 1]] and P.dtype == np.float32 and V.tolist() == [np.float32(0.0), np.float32(0.1)]
    rep, A, P, V = tree.seen[4]
    assert list(rep["terminal"]) == [1] and list(rep["white_reward"]) == [1.0] and int(rep["key"][0][0]) == 6
    # policy over the available actions of the root, advance moves the host's root too, reset forgets the worker's states
    (acts, pi), = env.policy([1])
    assert acts == [0, 2] and pi.tolist() == [0.75, 0.25]
    env.advance([0], [2])
    assert env.roots[0] == 3 and tree.calls[-1] == ("advance", [0], [2])
    env.reset([0])
    assert env.states[0] == {} and env.states[1] == {0: 1, 1: 2} and tree.calls[-1] == ("reset", [0])
    assert HostTree.step.__doc__ and HostTree.root_stats.__doc__
