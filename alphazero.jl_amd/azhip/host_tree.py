"""Device search trees for a host-stepped game (include/azhip.h "device search trees", csrc/host_tree.hip).

HostTree is the thin mirror of az_host_tree_*: W per-worker MCTS trees (MCTS.Env, src/mcts.jl:124-226) in HBM that ask the host
one question per simulation at most.  HostSteppedEnv drives one for any rules object and keeps the host's share of the tree: the
game states, by (worker, node id) -- or, over chance trees (AZ_HOST_TREE_CHANCE: play may be random), one simulation env per worker."""
import ctypes as C

import numpy as np

from . import _lib

REPLY_DTYPE = np.dtype([("key", "<u8", 2), ("white_reward", "<f4"), ("terminal", "u1"), ("white_playing", "u1"), ("reserved", "u1", 2)])
REQUEST_DTYPE = np.dtype([("worker", "<i4"), ("node", "<i4"), ("action", "<i4"), ("kind", "<i4")])
assert REPLY_DTYPE.itemsize == C.sizeof(_lib.HostTreeReply) and REQUEST_DTYPE.itemsize == C.sizeof(_lib.HostTreeRequest)
PLAY, ROOT, FULL, DEPTH = _lib.HT_PLAY, _lib.HT_ROOT, _lib.HT_FULL, _lib.HT_DEPTH


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _arr(a, dtype, shape=None):
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=dtype)
    if shape is not None and a.shape != shape:
        raise ValueError("expected an array of shape %s, got %s" % (shape, a.shape))
    return a


class HostTree:
    """az_host_tree: engine = an azhip.Engine with the ResNet oracle and its parameters set (new states are evaluated by its network
    on the device), or None (the caller supplies P and V with every non-terminal reply).  chance: AZ_HOST_TREE_CHANCE, the trees of a
    game whose play may give another state each time -- no edge is remembered, every ply of every simulation asks."""

    def __init__(self, num_actions, num_workers, nodes_per_worker, edge_slots_per_worker=None, max_depth=256, engine=None, device=0,
                 gamma=1.0, cpuct=1.0, dirichlet_noise_eps=0.0, dirichlet_noise_alpha=1.0, prior_temperature=1.0, seed=0, chance=False):
        self._lib = _lib.lib()
        self.h = C.c_void_p()
        cfg = _lib.HostTreeCfg()
        _lib.check(self._lib.az_host_tree_cfg_init(C.byref(cfg)))
        cfg.gamma, cfg.cpuct, cfg.dirichlet_noise_eps, cfg.dirichlet_noise_alpha = gamma, cpuct, dirichlet_noise_eps, dirichlet_noise_alpha
        cfg.prior_temperature, cfg.seed = prior_temperature, seed
        cfg.flags = _lib.HOST_TREE_CHANCE if chance else 0
        self.chance = bool(chance)
        if edge_slots_per_worker is None:
            edge_slots_per_worker = nodes_per_worker * num_actions
        self.engine = engine                                          # keeps it alive: the tree launches on its stream
        self.num_actions, self.num_workers = num_actions, num_workers
        _lib.check(self._lib.az_host_tree_create(engine._h if engine is not None else None, device, num_actions, num_workers, nodes_per_worker,
                                                 edge_slots_per_worker, max_depth, C.byref(cfg), C.byref(self.h)))
        self._req = np.zeros(num_workers, dtype=REQUEST_DTYPE)
        self._new = np.zeros(num_workers, dtype=np.int32)
        self._dep = np.zeros(num_workers, dtype=np.int32)

    def close(self):
        if self.h:
            self._lib.az_host_tree_destroy(self.h)
            self.h = C.c_void_p()

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def explore(self, workers, game_ids, moves, nsims):
        w = _arr(workers, np.int32)
        g, m = _arr(game_ids, np.uint32, w.shape), _arr(moves, np.uint32, w.shape)
        _lib.check(self._lib.az_host_tree_explore(self.h, len(w), _vp(w), _vp(g), _vp(m), int(nsims)))

    def step(self, replies=None, X=None, A=None, P=None, V=None):
        """-> (requests [REQUEST_DTYPE], new_nodes [len(replies)]); X / A / P / V are indexed by reply"""
        replies = np.zeros(0, dtype=REPLY_DTYPE) if replies is None else np.ascontiguousarray(replies, dtype=REPLY_DTYPE)
        n = len(replies)
        A = _arr(A, np.float32, (n, self.num_actions))
        P = _arr(P, np.float32, (n, self.num_actions))
        V = _arr(V, np.float32, (n,))
        X = None if X is None else np.ascontiguousarray(X, dtype=np.float32)
        if X is not None and len(X) != n:
            raise ValueError("X has %d rows for %d replies" % (len(X), n))
        nreq = C.c_int32()
        _lib.check(self._lib.az_host_tree_step(self.h, n, _vp(replies), _vp(X), _vp(A), _vp(P), _vp(V), _vp(self._req), C.byref(nreq), _vp(self._new)))
        return self._req[:nreq.value].copy(), self._new[:n].copy()

    def request_depths(self):
        """-> the path length at which each PLAY / ROOT request of the last step was asked, in their order (0: the simulation starts)"""
        n = C.c_int32()
        _lib.check(self._lib.az_host_tree_request_depths(self.h, _vp(self._dep), len(self._dep), C.byref(n)))
        return self._dep[:n.value].copy()

    def root_stats(self, workers):
        """-> N [n][nA] int32, W float64, P float32 by full action index, Vest [n], root_node [n]"""
        w = _arr(workers, np.int32)
        n, nA = len(w), self.num_actions
        N, W, P = np.zeros((n, nA), np.int32), np.zeros((n, nA), np.float64), np.zeros((n, nA), np.float32)
        Vest, root = np.zeros(n, np.float32), np.zeros(n, np.int32)
        _lib.check(self._lib.az_host_tree_root_stats(self.h, n, _vp(w), _vp(N), _vp(W), _vp(P), _vp(Vest), _vp(root)))
        return N, W, P, Vest, root

    def advance(self, workers, actions):
        w = _arr(workers, np.int32)
        a = _arr(actions, np.int32, w.shape)
        _lib.check(self._lib.az_host_tree_advance(self.h, len(w), _vp(w), _vp(a)))

    def reset(self, workers):
        w = _arr(workers, np.int32)
        _lib.check(self._lib.az_host_tree_reset(self.h, len(w), _vp(w)))

    def stats(self):
        s = _lib.HostTreeStats()
        _lib.check(self._lib.az_host_tree_get_stats(self.h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in s._fields_}


class HostSteppedEnv:
    """MCTS.Env for a game whose rules the caller owns, over a HostTree (or anything with its methods).

    rules: play(state, action) -> state, mask(state) -> availability by action, key(state) -> (k0, k1), reward(state) -> white's
    reward on reaching the state, terminal(state), white_playing(state), and planes(state) -> the network's input (engine mode).
    oracle(state) -> (P by full action index, V): host-oracle mode only.  The host keeps what the device cannot: the states, by
    (worker, node id), and answers the tree's requests from them.

    Over chance trees (tree.chance) rules.play(state, action) may be random -- the rules own their generator -- and a state may carry
    more than its key tells (grid-world's time), so a node id does not name one.  The host then keeps one simulation env per worker:
    a request at depth 0 (tree.request_depths) starts from roots[w], any other goes on from where the last reply left the worker;
    request.node is only checked against that env's key.  advance plays the real move with the rules, the tree forgets its root."""

    def __init__(self, rules, tree, oracle=None):
        self.rules, self.tree, self.oracle = rules, tree, oracle
        self.chance = bool(getattr(tree, "chance", False))
        self.states = {}          # worker -> {node id: state}; chance: {node id: key}
        self.sims = {}            # chance: worker -> the env of its simulation in progress
        self.roots = {}           # worker -> the state its explore starts from
        self.stopped = {}         # worker -> FULL / DEPTH of its last explore

    def _describe(self, state, rows):
        r = self.rules
        rep = np.zeros(1, dtype=REPLY_DTYPE)[0]
        rep["key"] = np.array(r.key(state), dtype=np.uint64)
        rep["white_reward"] = r.reward(state)
        rep["terminal"] = bool(r.terminal(state))
        rep["white_playing"] = bool(r.white_playing(state))
        nA = self.tree.num_actions
        A, P, V, X = np.zeros(nA, np.float32), np.zeros(nA, np.float32), np.float32(0), None
        if not rep["terminal"]:
            A[:] = np.asarray(r.mask(state), dtype=np.float32)
            if self.oracle is not None:
                P[:], V = self.oracle(state)
            else:
                X = np.asarray(r.planes(state), dtype=np.float32)
        rows.append((rep, A, P, V, X))

    def explore(self, games, nsims, workers=None, game_ids=None, moves=None):
        """MCTS.explore!(env, game, nsims) for every worker, in lock step; -> {worker: FULL / DEPTH} for the workers that had to stop"""
        workers = list(range(len(games))) if workers is None else list(workers)
        n = len(workers)
        for w, g in zip(workers, games):
            self.roots[w] = g
            self.states.setdefault(w, {})
        self.tree.explore(workers, [0] * n if game_ids is None else game_ids, [0] * n if moves is None else moves, nsims)
        self.stopped = {}
        reqs, _ = self.tree.step()
        while True:
            rows, asked = [], []
            depths = iter(self.tree.request_depths()) if self.chance else None
            for q in reqs:
                w, kind = int(q["worker"]), int(q["kind"])
                if kind in (FULL, DEPTH):
                    self.stopped[w] = kind
                    continue
                if self.chance:
                    state = self._chance_reply(w, kind, int(q["node"]), int(q["action"]), int(next(depths)))
                else:
                    state = self.roots[w] if kind == ROOT else self.rules.play(self.states[w][int(q["node"])], int(q["action"]))
                self._describe(state, rows)
                asked.append((w, state))
            if not asked:
                return self.stopped
            replies = np.array([r[0] for r in rows], dtype=REPLY_DTYPE)
            A = np.stack([r[1] for r in rows])
            if self.oracle is not None:
                reqs, new = self.tree.step(replies, None, A, np.stack([r[2] for r in rows]), np.array([r[3] for r in rows], np.float32))
            else:
                shape = next((r[4].shape for r in rows if r[4] is not None), (0,))
                X = np.stack([r[4] if r[4] is not None else np.zeros(shape, np.float32) for r in rows])
                reqs, new = self.tree.step(replies, X, A)
            for (w, state), node in zip(asked, new):
                if node >= 0:
                    self.states[w].setdefault(int(node), tuple(map(int, self.rules.key(state))) if self.chance else state)

    def _chance_reply(self, w, kind, node, action, depth):
        """the state worker w's simulation reaches: its env is a copy of the root at depth 0 and plays on from there"""
        if kind == ROOT:
            state = self.roots[w]
        else:
            cur = self.roots[w] if depth == 0 else self.sims[w]
            if self.states[w].get(node) != tuple(map(int, self.rules.key(cur))):
                raise RuntimeError("worker %d: the tree asks about node %d, whose key is not that of the state its simulation stands in" % (w, node))
            state = self.rules.play(cur, action)
        self.sims[w] = state
        return state

    def policy(self, workers):
        """MCTS.policy (mcts.jl:255-271): per worker (available actions, pi = N / sum N)"""
        N, _, _, _, root = self.tree.root_stats(workers)
        out = []
        for i, w in enumerate(workers):
            if root[i] < 0:
                raise RuntimeError("MCTS.explore! must be called before MCTS.policy (worker %d)" % w)
            acts = [a for a, ok in enumerate(self.rules.mask(self.roots[w])) if ok]
            cnt = N[i, acts].astype(np.float64)
            out.append((acts, cnt / cnt.sum()))
        return out

    def advance(self, workers, actions):
        """the move is played: the root follows it, the tree is kept"""
        self.tree.advance(workers, actions)
        for w, a in zip(workers, actions):
            self.roots[w] = self.rules.play(self.roots[w], a)

    def reset(self, workers):
        """MCTS.reset!"""
        self.tree.reset(workers)
        for w in workers:
            self.states[w] = {}
