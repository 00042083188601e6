"""MCTS for games whose play! may be random, in Python Float64: the reference the chance mode of the device search trees
(AZ_HOST_TREE_CHANCE, include/azhip.h "chance") is held to.  No GPU, no library.

  Tree       one worker's MCTS.Env.tree: a dict by key, the scores and the backup in the operation order include/azhip.h states for
             the host trees (first maximum wins), the pools and max_depth as AZ_HT_FULL / AZ_HT_DEPTH define them
  RefSearch  run_simulation! / explore! / policy / reset! (src/mcts.jl:199-283) as one loop per simulation over any rules object:
             play is called at every ply, the statistics stay per (state, action), the backup runs along the states met
  RefTree    the same trees behind the HostTree method set (explore, step, root_stats, advance, reset, request_depths, stats), asking
             the questions the device asks, so HostSteppedEnv can run over it; chance=False remembers edges as the device does
and the small games and oracles the tests of both share."""
import math

import numpy as np

from azhip.host_tree import DEPTH, FULL, PLAY, REQUEST_DTYPE, ROOT

M64 = (1 << 64) - 1


def mix64(x):
    x = (x + 0x9e3779b97f4a7c15) & M64
    x = ((x ^ (x >> 30)) * 0xbf58476d1ce4e5b9) & M64
    x = ((x ^ (x >> 27)) * 0x94d049bb133111eb) & M64
    return x ^ (x >> 31)


class Node:
    __slots__ = ("key", "acts", "P", "W", "N", "vest", "wp", "memo")


class Tree:
    def __init__(self, gamma=1.0, cpuct=1.0, eps=0.0, max_nodes=1 << 30, max_edges=1 << 30, max_depth=1 << 30):
        self.gamma, self.cpuct, self.eps = float(gamma), float(cpuct), float(eps)
        self.max_nodes, self.max_edges, self.max_depth = max_nodes, max_edges, max_depth
        self.simulations = self.nodes_traversed = self.evaluations = self.transposition_hits = self.sims_without_host = 0
        self.max_nodes_seen = self.max_edges_seen = self.max_path = 0
        self.reset()

    def reset(self):
        """MCTS.reset!: the counters and high-water marks are kept"""
        self.nodes, self.index, self.nedges, self.root = [], {}, 0, -1

    def create(self, key, A, P, V, wp):
        """-> node id, or -1 where a pool is exhausted (nothing stored)"""
        acts = [a for a in range(len(A)) if A[a] != 0]
        if len(self.nodes) >= self.max_nodes or self.nedges + len(acts) > self.max_edges:
            return -1
        nd = Node()
        nd.key, nd.acts, nd.P = key, acts, [np.float32(P[a]) for a in acts]
        nd.W, nd.N, nd.memo = [0.0] * len(acts), [0] * len(acts), [None] * len(acts)
        nd.vest, nd.wp = np.float32(V), bool(wp)
        self.index[key] = len(self.nodes)
        self.nodes.append(nd)
        self.nedges += len(acts)
        self.max_nodes_seen, self.max_edges_seen = max(self.max_nodes_seen, len(self.nodes)), max(self.max_edges_seen, self.nedges)
        return len(self.nodes) - 1

    def select(self, nid, at_root, eta):
        """uct_scores + argmax (mcts.jl:180-188, 211): the rank of the first maximum"""
        nd = self.nodes[nid]
        s = math.sqrt(float(sum(nd.N)))
        best, rank = None, 0
        for i in range(len(nd.acts)):
            Q = nd.W[i] / float(max(nd.N[i], 1))
            Pd = float(nd.P[i])
            if at_root and self.eps != 0.0:
                Pd = (1.0 - self.eps) * Pd + self.eps * eta[i]
            score = Q + ((self.cpuct * Pd) * s) / float(nd.N[i] + 1)
            if best is None or score > best:
                best, rank = score, i
        return rank

    def backup(self, path, q, asked=True):
        """mcts.jl:216-223 over the path entries (node, rank, r, pswitch), last entry first; the simulation is complete"""
        for nid, rank, r, ps in reversed(path):
            qn = -q if ps else q
            q = r + self.gamma * qn
            nd = self.nodes[nid]
            nd.W[rank] += q
            nd.N[rank] += 1
        self.simulations += 1
        self.nodes_traversed += len(path)
        self.sims_without_host += 0 if asked else 1
        self.max_path = max(self.max_path, len(path))

    def meet(self, key, A, P, V, wp):
        """a non-terminal state was described: -> (node id or -1 when the pools are exhausted, created)"""
        self.evaluations += 1
        nid = self.index.get(key)
        if nid is not None:
            self.transposition_hits += 1
            return nid, False
        return self.create(key, A, P, V, wp), True

    def root_stats(self, num_actions):
        N, W, P = np.zeros(num_actions, np.int32), np.zeros(num_actions, np.float64), np.zeros(num_actions, np.float32)
        if self.root < 0:
            return N, W, P, np.float32(0), -1
        nd = self.nodes[self.root]
        N[nd.acts], W[nd.acts], P[nd.acts] = nd.N, nd.W, nd.P
        return N, W, P, nd.vest, self.root

    def counters(self):
        return dict(simulations=self.simulations, nodes_traversed=self.nodes_traversed, evaluations=self.evaluations,
                    transposition_hits=self.transposition_hits, sims_without_host=self.sims_without_host, max_nodes=self.max_nodes_seen,
                    max_edge_slots=self.max_edges_seen, max_path=self.max_path)


def entry_values(nd, wr, wp_after):
    """the mover's reward (Float64 of the Float32 given) and pswitch of a path entry that leaves node nd"""
    wr = float(np.float32(wr))
    return (wr if nd.wp else -wr), nd.wp != bool(wp_after)


class RefSearch(Tree):
    """MCTS.Env of one worker, driven directly: explore(root_state, nsims) runs run_simulation! on a clone of the game nsims times.
    rules: play / mask / key / reward / terminal / white_playing; oracle(state) -> (P by full action index, V)."""

    def __init__(self, rules, oracle, **kw):
        super().__init__(**kw)
        self.rules, self.oracle = rules, oracle

    def _meet(self, state):
        r = self.rules
        P, V = self.oracle(state)
        return self.meet(tuple(map(int, r.key(state))), np.asarray(r.mask(state), dtype=np.float32), P, V, r.white_playing(state))

    def advance(self):
        """the real move was played: where it led is not known until the next explore describes its root"""
        self.root = -1

    def explore(self, root_state, nsims, eta=None):
        """-> None, or FULL / DEPTH: that simulation is abandoned with nothing of it backed up, and the explore ends there"""
        for _ in range(nsims):
            stop = self._simulate(root_state, eta)
            if stop is not None:
                return stop
        return None

    def _simulate(self, state, eta):
        r, path = self.rules, []
        if self.root < 0:
            nid, new = self._meet(state)
            if nid < 0:
                return FULL
            self.root = nid
            if new:
                self.backup(path, float(self.nodes[nid].vest))
                return None
        nid = self.root
        while True:
            rank = self.select(nid, not path, eta)
            if len(path) >= self.max_depth:
                return DEPTH
            nd = self.nodes[nid]
            state = r.play(state, nd.acts[rank])
            path.append((nid, rank) + entry_values(nd, r.reward(state), r.white_playing(state)))
            if r.terminal(state):
                self.backup(path, 0.0)
                return None
            nid, new = self._meet(state)
            if nid < 0:
                return FULL
            if new:
                self.backup(path, float(self.nodes[nid].vest))
                return None

    def policy(self, num_actions):
        """MCTS.policy (mcts.jl:255-271) by full action index"""
        N = self.root_stats(num_actions)[0].astype(np.float64)
        return N / N.sum()


class _Worker:
    def __init__(self, tree):
        self.tree, self.cur, self.path, self.quota, self.pending, self.eta, self.touched = tree, -1, [], 0, None, None, False
        self.game = self.move = 0


class RefTree:
    """az_host_tree_* in host-oracle mode, on the CPU: per worker a Tree and the state machine of one step (absorb the reply, then
    back up / select until the host is needed or the quota is spent).  noise(game_id, move, n) -> eta, where eps != 0."""

    def __init__(self, num_actions, num_workers, nodes_per_worker, edge_slots_per_worker=None, max_depth=256, gamma=1.0, cpuct=1.0,
                 dirichlet_noise_eps=0.0, noise=None, chance=False):
        edges = nodes_per_worker * num_actions if edge_slots_per_worker is None else edge_slots_per_worker
        self.num_actions, self.num_workers, self.chance, self.noise = num_actions, num_workers, bool(chance), noise
        self.ws = [_Worker(Tree(gamma, cpuct, dirichlet_noise_eps, nodes_per_worker, edges, max_depth)) for _ in range(num_workers)]
        self.arms, self.outstanding, self.steps = [], [], 0

    def explore(self, workers, game_ids, moves, nsims):
        for w, g, m in zip(workers, game_ids, moves):
            s = self.ws[w]
            s.quota, s.game, s.move, s.eta, s.path, s.pending, s.touched, s.cur = int(nsims), int(g), int(m), None, [], None, False, s.tree.root
            self.arms.append(int(w))

    def step(self, replies=None, X=None, A=None, P=None, V=None):
        replies = [] if replies is None else replies
        assert len(replies) == len(self.outstanding), "%d replies for %d outstanding requests" % (len(replies), len(self.outstanding))
        active = sorted([(q[0], i) for i, (q, _) in enumerate(self.outstanding)] + [(w, -1) for w in self.arms])
        self.arms = []
        if not active:
            return np.zeros(0, dtype=REQUEST_DTYPE), np.zeros(0, dtype=np.int32)
        self.steps += 1
        reqs, new, self.outstanding = [], [-1] * len(replies), []
        for w, i in active:
            reply = None
            if i >= 0:
                rp = replies[i]
                term = bool(rp["terminal"])
                reply = (tuple(map(int, rp["key"])), rp["white_reward"], term, bool(rp["white_playing"]),
                         None if term else A[i], None if term else P[i], None if term else V[i])
            rq, depth, nn = self._run(w, reply)
            if i >= 0:
                new[i] = nn
            if rq is not None:
                reqs.append(rq)
                if rq[3] in (PLAY, ROOT):
                    self.outstanding.append((rq, depth))
        return np.array(reqs, dtype=REQUEST_DTYPE), np.array(new, dtype=np.int32)

    def _entry(self, s, wr, wp, child):
        nid, rank = s.path[-1][0], s.path[-1][1]
        nd = s.tree.nodes[nid]
        r, ps = entry_values(nd, wr, wp)
        s.path[-1] = (nid, rank, r, ps)
        if not self.chance:
            nd.memo[rank] = (child, r, ps)

    def _run(self, w, reply):
        s = self.ws[w]
        t = s.tree
        unwind = descending = False
        q, nn = 0.0, -1
        if reply is not None and s.pending is not None:
            key, wr, term, wp, Arow, Prow, V = reply
            pending, s.pending = s.pending, None
            if term:
                if pending == PLAY and s.path:
                    self._entry(s, wr, wp, -1)
                    q, unwind = 0.0, True
            else:
                nid, created = t.meet(key, Arow, Prow, V, wp)
                if nid < 0:                                              # AZ_HT_FULL
                    rq = (w, s.cur if pending == PLAY else -1, t.nodes[s.path[-1][0]].acts[s.path[-1][1]] if pending == PLAY and s.path else -1, FULL)
                    s.quota, s.path = 0, []
                    return rq, 0, -1
                nn = nid
                if pending == PLAY and s.path:
                    self._entry(s, wr, wp, nid)
                else:
                    t.root = nid
                if created:
                    q, unwind = float(t.nodes[nid].vest), True
                else:
                    s.cur, descending = nid, True
        while True:
            if unwind:
                t.backup(s.path, q, s.touched)
                s.quota -= 1
                s.path, unwind, descending = [], False, False
            if not descending:
                if s.quota <= 0:
                    s.quota = 0
                    return None, 0, nn
                s.touched, s.path = False, []
                if t.root < 0:
                    s.pending, s.touched = ROOT, True
                    return (w, -1, -1, ROOT), 0, nn
                s.cur, descending = t.root, True
            nd = t.nodes[s.cur]
            if not s.path and t.eps != 0.0 and s.eta is None:
                s.eta = self.noise(s.game, s.move, len(nd.acts))
            rank = t.select(s.cur, not s.path, s.eta)
            if len(s.path) >= t.max_depth:                               # AZ_HT_DEPTH
                s.quota, s.path = 0, []
                return (w, s.cur, nd.acts[rank], DEPTH), 0, nn
            s.path.append((s.cur, rank, 0.0, False))
            memo = None if self.chance else nd.memo[rank]
            if memo is None:
                s.pending, s.touched = PLAY, True
                return (w, s.cur, nd.acts[rank], PLAY), len(s.path) - 1, nn
            child, r, ps = memo
            s.path[-1] = (s.cur, rank, r, ps)
            if child < 0:
                q, unwind = 0.0, True
                continue
            s.cur = child

    def request_depths(self):
        return np.array([d for _, d in self.outstanding], dtype=np.int32)

    def root_stats(self, workers):
        rows = [self.ws[w].tree.root_stats(self.num_actions) for w in workers]
        return (np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]), np.stack([r[2] for r in rows]),
                np.array([r[3] for r in rows], np.float32), np.array([r[4] for r in rows], np.int32))

    def advance(self, workers, actions):
        for w, a in zip(workers, actions):
            t = self.ws[w].tree
            if t.root < 0:
                continue
            nd = t.nodes[t.root]
            assert a in nd.acts, "worker %d: its root has no action %d" % (w, a)
            memo = None if self.chance else nd.memo[nd.acts.index(a)]
            t.root = memo[0] if memo is not None and memo[0] >= 0 else -1
            self.ws[w].cur, self.ws[w].path = t.root, []

    def reset(self, workers):
        for w in workers:
            s = self.ws[w]
            s.tree.reset()
            s.cur, s.path, s.quota, s.pending, s.eta, s.touched = -1, [], 0, None, None, False

    def stats(self):
        out = dict(simulations=0, nodes_traversed=0, evaluations=0, transposition_hits=0, sims_without_host=0, max_nodes=0, max_edge_slots=0,
                   max_path=0, steps=self.steps)
        for s in self.ws:
            for k, v in s.tree.counters().items():
                out[k] = max(out[k], v) if k.startswith("max_") else out[k] + v
        return out


# ------------------------------------------------------------------------------------------------ rules and oracles of the tests
def philox(seed, worker):
    """the generator stream of one worker: device and reference each get their own copy of it"""
    return np.random.Generator(np.random.Philox(key=np.array([seed, worker], dtype=np.uint64)))


class PerWorker:
    """W rules objects, each with its own generator, behind one: a state is (worker, the state of that worker's rules), so the
    interleaving of the workers in a lock-step driver does not change which numbers a worker's play draws"""

    def __init__(self, rules):
        self.rules = list(rules)

    def root(self, w, state):
        return (w, state)

    def play(self, s, a):
        return (s[0], self.rules[s[0]].play(s[1], a))

    def mask(self, s):
        return self.rules[s[0]].mask(s[1])

    def key(self, s):
        return self.rules[s[0]].key(s[1])

    def reward(self, s):
        return self.rules[s[0]].reward(s[1])

    def terminal(self, s):
        return self.rules[s[0]].terminal(s[1])

    def white_playing(self, s):
        return self.rules[s[0]].white_playing(s[1])

    def planes(self, s):
        return self.rules[s[0]].planes(s[1])


def key_oracle(rules, num_actions):
    """a deterministic (P by full action index, V) from the key alone (and the mask, which the key determines): kept by key"""
    seen = {}

    def f(state):
        k0, k1 = map(int, rules.key(state))
        if (k0, k1) not in seen:
            h = mix64(k0 ^ mix64(k1))
            A = np.asarray(rules.mask(state), dtype=bool)
            raw = np.array([float((mix64(h + a + 1) >> 40) + 1) if A[a] else 0.0 for a in range(num_actions)])
            seen[(k0, k1)] = (raw / raw.sum()).astype(np.float32), np.float32((mix64(h ^ 0x5555) >> 11) / float(1 << 53) * 2.0 - 1.0)
        return seen[(k0, k1)]
    return f


class OneState:
    """one non-terminal state, one action: it stays with reward +1, stays with reward -1, or ends with reward 0.5.  A simulation
    walks the one edge again and again, each time with the reward it drew.  state = (alive, reward on arrival)"""

    def __init__(self, rng, p_end=0.15):
        self.rng, self.p_end = rng, p_end

    def play(self, s, a):
        u = self.rng.random()
        return (False, 0.5) if u < self.p_end else (True, 1.0 if u < self.p_end + (1.0 - self.p_end) / 2 else -1.0)

    def mask(self, s):
        return [True]

    def key(self, s):
        return (7 if s[0] else 8, 1)

    def reward(self, s):
        return s[1]

    def terminal(self, s):
        return not s[0]

    def white_playing(self, s):
        return True


class Slippery:
    """a pyref game whose move lands, with probability slip, on another of the available actions (two players: pswitch is true on
    every entry; one (state, action) is followed by terminal and non-terminal states in turn)"""

    def __init__(self, G, rng, slip=0.3):
        self.G, self.rng, self.slip = G, rng, slip

    def play(self, g, a):
        if self.rng.random() < self.slip:
            other = [b for b, ok in enumerate(self.G.mask(g)) if ok and b != a]
            if other:
                a = other[int(self.rng.integers(len(other)))]
        return self.G.play(g, a)

    def mask(self, g):
        return self.G.mask(g)

    def key(self, g):
        return self.G.key(g)

    def reward(self, g):
        return self.G.reward(g)

    def terminal(self, g):
        import pyref
        return pyref.finished(self.G, g)

    def white_playing(self, g):
        import pyref
        return pyref.white_playing(self.G, g)

    def planes(self, g):
        """Tic-tac-toe only: three planes of the 3 x 3 board -- empty, the mover's marks, the other's"""
        X = np.zeros((3, 3, 3), np.float32)
        for c, x in enumerate(g[0]):
            X[0 if x == 0 else 1 if x == g[1] else 2, c // 3, c % 3] = 1.0
        return X


class WideChance:
    """wide nodes with random outcomes: 100 actions, all legal at the root and a hash-chosen 1..100 of them elsewhere (two ranks per
    lane), over after 3 plies or earlier, rewards -1 / 0 / 1, the mover does not always change, few distinct successors.
    state = (h, ply, white to move, finished, white reward)"""
    A = 100

    def __init__(self, rng):
        self.rng, self._masks = rng, {}

    @staticmethod
    def root(n):
        return (mix64(5000 + n), 0, True, False, 0.0)

    def mask(self, s):
        h, ply = s[0], s[1]
        if (h, ply) not in self._masks:
            n = 100 if ply == 0 else 1 + mix64(h + 7) % 100
            order = sorted(range(100), key=lambda a: mix64(h ^ ((a + 1) * 0x9e3779b97f4a7c15 & M64)))
            legal = set(order[:n])
            self._masks[(h, ply)] = [a in legal for a in range(100)]
        return self._masks[(h, ply)]

    def play(self, s, a):
        h, ply, white = s[0], s[1], s[2]
        h2 = mix64((h + (a % 5) * 0x9e37 + int(self.rng.integers(3)) * 0x51ed + ply + 1) & M64) % 64
        fin = ply + 1 >= 3 or h2 % 7 == 0
        return (h2, ply + 1, white if h2 & 3 == 0 else not white, fin, float(h2 % 3 - 1) if fin else 0.0)

    def key(self, s):
        return (s[0], s[1] | ((not s[2]) << 63))

    def reward(self, s):
        return s[4]

    def terminal(self, s):
        return s[3]

    def white_playing(self, s):
        return s[2]


# ------------------------------------------------------------------------------------------------ comparing a tree with RefSearch
COUNTERS = ("simulations", "nodes_traversed", "evaluations", "transposition_hits", "sims_without_host", "max_nodes", "max_edge_slots", "max_path")


def assert_same(tree, refs, num_actions, workers=None):
    """tree (a HostTree or a RefTree) against one RefSearch per worker: N equal, W / P / Vest bit for bit at the roots of `workers`
    (default: all), and the counters, which the tree sums over all its workers"""
    workers = list(range(len(refs))) if workers is None else list(workers)
    N, W, P, Vest, root = tree.root_stats(workers)
    for i, w in enumerate(workers):
        rN, rW, rP, rV, rroot = refs[w].root_stats(num_actions)
        assert (root[i] >= 0) == (rroot >= 0), (w, root[i], rroot)
        assert np.array_equal(N[i], rN), (w, N[i], rN)
        assert np.array_equal(W[i].view(np.uint64), rW.view(np.uint64)), (w, W[i], rW)
        assert np.array_equal(P[i].view(np.uint32), rP.view(np.uint32)), (w, P[i], rP)
        assert np.float32(Vest[i]).view(np.uint32) == np.float32(rV).view(np.uint32), (w, Vest[i], rV)
    st = tree.stats()
    cs = [r.counters() for r in refs]
    for k in COUNTERS:
        want = max(c[k] for c in cs) if k.startswith("max_") else sum(c[k] for c in cs)
        assert st[k] == want, (k, st[k], want)
    return st


def play_episodes(env, refs, twin_rules, games, nsims, num_actions, max_moves, reset_after=None):
    """Whole episodes in lock step: explore, compare, play the most visited action (the first of them) with the rules' own
    randomness, advance.  env runs over the tree under test with its PerWorker rules, refs[w] over twin_rules (the same generator
    streams).  reset_after: the move after which every worker's tree is emptied once.  -> how often a root was found again by key
    with visits from earlier moves, which the tree under test must then show"""
    tree, W = env.tree, len(games)
    games, twins, found_again = list(games), list(games), 0
    alive = list(range(W))
    for move in range(max_moves):
        alive = [w for w in alive if not env.rules.terminal(games[w])]
        if not alive:
            break
        prior = {}
        for w in alive:
            nid = refs[w].index.get(tuple(map(int, twin_rules.key(twins[w]))))
            prior[w] = None if nid is None else sum(refs[w].nodes[nid].N)
        assert env.explore([games[w] for w in alive], nsims, workers=alive, game_ids=alive, moves=[move] * len(alive)) == {}
        for w in alive:
            assert refs[w].explore(twins[w], nsims) is None
        assert_same(tree, refs, num_actions, alive)
        N = tree.root_stats(alive)[0]
        for i, w in enumerate(alive):
            # every simulation but the one that creates the root leaves it once, and may come back to it and leave it again
            assert int(N[i].sum()) >= (nsims - 1 if prior[w] is None else prior[w] + nsims), (w, move, prior[w], N[i])
            found_again += bool(prior[w])
        acts = [int(np.argmax(N[i])) for i in range(len(alive))]
        env.advance(alive, acts)
        assert list(tree.root_stats(alive)[4]) == [-1] * len(alive)        # the device cannot know where the move led
        for w, a in zip(alive, acts):
            twins[w] = twin_rules.play(twins[w], a)
            refs[w].advance()
            games[w] = env.roots[w]
            assert games[w] == twins[w], (w, move)
        if move == reset_after:
            env.reset(alive)
            for w in alive:
                refs[w].reset()
    return found_again
