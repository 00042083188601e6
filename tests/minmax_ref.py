"""minmax_ref.py -- CPU reference of the MinMax baseline player (src/minmax.jl) for tests/test_minmax_*.py.

A pure-Python restatement over oracle/pyref.py's games, written from the reference sources (src/minmax.jl:14-114,
games/*/game.jl "Simple heuristic for minmax") and independent of csrc/minmax.h: Python floats are Float64 and every
arithmetic step below is one IEEE operation, so values compare bit for bit with the device.  exp / pow, the move stream and
the categorical draw are the C oracle's (libazref.so), as the contract in include/azhip.h names them.  Like every bit-exact
check of this project it pins the device to this restatement, not to a Julia run.
"""
import ctypes as C
import math
import random
import struct

import numpy as np

import azref as R
import pyref

INF = float("inf")
EPS = 2.220446049250313e-16          # eps(Float64)
GAMES = {R.C4: pyref.ConnectFour, R.TTT: pyref.TicTacToe, R.MANCALA: pyref.Mancala}


def _lib():
    L = R.lib()
    L.azr_apply_temperature.restype = None
    L.azr_apply_temperature.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_void_p]
    L.azr_stream_uniforms.restype = None
    L.azr_stream_uniforms.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p]
    return L


def bits(x):
    """the 64 bits of a Float64 (distinguishes -0.0 from 0.0, unlike ==)"""
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


# ---------------------------------------------------------------- heuristic_value
def _c4_alignments():
    """ALIGNMENTS of games/connect-four/game.jl:177-196 as cell lists (col, row 1-based), in its order"""
    out = []
    for dx, dy in ((1, 1), (1, -1), (0, 1), (1, 0)):
        for x in range(1, 8):
            for y in range(1, 7):
                al = [(x + i * dx, y + i * dy) for i in range(4)]
                if all(1 <= cx <= 7 and 1 <= cy <= 6 for cx, cy in al):
                    out.append(al)
    return out


C4_AL = _c4_alignments()
assert len(C4_AL) == 69
C4_AL_IDX = [tuple((cx - 1) + 7 * (cy - 1) for cx, cy in al) for al in C4_AL]                  # pyref board index col + 7*row
C4_AL_MASK = [sum(1 << ((cx - 1) * 7 + (cy - 1)) for cx, cy in al) for al in C4_AL]            # key bit col*7 + row
C4_POW = {3: (0.1 * 0.1) * 0.1, 2: 0.1 * 0.1, 1: 0.1, 0: 1.0, -1: 1.0 / 0.1}                    # 0.1 ^ k
TTT_POW = {2: 0.3 * 0.3, 1: 0.3, 0: 1.0, -1: 1.0 / 0.3}                                        # 0.3 ^ k
assert C4_POW[2] == 0.010000000000000002 and C4_POW[3] == 0.0010000000000000002


def _seq_sum(vals):
    s = None
    for v in vals:
        s = v if s is None else s + v
    return s


def _align_value_cells(board, idx, player, powers, top):
    n = 0
    for i in idx:
        c = board[i]
        if c == player:
            n += 1
        elif c != 0:
            return 0.0
    return powers[top - n]


def heuristic_cells(G, g):
    """GI.heuristic_value cell by cell, as the reference writes it (slow; the check of `heuristic`)"""
    if G is pyref.Mancala:
        v = g[2] - g[3]
        return float(-v if g[4] == 2 else v)
    als, powers, top = (C4_AL_IDX, C4_POW, 3) if G is pyref.ConnectFour else (pyref.TicTacToe.AL, TTT_POW, 2)
    cur = g[1]
    mine = _seq_sum(_align_value_cells(g[0], al, cur, powers, top) for al in als)
    yours = _seq_sum(_align_value_cells(g[0], al, 3 - cur, powers, top) for al in als)
    return mine - yours


def _c4_side(me, op):
    s = None
    for m in C4_AL_MASK:
        v = 0.0 if op & m else C4_POW[3 - bin(me & m).count("1")]
        s = v if s is None else s + v
    return s


_hcache = {}


def heuristic(G, g):
    """GI.heuristic_value(g); Connect Four on the packed key (same alignments, same order), memoised"""
    if G is not pyref.ConnectFour:
        return heuristic_cells(G, g)
    k = (g[0], g[1])
    h = _hcache.get(k)
    if h is None:
        a, b = G.key(g)
        a &= (1 << 63) - 1
        me, op = (a, b) if g[1] == 1 else (b, a)
        h = _hcache[k] = _c4_side(me, op) - _c4_side(op, me)
    return h


# ---------------------------------------------------------------- value / qvalue (minmax.jl:14-46)
def jl_max(a, b):
    """Julia's max on non-NaN Float64: -0.0 < 0.0"""
    sa, sb = math.copysign(1.0, a) < 0, math.copysign(1.0, b) < 0
    return b if (b > a) or (sb < sa) else a


_children = {}


def children(G, g):
    """[(action, next game, white_playing changed, white reward of next)] over the available actions, memoised"""
    k = (G, g)
    c = _children.get(k)
    if c is None:
        wp = pyref.white_playing(G, g)
        c = []
        for a, ok in enumerate(G.mask(g)):
            if ok:
                nx = G.play(g, a)
                c.append((a, nx, wp != pyref.white_playing(G, nx), G.reward(nx)))
        _children[k] = c
    return c


class MinMax:
    """MinMax.Player(depth, amplify_rewards, τ, γ) on one of pyref's games"""

    def __init__(self, game, depth, amplify_rewards, tau=0.0, gamma=1.0):
        self.game, self.G = game, GAMES[game]
        self.depth, self.amplify, self.tau, self.gamma = depth, amplify_rewards, tau, gamma
        self._memo = {}

    def value(self, g, depth):
        G = self.G
        if pyref.finished(G, g):
            return 0.0
        if depth == 0:
            return heuristic(G, g)
        k = (g, depth)
        v = self._memo.get(k)
        if v is None:
            v = None
            wp = pyref.white_playing(G, g)
            for a, nx, sw, wr in children(G, g):
                q = self._q(wp, nx, sw, wr, depth)
                v = q if v is None else jl_max(v, q)
            self._memo[k] = v
        return v

    def _q(self, wp, nx, switched, wr, depth):
        r = wr if wp else -wr
        if self.amplify and r != 0:
            r = math.copysign(INF, r)
        nextv = self.value(nx, depth - 1)
        if switched:
            nextv = -nextv
        return r + self.gamma * nextv

    def qvalues(self, g):
        """(available actions 0-based, [qvalue(p, g, a, p.depth)])"""
        wp = pyref.white_playing(self.G, g)
        ch = children(self.G, g)
        return [a for a, _, _, _ in ch], [self._q(wp, nx, sw, wr, self.depth) for _, nx, sw, wr in ch]

    def think(self, g):
        acts, qs = self.qvalues(g)
        return acts, qs, think_policy(qs, self.tau)


def think_policy(qs, tau):
    """think (minmax.jl:87-114): π over the available actions from their q-values"""
    L = _lib()
    n = len(qs)
    if any(q == INF for q in qs):
        pi = [1.0 if q == INF else 0.0 for q in qs]
    elif all(q == -INF for q in qs):
        pi = [1.0] * n
    else:
        qmax = qs[0]
        for q in qs[1:]:
            qmax = jl_max(qmax, q)
        if tau == 0:
            pi = [1.0 if q == qmax else 0.0 for q in qs]
        else:
            Cn = max(abs(q) for q in qs if q > -INF) + EPS
            pi = [0.0 if q == -INF else L.azr_exp((q - qmax) / Cn) for q in qs]
            pi = [L.azr_pow(p, 1 / tau) for p in pi]
    s = _seq_sum(pi)
    return [p / s for p in pi]


def select_move(pi, seed, game_id, move):
    """the default select_move (play.jl:48-53): temperature 1.0, fix_probvec + rand_categorical on the MOVE stream -> index"""
    L = _lib()
    p = np.ascontiguousarray(pi, dtype=np.float64)
    res = np.zeros_like(p)
    L.azr_apply_temperature(p.ctypes.data, len(p), 1.0, res.ctypes.data)
    u = L.azr_move_uniform(seed, game_id, move)
    return L.azr_rand_categorical(res.ctypes.data, len(res), u)


def flip_draw(seed, game_id, move, flip_probability, nsym):
    """play_game's per-turn flip (play.jl:305-307): index of the symmetry to apply, or None"""
    if flip_probability == 0.0:
        return None
    u64, u32 = np.zeros(2), np.zeros(2, np.float32)
    _lib().azr_stream_uniforms(seed, game_id, move, 3, 2, u64.ctypes.data, u32.ctypes.data)
    if u64[0] < flip_probability:
        return min(int(u64[1] * nsym), nsym - 1)
    return None


def f32_bits(x):
    return int(np.array([x], dtype=np.float64).astype(np.float32).view(np.int32)[0])


# ---------------------------------------------------------------- arena of two MinMax players (simulations.jl:207-244)
def arena(game, players, num_games, seed, alternate_colors, flip_probability, gamma=1.0, first_game_id=0):
    """TwoPlayers(players[0], players[1]) over num_games games: per game the move records
    (key before the flip, N[0..AMAX] as az_arena_run writes them, action, reward), the final key; rewards from players[0]'s
    side and the redundancy (rewards_and_redundancy, simulations.jl:296-311).  MinMax players keep no state, so a game
    depends on its id alone."""
    G = GAMES[game]
    games, rewards, states = [], [], []
    for i in range(num_games):
        gid = first_game_id + i
        flipped = alternate_colors and (i + 1) % 2 == 1
        g, recs = G.init(), []
        while not pyref.finished(G, g):
            key = G.key(g)
            k = flip_draw(seed, gid, len(recs), flip_probability, len(G.symmetries(g)) if hasattr(G, "symmetries") else 0)
            if k is not None:
                g = G.symmetries(g)[k]
            who = 0 if (pyref.white_playing(G, g) != flipped) else 1
            acts, qs, pi = players[who].think(g)
            N = [0] * (R.AMAX + 1)
            for a, p in zip(acts, pi):
                N[a] = f32_bits(p)
            N[R.AMAX] = 0x300 | (0 if k is None else k + 1)
            act = acts[select_move(pi, seed, gid, len(recs))]
            g = G.play(g, act)
            recs.append((key, N, act, G.reward(g)))
        wr, gp = 0.0, 1.0
        for _, _, _, r in recs:
            wr += gp * r
            gp *= gamma
        rewards.append(-wr if flipped else wr)
        states += [r[0] for r in recs] + [G.key(g)]
        games.append((recs, G.key(g)))
    return games, rewards, 1.0 - len(set(states)) / len(states)


# ---------------------------------------------------------------- the position sets
# per game: (seed, most random plies, depth at which the classes below are counted); chosen so that the set meets
# test_minmax_cpu.py::test_position_sets_cover_every_class -- a condition on this reference alone
POSITION_SETS = {R.C4: (11, 30, 3), R.TTT: (1, 7, 6), R.MANCALA: (13, 30, 4)}
NUM_POSITIONS = 64
_sets = {}


def positions(game):
    """64 non-terminal positions: the initial one, then states reached by 0..max random plies (fixed seed)"""
    if game not in _sets:
        seed, maxp, _ = POSITION_SETS[game]
        G = GAMES[game]
        rng = random.Random(seed * 1000 + game)
        out = [G.init()]
        while len(out) < NUM_POSITIONS:
            g = G.init()
            for _ in range(rng.randint(0, maxp)):
                acts = [a for a, ok in enumerate(G.mask(g)) if ok]
                g = G.play(g, rng.choice(acts))
                if pyref.finished(G, g):
                    break
            if not pyref.finished(G, g):
                out.append(g)
        _sets[game] = out
    return _sets[game]


def classify(qs):
    """which of the classes of think() a q-vector belongs to"""
    fin = [q for q in qs if abs(q) != INF]
    return {"win": any(q == INF for q in qs),
            "lost": all(q == -INF for q in qs),
            "partly_lost": any(q == -INF for q in qs) and not all(q == -INF for q in qs),
            "tie": bool(fin) and not any(q == INF for q in qs) and sum(1 for q in fin if q == max(fin)) > 1}


def keys_of(game, gs):
    return np.array([GAMES[game].key(g) for g in gs], dtype=np.uint64)
