"""GameInterface mirror (src/game.jl:34-336) over the device twins of alphazero.jl_amd/csrc/games.h.

States are the packed 16-byte keys of include/azhip.h (tuples of two Python ints); every rule
evaluation (play!, game_terminated, white_reward, actions_mask, vectorize_state) runs on the GPU
through az_game_play / az_game_encode, so the invariants of src/scripts/test_game.jl exercise the same
code the search kernels use."""
import numpy as np

from . import _lib as L
from .engine import Engine

BLACK_BIT = 1 << 63


class GameSpec:
    game_id = None
    name = None
    _engines = {}

    def _eng(self):
        e = GameSpec._engines.get(self.game_id)
        if e is None:
            e = Engine(game=self.game_id, oracle=L.ORACLE_UNIFORM, num_workers=1, batch_size=1, num_iters_per_turn=2)
            GameSpec._engines[self.game_id] = e
        return e

    # --- static properties (game.jl:34-75, 243-336) ---
    def two_players(self):
        return True

    def actions(self):
        return list(range(1, self.num_actions() + 1))     # 1-based like the reference

    def num_actions(self):
        return {L.GAME_CONNECT_FOUR: 7, L.GAME_TICTACTOE: 9, L.GAME_MANCALA: 6, L.GAME_GO9_PLANES: 82}[self.game_id]

    def state_dim(self):
        return {L.GAME_CONNECT_FOUR: (7, 6, 3), L.GAME_TICTACTOE: (3, 3, 3), L.GAME_MANCALA: (14, 1, 5), L.GAME_GO9_PLANES: (9, 9, 4)}[self.game_id]

    def init(self, state=None):
        return GameEnv(self, state)

    def vectorize_state(self, state):
        X, _ = self._eng().encode([state])
        w, h, c = self.state_dim()
        return np.transpose(X[0], (2, 1, 0)).copy()       # (W, H, C) like the Julia array

    def __eq__(self, other):
        return type(self) is type(other)

    def __hash__(self):
        return hash(type(self))


class ConnectFourSpec(GameSpec):
    game_id, name = L.GAME_CONNECT_FOUR, "connect-four"

    def symmetries(self, state):
        """games/connect-four/game.jl:247-257: column mirror, sigma = 7..1"""
        a, b = state

        def mirror(x):
            flag, x = x & BLACK_BIT, x & ~BLACK_BIT
            out = 0
            for c in range(7):
                out |= ((x >> (7 * c)) & 0x7f) << (7 * (6 - c))
            return out | flag
        return [((mirror(a), mirror(b)), list(range(7, 0, -1)))]


class TicTacToeSpec(GameSpec):
    game_id, name = L.GAME_TICTACTOE, "tictactoe"


class MancalaSpec(GameSpec):
    game_id, name = L.GAME_MANCALA, "mancala"


class Go9PlanesSpec(GameSpec):
    """The 9 x 9 x 4 plane geometry with 82 actions (BASELINE configs[4]: OpenSpiel 9x9 Go): geometry only.  The rules and the tree
    of such a game stay on the host, so there is no environment to create; ResNet(gspec, hp), TensorDataset and Trainer take it."""
    game_id, name = L.GAME_GO9_PLANES, "go9-planes"

    def init(self, state=None):
        raise NotImplementedError("Go9PlanesSpec carries the network geometry only: the game's rules run on the host")

    def vectorize_state(self, state):
        raise NotImplementedError("Go9PlanesSpec carries the network geometry only: the host encodes its own states")


class GridWorldRules:
    """games/grid-world/game.jl on the host, as the rules object HostSteppedEnv drives over chance trees (HostTree(chance=True)): a
    one-player MDP whose play is random.  A state is (x, y, time), 1-based like the reference; the key is built from (x, y) only,
    as the reference's state is -- time is the env's, which is why the host keeps an env per simulation.  The four actions
    r, l, u, d (game.jl:37) are always available and sit on the action indices 0..3 of whatever width is asked for.

    size (w, h); rewards {(x, y): reward}, every such cell terminal (default: the reference's four cells, which a 9 x 9 world holds
    too); slip: the probability that a move goes in a uniformly drawn direction instead (game.jl:45); the episode ends when
    time > episode_length_bound; rng: the numpy Generator play draws from -- the rules own it.  gspec: the network geometry planes
    and mask are written for (default: one plane of the world's size, four actions)."""
    MOVES = ((1, 0), (-1, 0), (0, 1), (0, -1))
    REWARDS = {(9, 3): 10.0, (8, 8): 3.0, (4, 3): -10.0, (4, 6): -5.0}
    KEY_TAG = 0x67726964776f726c                                      # "gridworl": the second key word

    def __init__(self, size=(10, 10), rewards=None, slip=0.4, episode_length_bound=200, rng=None, gspec=None):
        self.size = (int(size[0]), int(size[1]))
        self.rewards = dict(self.REWARDS if rewards is None else rewards)
        self.slip, self.episode_length_bound = float(slip), int(episode_length_bound)
        self.rng = np.random.default_rng() if rng is None else rng
        if gspec is None:
            self.num_actions, self.plane_shape = 4, (1, self.size[1], self.size[0])
        else:
            w, h, c = gspec.state_dim()
            self.num_actions, self.plane_shape = gspec.num_actions(), (c, h, w)
        if self.num_actions < 4 or self.plane_shape[1] < self.size[1] or self.plane_shape[2] < self.size[0]:
            raise ValueError("a %d x %d world does not fit the geometry %s with %d actions" % (self.size + (self.plane_shape, self.num_actions)))
        for (x, y) in self.rewards:
            if not (1 <= x <= self.size[0] and 1 <= y <= self.size[1]):
                raise ValueError("reward cell (%d, %d) outside the %d x %d world" % ((x, y) + self.size))

    def init(self):
        """RL.reset! (game.jl:36): a uniformly drawn cell, time 0"""
        return (int(self.rng.integers(1, self.size[0] + 1)), int(self.rng.integers(1, self.size[1] + 1)), 0)

    def play(self, state, action):
        """RL.act! (game.jl:43-51)"""
        x, y, time = state
        if not 0 <= action < 4:
            raise ValueError("action %r outside 0..3" % (action,))
        if self.rng.random() < self.slip:
            action = int(self.rng.integers(4))
        dx, dy = self.MOVES[action]
        return (min(max(x + dx, 1), self.size[0]), min(max(y + dy, 1), self.size[1]), time + 1)

    def mask(self, state):
        m = np.zeros(self.num_actions, dtype=bool)
        m[:4] = True
        return m

    def key(self, state):
        return (state[0] | (state[1] << 32), self.KEY_TAG)

    def reward(self, state):
        return self.rewards.get((state[0], state[1]), 0.0)

    def terminal(self, state):
        return (state[0], state[1]) in self.rewards or state[2] > self.episode_length_bound

    def white_playing(self, state):
        return True

    def planes(self, state):
        """GI.vectorize_state (game.jl:86-90): the one-hot position, in plane 0"""
        X = np.zeros(self.plane_shape, dtype=np.float32)
        X[0, state[1] - 1, state[0] - 1] = 1.0
        return X


SPECS = {"connect-four": ConnectFourSpec, "tictactoe": TicTacToeSpec, "mancala": MancalaSpec}


def spec_of_game_id(game_id):
    """the GameSpec of an az_game_id, the network-only geometry included"""
    for cls in (ConnectFourSpec, TicTacToeSpec, MancalaSpec, Go9PlanesSpec):
        if cls.game_id == game_id:
            return cls()
    raise ValueError("unknown game id %r" % (game_id,))


def _dihedral_src(k, p, n):
    """the cell whose content image k has at cell p = y * n + x of an n x n board: the 7 non-trivial dihedral maps in the reference's
    order (rot, rot2, rot3, flip, flip.rot, flip.rot2, flip.rot3; games/tictactoe/game.jl:149-168), rot(x, y) = (y, n-1-x),
    flip(x, y) = (x, n-1-y), 0-based -- TicTacToe::sym_src of csrc/games.h for any n"""
    x, y = p % n, p // n
    for _ in range(k + 1 if k < 3 else k - 3):
        x, y = y, n - 1 - x
    if k >= 3:
        y = n - 1 - y
    return y * n + x


def plane_symmetries(gspec):
    """GI.symmetries(gspec) as the gather tables PlaneMemoryBuffer.set_symmetries takes: (xperm (nsym, C*H*W), aperm (nsym, num_actions)),
    int32, with X'[w] = X[xperm[k][w]], A'[j] = A[aperm[k][j]], π'[j] = π[aperm[k][j]].

    They assume the encodings of this package: X is (C, H, W), word c*H*W + y*W + x is plane c at column x of row y, and every plane is
    a picture of the board (a symmetry moves all planes alike).
      Tic-tac-toe    the 7 non-trivial dihedral maps in the reference's order; action j is cell j = y*3 + x
      Connect Four   the column mirror x -> 6 - x; action a is column a, so a -> 6 - a
      Go9PlanesSpec  the same 7 maps on the cell p = y*9 + x of the 9 x 9 board; action p < 81 plays cell p and moves with it, the
                     pass action 81 is fixed.  A host whose planes or actions are indexed otherwise builds its own tables
      Mancala        none (the reference declares none): empty tables"""
    nA = gspec.num_actions()
    w, h, c = gspec.state_dim()
    gid = gspec.game_id
    if gid in (L.GAME_TICTACTOE, L.GAME_GO9_PLANES):
        cell = np.array([[_dihedral_src(k, p, w) for p in range(w * h)] for k in range(7)], dtype=np.int32)
        aperm = np.concatenate([cell, np.tile(np.arange(w * h, nA, dtype=np.int32), (7, 1))], axis=1)
    elif gid == L.GAME_CONNECT_FOUR:
        cell = np.array([[y * w + (w - 1 - x) for y in range(h) for x in range(w)]], dtype=np.int32)
        aperm = np.arange(nA - 1, -1, -1, dtype=np.int32)[None, :]
    else:
        return np.zeros((0, c * h * w), dtype=np.int32), np.zeros((0, nA), dtype=np.int32)
    xperm = np.concatenate([cell + k * w * h for k in range(c)], axis=1)
    return np.ascontiguousarray(xperm, dtype=np.int32), np.ascontiguousarray(aperm, dtype=np.int32)


class GameEnv:
    """AbstractGameEnv (game.jl:77-175)."""

    def __init__(self, spec, state=None):
        self._spec = spec
        if state is None:
            self._state = spec._eng().init_key()
            self._terminated, self._reward = False, 0.0
        else:
            self.set_state(state)

    def spec(self):
        return self._spec

    def set_state(self, state):
        state = (int(state[0]), int(state[1]))
        nxt, term, rew = self._spec._eng().play([state], [-1])
        self._state, self._terminated, self._reward = state, bool(term[0]), float(rew[0])

    def clone(self):
        g = GameEnv.__new__(GameEnv)
        g._spec, g._state, g._terminated, g._reward = self._spec, self._state, self._terminated, self._reward
        return g

    def current_state(self):
        return self._state

    def game_terminated(self):
        return self._terminated

    def white_playing(self):
        return not (self._state[0] & BLACK_BIT)

    def white_reward(self):
        return self._reward

    def heuristic_value(self):
        """GI.heuristic_value (the MinMax baseline's leaf value), on the device like the other rules"""
        return float(self._spec._eng().heuristic([self._state])[0])

    def actions_mask(self):
        _, A = self._spec._eng().encode([self._state])
        return A[0] > 0

    def available_actions(self):
        return [a for a, m in zip(self._spec.actions(), self.actions_mask()) if m]

    def play(self, action):
        """GI.play!(game, action) with a 1-based action like the reference."""
        nxt, term, rew = self._spec._eng().play([self._state], [int(action) - 1])
        self._state = (int(nxt[0][0]), int(nxt[0][1]))
        self._terminated, self._reward = bool(term[0]), float(rew[0])

    def vectorize_state(self):
        return self._spec.vectorize_state(self._state)

    def apply_random_symmetry(self, rng):
        """GI.apply_random_symmetry! (game.jl:329-336)."""
        syms = self._spec.symmetries(self._state) if hasattr(self._spec, "symmetries") else []
        assert syms, "no symmetries were declared for this game"
        symstate, _ = syms[int(rng.integers(len(syms)))]
        self.set_state(symstate)
