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
