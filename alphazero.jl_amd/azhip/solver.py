"""Solver mirror (games/connect-four/solver.jl): the perfect Connect-Four player.

The reference pipes positions to an external solver program; here the exact alpha-beta search runs on the device
(csrc/solver.hip; contract in include/azhip.h "Connect Four solver").  Scores follow Pascal Pons' convention: 0 a draw,
+k the player to move wins with his k-th stone counted from his last, -k the opponent does."""
import ctypes as C

import numpy as np

from . import _lib as L

NA, UNSOLVED = L.SOLVER_NA, L.SOLVER_UNSOLVED


def policy(q):
    """think()'s π from q-values by FULL action index (NA where unavailable): az_solver_policy, pure host"""
    q = np.ascontiguousarray(q, dtype=np.int8)
    pi = np.zeros(q.size, dtype=np.float64)
    L.check(L.lib().az_solver_policy(q.ctypes.data_as(C.c_void_p), q.size, pi.ctypes.data_as(C.c_void_p)))
    return pi


class Table:
    """The solver's transposition table (az_solver_table, include/azhip.h "Connect Four solver"): 2^log2_entries entries of 8 bytes
    in the memory of `device` (23: 64 MB).  It belongs to whoever made it: hand it to any c4_solve call, Player or Pons run of that
    device, strong or weak, and what one call learns the next one finds.  A context manager; close() frees it."""

    def __init__(self, log2_entries=23, device=0):
        h = C.c_void_p()
        L.check(L.lib().az_solver_table_create(int(device), int(log2_entries), C.byref(h)))
        self._h, self.log2_entries, self.device = h, int(log2_entries), int(device)

    def close(self):
        if getattr(self, "_h", None):
            L.lib().az_solver_table_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def clear(self):
        L.check(L.lib().az_solver_table_clear(self._h))

    def info(self):
        """dict(log2_entries, bytes, occupied); occupied is counted on the device by this call"""
        lg, nbytes, occ = C.c_int32(), C.c_int64(), C.c_int64()
        L.check(L.lib().az_solver_table_info(self._h, C.byref(lg), C.byref(nbytes), C.byref(occ)))
        return dict(log2_entries=lg.value, bytes=nbytes.value, occupied=occ.value)


class Player:
    """Solver.Player(), solver.jl:17-31; node_budget: nodes per (state, action) query, None = the library's default; table: a
    Table its searches share (None: the tableless search)"""

    def __init__(self, node_budget=None, table=None):
        self.node_budget, self.table = node_budget, table

    def _solve(self, game, weak=False):
        spec = game.spec()
        if spec.game_id != L.GAME_CONNECT_FOUR:
            raise TypeError("Solver.Player plays Connect Four, not %s" % spec.name)
        value, q, _ = spec._eng().c4_solve([game.current_state()], weak=weak, node_budget=self.node_budget, table=self.table)
        return int(value[0]), q[0]

    def value(self, game):
        """Solver.value (solver.jl:66-78); AzError if the position is not solved within the budget"""
        v, _ = self._solve(game)
        if v == UNSOLVED:
            raise L.AzError(L.AZ_ERR_CAPACITY, "the solver did not solve this position within its node budget")
        return v

    def qvalues(self, game):
        """available actions (1-based) and [qvalue(p, game, a) for a in them] (solver.jl:80-89, 93); UNSOLVED entries stay"""
        assert not game.game_terminated()
        _, q = self._solve(game)
        avail = q != NA
        return [int(a) + 1 for a in np.flatnonzero(avail)], q[avail].astype(np.int64)

    def think(self, game):
        """solver.jl:91-99: π uniform over the optimal actions"""
        assert not game.game_terminated()
        _, q = self._solve(game)
        if (q == UNSOLVED).any():
            raise L.AzError(L.AZ_ERR_CAPACITY, "the solver did not solve every move of this position within its node budget")
        avail = q != NA
        return [int(a) + 1 for a in np.flatnonzero(avail)], policy(q)[avail]

    def player_temperature(self, game, turn):
        return 1.0                                  # the default of AbstractPlayer (play.jl:36-38)

    def reset_player(self):
        pass
