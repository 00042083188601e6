"""MinMax mirror (src/minmax.jl): the stochastic minmax baseline player.

The exhaustive depth-limited walk runs on the device (csrc/minmax.hip; contract in include/azhip.h "MinMax player"):
`think` goes through az_minmax_qvalues for host-stepped games (play.play_game), and the device arena plays the same
player without leaving the device (arena._engine -> az_engine_set_minmax)."""
import ctypes as C

import numpy as np

from . import _lib as L


def policy(qs, τ=0.0):
    """think()'s π from the q-values of the available actions (minmax.jl:91-112): az_minmax_policy, pure host"""
    q = np.ascontiguousarray(qs, dtype=np.float64)
    pi = np.zeros_like(q)
    L.check(L.lib().az_minmax_policy(q.ctypes.data_as(C.c_void_p), q.size, float(τ), pi.ctypes.data_as(C.c_void_p)))
    return pi


class Player:
    """MinMax.Player(;depth, amplify_rewards, τ=0., γ=1.), minmax.jl:77-85"""

    def __init__(self, depth, amplify_rewards, τ=0.0, γ=1.0):
        self.depth, self.amplify_rewards, self.τ, self.gamma = int(depth), bool(amplify_rewards), float(τ), float(γ)

    def cfg(self):
        c = L.MinMaxCfg()
        L.check(L.lib().az_minmax_cfg_init(C.byref(c)))
        c.depth, c.amplify_rewards, c.tau, c.gamma = self.depth, int(self.amplify_rewards), self.τ, self.gamma
        return c

    def qvalues(self, game):
        """[qvalue(p, game, a, p.depth) for a in available_actions(game)] (minmax.jl:90) and think()'s π over them"""
        Q, pi = game.spec()._eng().minmax_qvalues(self.cfg(), [game.current_state()])
        avail = ~np.isnan(Q[0])
        return [a + 1 for a in np.flatnonzero(avail)], Q[0][avail], pi[0][avail]

    def think(self, game):
        actions, _, pi = self.qvalues(game)
        return actions, pi

    def player_temperature(self, game, turn):
        return 1.0                                  # the default of AbstractPlayer (play.jl:36-38)

    def reset_player(self):
        pass
