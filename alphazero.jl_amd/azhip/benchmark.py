"""Benchmark mirror (src/benchmark.jl): Duel / Single evaluations between standard players, on the device arena.

Players (benchmark.jl:124-192): Full(params) = MctsPlayer + the network, MctsRollouts(params) = MctsPlayer +
MCTS.RolloutOracle, NetworkOnly(τ) = PlayerWithTemperature(NetworkPlayer(nn), ConstSchedule(τ)), MinMaxTS(depth, amplify_rewards, τ) =
MinMax.Player (src/minmax.jl), whose exhaustive walk runs on the device too (azhip/minmax.py, csrc/minmax.hip).  Solver = the exact
Connect-Four player of games/connect-four/solver.jl (azhip/solver.py, csrc/solver.hip), for host-stepped games."""
import time
from dataclasses import dataclass

import numpy as np

from . import mcts as MCTS
from . import minmax as MinMax
from . import solver as SolverMod
from .arena import Evaluation, pit_players
from .network import copy as network_copy
from .params import ConstSchedule, MctsParams, SimParams
from .play import MctsPlayer, NetworkPlayer, PlayerWithTemperature, TwoPlayers


@dataclass
class Full:
    params: MctsParams
    name = "AlphaZero"

    def instantiate(self, gspec, nn):
        return MctsPlayer(gspec, nn, self.params)


@dataclass
class MctsRollouts:
    params: MctsParams

    @property
    def name(self):
        return "MCTS (%d rollouts)" % self.params.num_iters_per_turn

    def instantiate(self, gspec, nn):
        return MctsPlayer(gspec, MCTS.RolloutOracle(gspec), self.params)


@dataclass
class NetworkOnly:
    τ: float = 1.0
    name = "Network Only"

    def instantiate(self, gspec, nn):
        return PlayerWithTemperature(NetworkPlayer(nn), ConstSchedule(self.τ))


@dataclass
class MinMaxTS:
    """Benchmark.MinMaxTS(depth, amplify_rewards, τ=0.), benchmark.jl:179-194"""
    depth: int
    amplify_rewards: bool
    τ: float = 0.0

    @property
    def name(self):
        return "MinMax (depth %d)" % self.depth

    def instantiate(self, gspec, nn):
        return MinMax.Player(depth=self.depth, amplify_rewards=self.amplify_rewards, τ=self.τ)


@dataclass
class Solver:
    """The perfect Connect-Four player (Solver.Player, games/connect-four/solver.jl) as a player description: host-stepped play only
    (play.play_game, scripts of the Pons benchmark); the device arena does not seat it (include/azhip.h "Connect Four solver")."""
    node_budget: object = None
    table: object = None
    name = "Solver"

    def instantiate(self, gspec, nn):
        return SolverMod.Player(node_budget=self.node_budget, table=self.table)


@dataclass
class Duel:
    """Benchmark.Duel(player, baseline, sim), benchmark.jl:55-61"""
    player: object
    baseline: object
    sim: SimParams

    @property
    def name(self):
        return "%s / %s" % (self.player.name, self.baseline.name)


def run(gspec, bestnn, duel: Duel, gamma=1.0, progress=None, device=0, seed=1):
    """Benchmark.run(env, duel, progress) (benchmark.jl:78-99) -> Report.Evaluation; `gamma` is
    env.params.self_play.mcts.gamma and must equal the players' (the engine discounts with the contender's)."""
    nn = network_copy(bestnn, on_gpu=duel.sim.use_gpu, test_mode=True)
    players = TwoPlayers(duel.player.instantiate(gspec, nn), duel.baseline.instantiate(gspec, nn))
    t0 = time.perf_counter()
    rewards, red, _ = pit_players(gspec, players, duel.sim, progress, device, seed)
    return Evaluation(duel.name, float(np.mean(rewards)), red, rewards, None, time.perf_counter() - t0)


@dataclass
class TernaryOutcomeStatistics:
    """benchmark.jl:105-122"""
    num_won: int
    num_draw: int
    num_lost: int

    @staticmethod
    def of(rewards):
        r = np.asarray(rewards)
        return TernaryOutcomeStatistics(int((r > 0).sum()), int((r == 0).sum()), int((r < 0).sum()))
