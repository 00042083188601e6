"""az_arena_run with SimpleNet engines:
  * two SimpleNet engines with the shipped Tic-tac-toe arena parameters (games/tictactoe/params.jl: 400 simulations, temperature 0.3,
    noise 0.1, flip_probability 0.5, alternating colours, reset_every 1) at 32 games: two runs give identical records;
  * a NetworkOnly player with a constant temperature of 0 plays, at every recorded state, the first argmax of the P that
    az_net_evaluate_keys gives for that state;
  * a SimpleNet engine against a 1x64 ResNet engine completes;
  * NetworkOnly against MinMaxTS(depth = 6) completes with rewards in [-1, 1]."""
import numpy as np
import pytest

import azhip
import azref as R
from azhip import Benchmark, MinMax
from azhip.arena import _engine, pit_players
from azhip.network import ResNet, ResNetHP, SimpleNet, SimpleNetHP
from azhip.params import ConstSchedule, MctsParams, SimParams
from azhip.play import MctsPlayer, NetworkPlayer, PlayerWithTemperature, TwoPlayers
from simplenet_ref import TTT_SHIPPED

pytestmark = pytest.mark.gpu

GSPEC = azhip.TicTacToeSpec()
ARENA_MCTS = MctsParams(num_iters_per_turn=400, cpuct=1.0, temperature=ConstSchedule(0.3), dirichlet_noise_ϵ=0.1, dirichlet_noise_α=1.0)
ARENA_SIM = SimParams(num_games=32, num_workers=100, batch_size=100, reset_every=1, flip_probability=0.5, alternate_colors=True)


def records(white, black, sim, seed=1):
    ec, eb = _engine(GSPEC, white, sim, 0, seed, "arena-white"), _engine(GSPEC, black, sim, 0, seed, "arena-black")
    games, moves, ng, nm, rewards, red = ec.arena_run(eb, sim.num_games, alternate_colors=sim.alternate_colors)
    assert ng == sim.num_games
    g = np.frombuffer(memoryview(games).cast("B"), dtype=np.uint8).reshape(-1, 56)[:ng].copy()
    m = np.frombuffer(memoryview(moves).cast("B"), dtype=np.uint8).reshape(-1, 64)[:nm].copy()
    return games, moves, g, m, rewards.copy()


def test_two_simplenets_shipped_arena_parameters_twice():
    a, b = SimpleNet(GSPEC, TTT_SHIPPED, seed=1), SimpleNet(GSPEC, TTT_SHIPPED, seed=2)
    players = (MctsPlayer(GSPEC, a, ARENA_MCTS), MctsPlayer(GSPEC, b, ARENA_MCTS))
    r1, r2 = records(*players, ARENA_SIM), records(*players, ARENA_SIM)
    assert np.array_equal(r1[2], r2[2]) and np.array_equal(r1[3], r2[3]) and np.array_equal(r1[4], r2[4])
    assert np.all(np.abs(r1[4]) <= 1.0) and len(r1[3]) >= 5 * 32


def test_network_only_at_temperature_zero_plays_the_first_argmax():
    nets = (SimpleNet(GSPEC, TTT_SHIPPED, seed=3), SimpleNet(GSPEC, SimpleNetHP(width=100, depth_common=4), seed=4))
    white, black = (PlayerWithTemperature(NetworkPlayer(n), ConstSchedule(0.0)) for n in nets)
    sim = SimParams(num_games=16, num_workers=16, batch_size=16, reset_every=1, flip_probability=0.0, alternate_colors=False)
    games, moves, g, m, rewards = records(white, black, sim)
    keys = np.array([list(moves[i].key) for i in range(len(m))], dtype=np.uint64)
    actions = np.array([moves[i].action for i in range(len(m))])
    by_white = np.array([R.Game(R.TTT, R.unpack_key(R.TTT, (int(k[0]), int(k[1])))).white_playing() for k in keys])
    assert by_white.any() and (~by_white).any()
    for net, mine in ((nets[0], by_white), (nets[1], ~by_white)):
        P, V = net._eng().net_evaluate_keys(keys[mine])
        assert np.array_equal(actions[mine], P.argmax(axis=1))       # numpy's argmax is the first one
        net.gc()


def test_simplenet_against_a_resnet():
    a = SimpleNet(GSPEC, TTT_SHIPPED, seed=5)
    b = ResNet(GSPEC, ResNetHP(num_blocks=1, num_filters=64, num_policy_head_filters=32, num_value_head_filters=32), seed=6)
    mcts = MctsParams(num_iters_per_turn=32, cpuct=1.0, temperature=ConstSchedule(0.3), dirichlet_noise_ϵ=0.1, dirichlet_noise_α=1.0)
    sim = SimParams(num_games=16, num_workers=16, batch_size=16, reset_every=1, flip_probability=0.5, alternate_colors=True)
    rewards, red, traces = pit_players(GSPEC, TwoPlayers(MctsPlayer(GSPEC, a, mcts), MctsPlayer(GSPEC, b, mcts)), sim)
    assert len(rewards) == 16 and np.all(np.isin(rewards, (-1.0, 0.0, 1.0))) and len(traces) == 16


def test_network_only_against_minmax():
    nn = SimpleNet(GSPEC, TTT_SHIPPED, seed=7)
    white = Benchmark.NetworkOnly().instantiate(GSPEC, nn)
    black = Benchmark.MinMaxTS(depth=6, amplify_rewards=True, τ=1.0).instantiate(GSPEC, nn)
    sim = SimParams(num_games=32, num_workers=32, batch_size=32, reset_every=1, flip_probability=0.5, alternate_colors=True)
    rewards, red, traces = pit_players(GSPEC, TwoPlayers(white, black), sim)
    assert len(rewards) == 32 and np.all((rewards >= -1.0) & (rewards <= 1.0))
