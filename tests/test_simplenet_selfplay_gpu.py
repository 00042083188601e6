"""Self-play phases of SimpleNet engines, EVERY game against the oracle in replay mode (the scheme of tests/test_replay_all_games_gpu.py:
the oracle's trees consume the device network's P / V through az_net_evaluate_keys of the SAME engine, so the tree, the move step, the
RNG streams, the wave's network seam, the evaluation cache and the free-running schedule are what is compared; the network itself is
tests/test_simplenet_net_gpu.py's).
  * Tic-tac-toe with the shipped MCTS parameters (games/tictactoe/params.jl) but 64 simulations: 128 workers, 256 games, reset_every 4
    with the assignment the device reports, free-running and lock step, once with flip_probability 0.5;
  * Connect Four with width 100: 256 workers, 256 games, 64 simulations.
oracle_calls == leaf_evals; with the evaluation cache off, the same records (lock step: the same bytes as with it on)."""
import ctypes as C

import numpy as np
import pytest

import azhip
import azref as R
from azhip.network import SimpleNetHP, simple_random_params
from simplenet_ref import TTT_SHIPPED
from test_replay_all_games_gpu import _compare, _views

pytestmark = pytest.mark.gpu


def phase_vs_replay(name, game, hp, slots, nsims, num_games, reset_every, flip, lock_step, cpuct, eps, temp):
    blob = simple_random_params(game, hp, seed=2026)
    with azhip.Engine(game=game, simplenet=hp, num_workers=slots, batch_size=slots, num_iters_per_turn=nsims, gamma=1.0, cpuct=cpuct,
                      dirichlet_noise_eps=eps, dirichlet_noise_alpha=1.0, prior_temperature=1.0, temperature=temp,
                      reset_every=reset_every, flip_probability=flip, seed=1, lock_step=lock_step) as e:
        e.net_set_params(blob)
        games, moves, ng, nm, stats = e.selfplay_run(num_games)
        assert ng == num_games and stats.aborted_games == 0
        hg, hm = _views(games, moves, ng, nm)
        assert np.array_equal(hg["game_id"], np.arange(num_games))
        evaluator = (C.cast(azhip._lib.lib().az_net_evaluate_keys, C.c_void_p).value, e._h.value)
        one_per_slot = reset_every == 1 and num_games <= slots
        rg_, rm_, rnm, info = R.replay(game, evaluator, num_games, num_games if one_per_slot else slots, nsims,
                                       assignment=None if one_per_slot else hg["slot"].astype(np.int32), cpuct=cpuct, noise_eps=eps,
                                       noise_alpha=1.0, temp_xs=temp[0], temp_ys=temp[1], reset_every=reset_every, seed=1, flip_probability=flip)
        rg, rm = _views(rg_, rm_, num_games, rnm)
        _compare(hg, hm, rg, rm, name)
        assert info["oracle_calls"] == stats.leaf_evals, (info["oracle_calls"], stats.leaf_evals)
        assert stats.simulations == nsims * nm
        in_game_order = np.concatenate([np.arange(a, a + n) for a, n in zip(hg["first_move"], hg["num_moves"])])
        return hg.copy(), hm[in_game_order].copy(), int(stats.evals_reused)


TTT_KW = dict(game=R.TTT, hp=TTT_SHIPPED, slots=128, nsims=64, num_games=256, reset_every=4, cpuct=1.0, eps=0.2, temp=((0,), (1.0,)))


@pytest.mark.parametrize("lock_step,flip", [(0, 0.0), (1, 0.0), (0, 0.5)], ids=["free-running", "lock-step", "free-running-flips"])
def test_tictactoe_shipped_parameters(lock_step, flip, monkeypatch):
    on = phase_vs_replay("ttt cache on", flip=flip, lock_step=lock_step, **TTT_KW)
    assert on[2] > 0                                                 # the cache did answer part of the phase
    monkeypatch.setenv("AZHIP_EVAL_CACHE", "0")
    off = phase_vs_replay("ttt cache off", flip=flip, lock_step=lock_step, **TTT_KW)
    assert off[2] == 0
    if lock_step:                                                    # a fixed assignment: the two phases are the same bytes
        assert np.array_equal(on[0]["slot"], off[0]["slot"]) and np.array_equal(on[1], off[1])


def test_connect_four_width_100(monkeypatch):
    hp = SimpleNetHP(width=100, depth_common=4, use_batch_norm=True)
    kw = dict(game=R.C4, hp=hp, slots=256, nsims=64, num_games=256, reset_every=1, flip=0.0, lock_step=0, cpuct=2.0, eps=0.25,
              temp=((0, 20, 30), (1.0, 1.0, 0.3)))
    on = phase_vs_replay("c4 cache on", **kw)
    monkeypatch.setenv("AZHIP_EVAL_CACHE", "0")
    off = phase_vs_replay("c4 cache off", **kw)
    # reset_every 1: a game depends on its id alone, whatever the schedule
    assert np.array_equal(on[1], off[1]) and all(np.array_equal(on[0][f], off[0][f]) for f in ("game_id", "num_moves", "nodes", "final_key"))
