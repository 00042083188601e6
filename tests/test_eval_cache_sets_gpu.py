"""The evaluation cache's two-way sets (csrc/eval_cache_rule.h, csrc/tree.h k_tree) change no record.

A state hashes to a set of two entries that share one 128-byte line; a look reads both ways at once, the first way that answers wins,
and a state without an answer claims the way ec_pick_victim names.  AZHIP_EVAL_CACHE_LOG2=4 leaves 8 sets for 64 slots: every
insertion contends, every set holds a mixture of answered and claimed ways, answers are evicted all the time.  What must hold:
  * the records of a free-running ResNet phase are the same with the cache off, with 8 sets and at the default size -- with one slot
    group and with two, whose launches fill and evict side by side;
  * with the exact hash oracle behind the cache (AZHIP_EVAL_CACHE=1) the records are the oracle's direct run; Tic-tac-toe has 9
    actions, 16 lanes per slot, so the priors of the second way must come from the right lanes;
  * az_net_set_params leaves no answer of the old weights in either way;
  * evals_reused is alive: twice the sets answer at least as many oracle calls.
Phases are run once per configuration and shared by the tests."""
import functools
import os

import pytest

import azref as R

pytestmark = pytest.mark.gpu

SCHED = ((0, 6, 12), (1.0, 1.0, 0.3))
NET = dict(num_blocks=1, num_filters=64, num_policy_head_filters=32, num_value_head_filters=32)
KNOBS = ("AZHIP_EVAL_CACHE", "AZHIP_EVAL_CACHE_LOG2")


class _env:
    """the two creation-time overrides of the cache for the engines created inside; whatever was set before comes back"""
    def __init__(self, cache=None, log2=None):
        self.want = dict(zip(KNOBS, (cache, log2)))

    def __enter__(self):
        self.before = {k: os.environ.get(k) for k in KNOBS}
        for k, v in self.want.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = str(v)

    def __exit__(self, *exc):
        for k, v in self.before.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _recs(games, moves, ng):
    """records by game id, without the per-worker counters (they depend on which games the worker played before)"""
    out = {}
    for i in range(ng):
        g = games[i]
        out[g.game_id] = (g.num_moves, g.nodes, tuple(g.final_key), [bytes(moves[g.first_move + k]) for k in range(g.num_moves)])
    return out


@functools.lru_cache(maxsize=None)
def _resnet_phase(cache, log2, batch):
    """Connect-Four, 1 block x 64 filters, 64 workers, 32 simulations per move, 128 games, free-running"""
    import azhip
    from azhip.network import ResNetHP, random_params
    blob = random_params(azhip.GAME_CONNECT_FOUR, ResNetHP(**NET), seed=11)
    with _env(cache, log2):
        with azhip.Engine(game=azhip.GAME_CONNECT_FOUR, oracle=azhip.ORACLE_RESNET, num_workers=64, batch_size=batch, num_iters_per_turn=32,
                          cpuct=2.0, dirichlet_noise_eps=0.25, dirichlet_noise_alpha=1.0, temperature=SCHED, reset_every=1, seed=5,
                          lock_step=0, **NET) as e:
            e.net_set_params(blob)
            g, m, ng, nm, st = e.selfplay_run(128)
            assert ng == 128 and st.aborted_games == 0 and st.simulations == 32 * nm
            return _recs(g, m, ng), st.leaf_evals, st.evals_reused


def test_resnet_phase_one_slot_group_off_eight_sets_default():
    off, tiny, dflt = _resnet_phase(0, None, 64), _resnet_phase(None, 4, 64), _resnet_phase(None, None, 64)
    assert off[0] == tiny[0] == dflt[0]
    assert off[1] == tiny[1] == dflt[1]                             # the reference's count of oracle calls does not move
    assert off[2] == 0 and tiny[2] > 0 and dflt[2] > 0


def test_resnet_phase_two_slot_groups_fill_and_evict_side_by_side():
    off, tiny = _resnet_phase(0, None, 64), _resnet_phase(None, 4, 32)
    assert tiny[0] == off[0] and tiny[1] == off[1] and tiny[2] > 0


def test_two_ways_hold_two_states():
    """not a performance figure: the counter of answered oracle calls is alive and does not fall when the sets double"""
    tiny, twice = _resnet_phase(None, 4, 64), _resnet_phase(None, 5, 64)
    assert twice[0] == tiny[0]
    assert twice[2] >= tiny[2] > 0, (tiny[2], twice[2])


HASH_GAMES = {"ttt": (lambda A: A.GAME_TICTACTOE, R.TTT, 40, 1.0, 0), "mancala": (lambda A: A.GAME_MANCALA, R.MANCALA, 48, 0.0, 200)}


@functools.lru_cache(maxsize=None)
def _hash_reference(game_name):
    _, gr, nsims, flip, _ = HASH_GAMES[game_name]
    rg, rm, _ = R.simulate(gr, R.ORACLE_HASH, 128, 64, nsims, cpuct=2.0, noise_eps=0.25, noise_alpha=1.0, temp_xs=SCHED[0], temp_ys=SCHED[1],
                           reset_every=1, seed=3, flip_probability=flip)
    return _recs(rg, rm, 128)


@pytest.mark.parametrize("game_name,log2", [("ttt", 4), ("ttt", 10), ("mancala", 4), ("mancala", 10)])
def test_hash_oracle_behind_the_sets_equals_the_oracle(game_name, log2):
    import azhip
    gh, _, nsims, flip, max_moves = HASH_GAMES[game_name]
    with _env(1, log2):
        with azhip.Engine(game=gh(azhip), oracle=azhip.ORACLE_HASH, num_workers=64, batch_size=64, num_iters_per_turn=nsims, cpuct=2.0,
                          dirichlet_noise_eps=0.25, dirichlet_noise_alpha=1.0, temperature=SCHED, reset_every=1, flip_probability=flip, seed=3,
                          lock_step=0) as e:
            g, m, ng, nm, st = e.selfplay_run(128)
    assert ng == 128 and st.aborted_games == 0
    assert _recs(g, m, ng) == _hash_reference(game_name)
    assert 0 < st.evals_reused < st.leaf_evals


@pytest.mark.parametrize("log2", [4, None])
def test_new_parameters_leave_no_old_answer_in_either_way(log2):
    """a warm engine -- both ways of its sets answered or claimed under the old weights -- that gets new weights plays exactly the
    games a fresh engine with those weights plays"""
    import azhip
    from azhip.network import ResNetHP, random_params
    a, b = (random_params(azhip.GAME_CONNECT_FOUR, ResNetHP(**NET), seed=s) for s in (1, 2))
    kw = dict(game=azhip.GAME_CONNECT_FOUR, oracle=azhip.ORACLE_RESNET, num_workers=64, batch_size=64, num_iters_per_turn=32, cpuct=2.0,
              dirichlet_noise_eps=0.25, dirichlet_noise_alpha=1.0, temperature=SCHED, reset_every=1, seed=8, lock_step=0, **NET)
    with _env(None, log2):
        with azhip.Engine(**kw) as e:
            e.net_set_params(a)
            ga, ma, nga, _, sta = e.selfplay_run(64)
            first_a = _recs(ga, ma, nga)
            e.net_set_params(b)
            gb, mb, ngb, _, stb = e.selfplay_run(64)
            warm_b = _recs(gb, mb, ngb)
        with azhip.Engine(**kw) as e:
            e.net_set_params(b)
            g, m, ng, _, st = e.selfplay_run(64)
            fresh_b = _recs(g, m, ng)
    assert warm_b == fresh_b and warm_b != first_a
    assert sta.evals_reused > 0 and stb.evals_reused > 0 and st.evals_reused > 0 and stb.leaf_evals == st.leaf_evals
