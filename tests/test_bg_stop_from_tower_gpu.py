"""The paired tower raises the background search's stop word itself (csrc/resnet16.h tower16x2_body, csrc/net_impl.h wave_net_f).

One slot group, free-running: a wave's background search (k_tree on the side stream, up to AZHIP_RUN_KBG simulations per slot) runs
under the wave's tower and leaves when the stop word reaches the wave's number.  The paired forms (k_tower16x2, k_tower16x2c and the
mixed k_tower16x2m) store it from their last round of workgroups, on the way into the head convolution; every other form keeps the
one-thread launch behind the tower.  When the word is raised decides only how far the background search gets, never what a game looks
like: with a tree per game (reset_every = 1) every record is the lock-step run's, whichever form serves the phase, and the phase ends.
That is all these tests can see: a word raised too early, too late or not at all changes the time a wave takes, not a record.  Who raises
it shows in a kernel trace (tools/trace_wave_handoffs.py: five launches per wave and no k_set_word where a paired form serves the phase,
profiles/r7/README.md)."""
import pytest

pytestmark = pytest.mark.gpu

SCHED = ((0, 6, 12), (1.0, 1.0, 0.3))
NET = dict(num_blocks=5, num_filters=64, num_policy_head_filters=32, num_value_head_filters=32)


def _by_id(games, moves, ng):
    out = {}
    for i in range(ng):
        g = games[i]
        out[g.game_id] = ((g.num_moves, g.nodes, tuple(g.final_key)), [bytes(moves[g.first_move + k]) for k in range(g.num_moves)])
    return out


def _run(game_name, slots, games, nsims, lock_step):
    import azhip
    from azhip.network import ResNetHP, random_params
    gh = {"c4": azhip.GAME_CONNECT_FOUR, "mancala": azhip.GAME_MANCALA}[game_name]
    with azhip.Engine(game=gh, oracle=azhip.ORACLE_RESNET, num_workers=slots, batch_size=slots, num_iters_per_turn=nsims, cpuct=2.0,
                      dirichlet_noise_eps=0.25, dirichlet_noise_alpha=1.0, temperature=SCHED, reset_every=1, seed=31, lock_step=lock_step,
                      max_moves_per_game=200 if game_name == "mancala" else 0, **NET) as e:
        e.net_set_params(random_params(gh, ResNetHP(**NET), seed=19))
        g, m, ng, nm, st = e.selfplay_run(games)                     # returns: the phase ended
        kernel = e.net_last_kernel()
    assert ng == games and st.aborted_games == 0 and st.games == games
    assert st.slot_launches > 0 and st.simulations == nsims * nm > 0
    return _by_id(g, m, ng), kernel


CASES = {"c4": (256, 1024, 32), "mancala": (512, 1024, 24)}          # slots, games (C4: four per slot), simulations per move


@pytest.fixture(scope="module")
def lock_step_records():
    cache = {}

    def get(monkeypatch, game_name):
        if game_name not in cache:
            monkeypatch.delenv("AZHIP_TOWER", raising=False)
            cache[game_name] = _run(game_name, *CASES[game_name], lock_step=1)[0]
        return cache[game_name]
    return get


@pytest.mark.parametrize("game_name,tower,kernel", [("c4", "21", "k_tower16x2<"), ("c4", "20", "k_tower16x2c<"), ("c4", "16", "k_tower16<"),
                                                    ("mancala", "21", "k_tower16x2<"), ("mancala", None, "k_tower")])
def test_records_do_not_depend_on_who_raises_the_stop_word(monkeypatch, lock_step_records, game_name, tower, kernel):
    want = lock_step_records(monkeypatch, game_name)
    monkeypatch.setenv("AZHIP_RUN_KBG", "32")
    if tower is None:
        monkeypatch.delenv("AZHIP_TOWER", raising=False)
    else:
        monkeypatch.setenv("AZHIP_TOWER", tower)
    got, seen = _run(game_name, *CASES[game_name], lock_step=0)
    assert seen.startswith(kernel), seen
    assert got == want
