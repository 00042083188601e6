"""The step report of a free-running phase (csrc/tree.h StepReport, csrc/azhip.hip k_step_report / fr_round).

A look of the host at a free-running phase reads ONE record the device wrote behind the wave: the phase's words, the error word, the
sums of the statistics accumulators and the number of retired slots; it copies the finished games' records in one batch and fetches
the slots' `finished` words only when the report counts a retired slot.  None of that may show in what a phase returns: however the
same phase is cut into az_selfplay_step calls -- one wave per call (a look after every wave), three, 129 (a look inside the call, at
fr_round_waves = 128, and one at its end) or one long call -- the collected records are identical per game id and the counters agree.

What makes the four runs comparable: 64 slots are one wavefront of k_move_fr, so the id race is decided in lane order, and with
reset_every = 1 a game depends on its id alone.  The hash oracle's waves are one stream without a network launch; the ResNet runs
switch off what depends on the clock -- the evaluation cache (which looks hit depends on which wavefront filled an entry first, so
evals_reused is 0 here; the cross-check below covers its sum with the cache on) and, for a phase that is cut off after a fixed number
of waves, the background search (it runs until the tower has, so a wave's simulations depend on the clock; the bounded phase keeps it:
its totals do not depend on when a simulation ran).
An unbounded phase keeps finished games in a staging area of one game per slot that every look drains; slots wait when it is full,
and then the cuts would differ.  Its runs therefore play slowly (~400 waves per game: at most a third of the slots finish between two
looks 129 waves apart)."""
import pytest

pytestmark = pytest.mark.gpu

SCHED = ((0, 6, 12), (1.0, 1.0, 0.3))
COUNTERS = ("simulations", "leaf_evals", "evals_reused", "nodes_traversed", "moves", "games")
BIT = 0x40000000
WAVES = 774                                                          # = 6 x 129 = 258 x 3: every way of cutting runs exactly this many


def _by_id(games, moves, ng):
    out = {}
    for i in range(ng):
        g = games[i]
        out[g.game_id] = ((g.num_moves, g.nodes, tuple(g.final_key)), [bytes(moves[g.first_move + k]) for k in range(g.num_moves)])
    return out


def _engine(oracle, lock_step=0, nsims=48, **extra):
    import azhip
    from azhip.network import ResNetHP, random_params
    kw = dict(game=azhip.GAME_CONNECT_FOUR, num_workers=64, batch_size=64, num_iters_per_turn=nsims, cpuct=2.0, dirichlet_noise_eps=0.25,
              dirichlet_noise_alpha=1.0, temperature=SCHED, reset_every=1, seed=29, lock_step=lock_step)
    kw.update(extra)
    if oracle == "hash":
        return azhip.Engine(oracle=azhip.ORACLE_HASH, **kw)
    net = dict(num_blocks=1, num_filters=64, num_policy_head_filters=32, num_value_head_filters=32)
    e = azhip.Engine(oracle=azhip.ORACLE_RESNET, **net, **kw)
    e.net_set_params(random_params(azhip.GAME_CONNECT_FOUR, ResNetHP(**net), seed=7))
    return e


def _phase(e, num_games, per_call):
    """one phase in calls of `per_call` waves, collected after every call: records by id, final counters, aborted ids"""
    e.selfplay_begin(num_games, 0)
    got, n = {}, 0
    calls = WAVES // per_call if num_games < 0 else 10 ** 6
    for _ in range(calls):
        e.selfplay_step(per_call)
        games, moves, ng, nm = e.selfplay_collect(512)
        got.update(_by_id(games, moves, ng))
        n += ng
        if num_games > 0 and e.selfplay_active() == 0:
            break
    st = e.selfplay_stats()
    aborted = sorted(e.selfplay_aborted())
    e.selfplay_end()
    assert n == len(got)                                             # no game twice
    return got, {k: getattr(st, k) for k in COUNTERS}, aborted, st


@pytest.mark.parametrize("oracle", ["hash", "resnet"])
@pytest.mark.parametrize("num_games", [-1, 160])
def test_cutting_a_phase_into_calls_changes_nothing(monkeypatch, oracle, num_games):
    nsims = 48
    if oracle == "resnet":
        # (no cache here and none with the hash oracle: evals_reused is 0 in every run below, so ITS equality across the cuts is not
        # exercised -- with the cache on the counter depends on the clock; its sum is checked in the last test of this file)
        monkeypatch.setenv("AZHIP_EVAL_CACHE", "0")
    if num_games < 0:
        # ~16 waves per move: without an evaluation cache every new leaf waits for the oracle, so a wave completes about one
        # simulation per slot
        nsims = 16
        if oracle == "resnet":
            monkeypatch.setenv("AZHIP_RUN_KBG", "0")
    runs = {}
    with _engine(oracle, nsims=nsims) as e:
        for per_call in (1, 3, 129, WAVES if num_games < 0 else 10 ** 6):
            runs[per_call] = _phase(e, num_games, per_call)
    ref = runs[1]
    assert len(ref[0]) >= 32 and ref[1]["simulations"] > 0 and ref[2] == []
    if num_games > 0:
        assert sorted(ref[0]) == list(range(num_games)) and ref[1]["games"] == num_games
    for per_call, (got, cnt, aborted, _) in runs.items():
        assert got == ref[0], per_call
        assert cnt == ref[1], (per_call, cnt, ref[1])
        assert aborted == [], per_call
        assert cnt["games"] == len(got)


@pytest.mark.parametrize("oracle", ["hash", "resnet"])
def test_retired_slots_are_found_through_the_report(oracle):
    """A node pool too small for the largest games: slots retire inside k_tree, the report counts them, and only then does the host
    fetch the slots' `finished` words.  Aborted ids, replacement games and every completed game are the lock-step run's, however
    the phase is cut."""
    with _engine(oracle) as full:
        g0, m0, n0, _, _ = full.selfplay_run(160)
    cap = int(sorted(g0[i].nodes for i in range(n0))[-6])
    want = None
    for lock_step, per_call in ((1, 48), (0, 1), (0, 3), (0, 129), (0, 10 ** 6)):
        with _engine(oracle, lock_step=lock_step, max_nodes_per_slot=cap) as e:
            got, cnt, aborted, st = _phase(e, 160, per_call)
        assert st.aborted_games == len(aborted) >= 1, (lock_step, per_call)          # a retirement happened
        assert any(not a & BIT for a in aborted)
        given_up = [a for a in aborted if a & BIT]
        assert len(got) == 160 - len(given_up) == cnt["games"]
        replaced = {gid for gid in got if gid & BIT}
        assert replaced == {a | BIT for a in aborted if not a & BIT} - set(given_up)
        if want is None:
            want = (got, aborted)
        assert aborted == want[1], (lock_step, per_call)
        assert got == want[0], (lock_step, per_call)


def test_stats_come_from_the_report_and_are_never_stale():
    """Evaluation cache on.  az_selfplay_get_stats right after a step takes its sums from the report: twice in a row the same values,
    after a further step new ones, and after az_selfplay_end (which launches: the report no longer counts as fresh) the sums the host
    adds up from the accumulators themselves -- the same numbers."""
    with _engine("resnet") as e:
        e.selfplay_begin(-1, 0)
        e.selfplay_step(40)
        a, b = e.selfplay_stats(), e.selfplay_stats()
        keys = COUNTERS + ("waves", "slot_launches", "aborted_games")
        assert [getattr(a, k) for k in keys] == [getattr(b, k) for k in keys]
        assert a.simulations > 0 and a.evals_reused > 0 and a.waves == 40
        e.selfplay_step(40)
        c = e.selfplay_stats()
        assert c.simulations > a.simulations and c.leaf_evals > a.leaf_evals and c.nodes_traversed > a.nodes_traversed and c.waves == 80
        e.selfplay_end()
        d = e.selfplay_stats()
        assert [getattr(c, k) for k in keys] == [getattr(d, k) for k in keys]
