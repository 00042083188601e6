"""The mapped-on-demand node pool (csrc/azhip.hip vm_grow) under every caller and schedule.

A slot's tree lies in 2 MB chunks of 16 384 nodes that the host backs before the slot can reach them; a slot that outruns its chunks
meets a bounds test (tree.h k_tree: idx >= slot_cap), which RETIRES it in self-play (the game is aborted and replaced) and ends a hook's
or the arena's call with AZ_ERR_CAPACITY.  Neither may happen while memory is left: the pool must give the oracle's records -- and the
plain pool's -- whoever drives it.  tests/test_capacity_gpu.py holds it to the oracle with the evaluation cache off and a fresh tree per
game; here:
  A  a WARM evaluation cache on slots that own only their first chunk (a wave then adds up to run_k + 1 + fr_kbg nodes, not one),
     under five settings of the scheduling knobs;
  B  the provisioning rule itself, read through a seam (az_debug_slot_caps) after every look of the host;
  C  trees kept over several games (reset_every = 0 and 2): a slot grows through two and more chunk boundaries;
  D  the ResNet in the loop: the background search and the move step on their own streams beside the tower;
  E  the stepping form (az_selfplay_begin(-1) / step / collect);
  G  the arena on mapped pools, with and without the cache;
  H  a memory budget (AZHIP_POOL_GB) that runs out: slots retire, the completed games are still the oracle's.
(F, the hooks and the Mancala phase with the cache on, are variants of tests/test_capacity_gpu.py's cases and live there.)

Two facts shape the warm cases: a chunk is never unmapped during an engine's life, and an engine's evaluation cache survives from one
phase to the next.  A second phase on the same slots would find its chunks in place and prove nothing; so phase 1 plays ids 16-31 on
slots 0-15, and phase 2 replays them on slots 16-31 (reset_every = 1: a game depends on its id alone), which own one chunk each."""
import ctypes as C
import functools

import numpy as np
import pytest

import azref as R

pytestmark = pytest.mark.gpu

SCHED = ((0, 6, 12), (1.0, 1.0, 0.3))
CHUNK = 16384                                       # nodes of a 2 MB chunk (128-byte Connect-Four nodes)
CHUNK_BYTES = 2 << 20
BIT = 0x40000000                                    # AZ_REPLACEMENT_GAME_BIT
NSIMS = 800
CAP_A = NSIMS * 42                                  # az_engine_create's bound for reset_every = 1: simulations x plies of the longest game
WARM_ENV = {"AZHIP_VMM": "1", "AZHIP_EVAL_CACHE": "1", "AZHIP_EVAL_CACHE_LOG2": "24"}
KNOB_NAMES = ("AZHIP_RUN_K", "AZHIP_RUN_KBG", "AZHIP_FR_ROUND")
KNOBS = [None, (1, 32, 128), (64, 0, 7), (3, 200, 128), (3, 32, 1000)]   # None: the defaults (3, 32 | 8, 128)


def _by_id(games, moves, ng, cumulative=False):
    """records by game id; `cumulative`: with the per-worker counters (they depend on which games the worker played before)"""
    out = {}
    for i in range(ng):
        g = games[i]
        head = (g.num_moves, g.nodes, tuple(g.final_key)) + ((g.slot, g.total_simulations, g.total_nodes_traversed) if cumulative else ())
        out[g.game_id] = (head, [bytes(moves[g.first_move + k]) for k in range(g.num_moves)])
    return out


def _cfg_a(workers=32, batch=32, **kw):
    import azhip
    return dict(dict(game=azhip.GAME_CONNECT_FOUR, oracle=azhip.ORACLE_HASH, num_workers=workers, batch_size=batch, num_iters_per_turn=NSIMS,
                     cpuct=2.0, dirichlet_noise_eps=0.25, dirichlet_noise_alpha=1.0, temperature=SCHED, reset_every=1, seed=5), **kw)


def _setenv(mp, env, knobs=None):
    for k in KNOB_NAMES + ("AZHIP_POOL_GB", "AZHIP_EVAL_CACHE", "AZHIP_EVAL_CACHE_LOG2", "AZHIP_VMM"):
        mp.delenv(k, raising=False)
    for k, v in env.items():
        mp.setenv(k, v)
    for k, v in zip(KNOB_NAMES, knobs or ()):
        mp.setenv(k, str(v))


@functools.lru_cache(maxsize=None)
def _oracle_a():
    """the oracle's 32 games of case A's configuration (a game depends on its id alone: whatever the workers, the phase, the slot)"""
    g, m, nm = R.simulate(R.C4, R.ORACLE_HASH, 32, 32, NSIMS, cpuct=2.0, noise_eps=0.25, noise_alpha=1.0, temp_xs=SCHED[0], temp_ys=SCHED[1],
                          reset_every=1, seed=5)
    return _by_id(g, m, 32), nm


@functools.lru_cache(maxsize=None)
def _cold_a():
    """a COLD engine's selfplay_run(32) on a mapped pool with the cache forced on: (records, stats)"""
    import azhip
    with pytest.MonkeyPatch.context() as mp:
        _setenv(mp, WARM_ENV)
        with azhip.Engine(**_cfg_a()) as e:
            g, m, ng, nm, st = e.selfplay_run(32)
            return _by_id(g, m, ng), (ng, st.aborted_games, st.leaf_evals, st.evals_reused)


def _slot_caps(e):
    """(node_count[G], slot_cap[G]) as of now: the device's node counts and the host's table of backed nodes (az_debug_slot_caps)"""
    from azhip import _lib as L
    f = L.lib().az_debug_slot_caps
    f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]
    G = e.cfg.num_workers
    nc, sc = np.zeros(G, dtype=np.int32), np.zeros(G, dtype=np.int32)
    L.check(f(e._h, nc.ctypes.data_as(C.c_void_p), sc.ctypes.data_as(C.c_void_p)))
    return nc, sc


def _ahead(batch, workers, knobs, cache=True, waves=None):
    """DESIGN 3b's rule for a free-running phase.  Per wave a slot adds at most run_k + 1 nodes in the wave's launch (the pending leaf and
    run_k answers of the cache) and fr_kbg in the background launch (32 with one slot group, 8 with several, unless AZHIP_RUN_KBG says
    otherwise); without a cache the pending leaf's node alone.  The host looks at the node counts every AZHIP_FR_ROUND waves, and on a
    mapped pool at least as often as it takes a slot to add an eighth of a chunk (2048 nodes).  ahead = waves between two looks x nodes
    per wave + 2, capped at the slot's bound.  `waves`: the same bound over that many waves instead."""
    k, kbg, rnd = knobs or (3, 32 if workers // batch == 1 else 8, 128)
    per_wave = (k + 1 + kbg) if cache else 1
    look = max(1, min(rnd, (CHUNK // 8) // per_wave))
    return min((waves or look) * per_wave + 2, CAP_A)


def _warm(e):
    """phase 1: slots 0-15 play ids 16-31 and fill the cache; slots 16-31 keep their first chunk"""
    g, m, ng, nm, st = e.selfplay_run(16, first_game_id=16)
    return _by_id(g, m, ng), ng, st


# ------------------------------------------------------------------------------------------------------------------ A
@pytest.mark.parametrize("knobs", KNOBS, ids=lambda k: "default" if k is None else "k%d_kbg%d_round%d" % k)
@pytest.mark.parametrize("batch", [32, 16])
def test_a_warm_cache_on_slots_that_own_one_chunk(monkeypatch, batch, knobs):
    """Nearly every leaf of ids 16-31 is a hit in phase 2: their slots take ~23 waves per move instead of 800 and cross node 16 384
    between two looks of the host.  Nobody may be retired for that, and every record is the oracle's.
    The 0.4 share of reused evaluations is the case's premise, not a tolerance: ids 16-31 make 505 of the oracle's 987 moves and are
    replayed warm; 2^24 direct-mapped entries for ~600 k distinct states evict a few percent."""
    import azhip
    want, _ = _oracle_a()
    _setenv(monkeypatch, WARM_ENV, knobs)
    with azhip.Engine(**_cfg_a(batch=batch)) as e:
        rec1, ng1, st1 = _warm(e)
        g, m, ng, nm, st = e.selfplay_run(32)
        aborted = e.selfplay_aborted()
        rec2 = _by_id(g, m, ng)
        held = e.device_bytes()
    big = sum(1 for i in range(16, 32) if i in rec2 and rec2[i][0][1] > CHUNK)
    print("case A batch=%d knobs=%s: phase 1 ng=%d aborted=%d; phase 2 ng=%d aborted=%d %s leaf_evals=%d reused=%d, ids 16-31 above %d nodes: %d, "
          "device_bytes=%d" % (batch, knobs, ng1, st1.aborted_games, ng, st.aborted_games, aborted, st.leaf_evals, st.evals_reused, CHUNK, big, held))
    assert ng1 == 16 and st1.aborted_games == 0
    assert ng == 32 and st.aborted_games == 0, aborted
    assert rec1 == {i: want[i] for i in range(16, 32)}
    assert rec2 == want
    cold_rec, (cold_ng, cold_aborted, cold_evals, _) = _cold_a()
    assert cold_ng == 32 and cold_aborted == 0 and cold_rec == want
    assert st.leaf_evals == cold_evals                               # the reference's count of oracle calls: the cache does not move it
    assert st.evals_reused > 0.4 * st.leaf_evals
    assert big >= 10                                                 # (the oracle: 13 of ids 16-31 end above 16 384 nodes)


# ------------------------------------------------------------------------------------------------------------------ B
@pytest.mark.parametrize("knobs", [None, (3, 200, 128)], ids=lambda k: "default" if k is None else "k%d_kbg%d_round%d" % k)
def test_b_every_slot_is_provisioned_for_what_it_can_add_before_the_next_look(monkeypatch, knobs):
    """The rule case A depends on, read directly: after az_selfplay_begin and after every az_selfplay_step of 128 waves (each ends with a
    look of the host) every slot has node_count <= slot_cap and slot_cap >= min(node_count + ahead, cap_nodes), `ahead` the documented
    worst-case growth until the next look (_ahead); and no slot's count grew by more than the same rule gives for the 128 waves since the
    last read -- the premise, checked against the device.  Defaults: 36 nodes per wave, a look every 56 waves, ahead = 2018;
    (3, 200, 128): 204 per wave, a look every 10 waves, ahead = 2042, up to 26 114 nodes in 128 waves."""
    import azhip
    want, _ = _oracle_a()
    ahead, per_step = _ahead(32, 32, knobs), _ahead(32, 32, knobs, waves=128)
    _setenv(monkeypatch, WARM_ENV, knobs)
    worst_growth, short, over, steps = 0, [], [], 0
    with azhip.Engine(**_cfg_a()) as e:
        _warm(e)
        e.selfplay_begin(32, 0)
        nc0, sc = _slot_caps(e)
        while True:
            over += [(steps, s, int(nc0[s]), int(sc[s])) for s in range(32) if nc0[s] > sc[s]]
            short += [(steps, s, int(nc0[s]), int(sc[s])) for s in range(32) if sc[s] < min(int(nc0[s]) + ahead, CAP_A)]
            if e.selfplay_active() == 0 or steps >= 4000:
                break
            e.selfplay_step(128)
            steps += 1
            nc, sc = _slot_caps(e)
            worst_growth = max(worst_growth, int((nc - nc0).max()))
            nc0 = nc
        games, moves, ng, nm = e.selfplay_collect(64)
        st = e.selfplay_stats()
        e.selfplay_end()
    print("case B knobs=%s: ahead=%d, %d steps, largest growth between two reads %d (bound %d), reads with slot_cap short of the rule %d (first %s), "
          "ng=%d aborted=%d" % (knobs, ahead, steps, worst_growth, per_step, len(short), short[:3], ng, st.aborted_games))
    assert steps < 4000
    assert not over, over[:5]
    assert worst_growth <= per_step
    assert not short, short[:5]
    assert ng == 32 and st.aborted_games == 0 and _by_id(games, moves, ng) == want


# ------------------------------------------------------------------------------------------------------------------ C
@pytest.mark.parametrize("reset_every,nsims,games,batch", [(0, 300, 64, 8), (0, 300, 64, 4), (2, NSIMS, 32, 8), (2, NSIMS, 32, 4)])
def test_c_trees_kept_over_several_games_grow_through_chunk_boundaries(monkeypatch, reset_every, nsims, games, batch):
    """reset_every = 0: eight games on one tree, every slot ends at 38-50 k nodes under the oracle's default assignment -- two chunk
    boundaries; the node count is NOT reset at a game's start, where a warm cache answers most.  reset_every = 2 with 800 simulations:
    the oracle has 27 of 32 games above 16 384 nodes and 7 above 32 768.  The records, per-worker counters included, are the oracle's
    for the worker -> game assignment the device reports."""
    import azhip
    _setenv(monkeypatch, WARM_ENV)
    kw = _cfg_a(workers=8, batch=batch, num_iters_per_turn=nsims, reset_every=reset_every, flip_probability=0.5,
                max_nodes_per_slot=300 * 42 * 8 if reset_every == 0 else 0)
    with azhip.Engine(**kw) as e:
        g, m, ng, nm, st = e.selfplay_run(games)
        aborted = e.selfplay_aborted()
        dev = _by_id(g, m, ng, cumulative=True)
    slot_nodes = [max([g[i].nodes for i in range(ng) if g[i].slot == s] or [0]) for s in range(8)]   # a tree that is never reset only grows
    game_nodes = [dev[i][0][1] for i in sorted(dev)]
    print("case C reset_every=%d batch=%d: ng=%d aborted=%d %s, slots' nodes %s, games above 16384: %d, above 32768: %d"
          % (reset_every, batch, ng, st.aborted_games, aborted, slot_nodes, sum(n > CHUNK for n in game_nodes), sum(n > 2 * CHUNK for n in game_nodes)))
    assert ng == games and st.aborted_games == 0, aborted
    asg = R.assignment_of(g, games)                                 # the outcome of the id race this phase took (util.jl:181-188)
    rg, rm, rnm = R.simulate(R.C4, R.ORACLE_HASH, games, 8, nsims, cpuct=2.0, noise_eps=0.25, noise_alpha=1.0, temp_xs=SCHED[0], temp_ys=SCHED[1],
                             reset_every=reset_every, seed=5, flip_probability=0.5, assignment=asg)
    assert rnm == nm and dev == _by_id(rg, rm, games, cumulative=True)
    if reset_every == 0:
        assert sum(n > 2 * CHUNK for n in slot_nodes) >= 4          # at least half the slots grew through two chunk boundaries
    else:
        # (conditions that keep the case meaningful; the oracle's default assignment gives 27 and 7)
        assert sum(n > CHUNK for n in game_nodes) >= 16 and sum(n > 2 * CHUNK for n in game_nodes) >= 1


# ------------------------------------------------------------------------------------------------------------------ D
def test_d_resnet_in_the_loop_side_streams_on_a_mapped_pool(monkeypatch):
    """One slot group and the ResNet oracle: the background launch and the move step run on their own streams beside the tower
    (wave_group, `side`), the cache is on by default.  Warm slots with one chunk again; the records are those of a plain pool in lock step."""
    import azhip
    from azhip.network import ResNetHP, random_params
    net = dict(num_blocks=1, num_filters=64, num_policy_head_filters=32, num_value_head_filters=32)
    blob = random_params(azhip.GAME_CONNECT_FOUR, ResNetHP(**net), seed=7)
    kw = _cfg_a(oracle=azhip.ORACLE_RESNET, **net)
    _setenv(monkeypatch, {"AZHIP_VMM": "1"})
    with azhip.Engine(**kw) as e:
        e.net_set_params(blob)
        rec1, ng1, st1 = _warm(e)
        g, m, ng, nm, st = e.selfplay_run(32)
        aborted = e.selfplay_aborted()
        rec2 = _by_id(g, m, ng)
    _setenv(monkeypatch, {"AZHIP_VMM": "0"})
    with azhip.Engine(**dict(kw, lock_step=1)) as e:
        e.net_set_params(blob)
        g, m, n0, _, st0 = e.selfplay_run(32)
        want = _by_id(g, m, n0)
    big = sum(1 for r in rec2.values() if r[0][1] > CHUNK)
    print("case D: phase 1 ng=%d aborted=%d; phase 2 ng=%d aborted=%d %s reused=%d of %d, games above %d nodes: %d"
          % (ng1, st1.aborted_games, ng, st.aborted_games, aborted, st.evals_reused, st.leaf_evals, CHUNK, big))
    assert n0 == 32 and st0.aborted_games == 0
    assert ng1 == 16 and st1.aborted_games == 0 and ng == 32 and st.aborted_games == 0, aborted
    assert rec1 == {i: want[i] for i in range(16, 32)} and rec2 == want
    assert st.leaf_evals == st0.leaf_evals and st.evals_reused > 0
    assert big >= 1


# ------------------------------------------------------------------------------------------------------------------ E
def test_e_stepping_form_on_a_warm_cache(monkeypatch):
    """az_selfplay_begin(-1) / step(300) / collect: the host looks every 128 waves and at the end of every step.  1800 waves are enough
    for the warm slots 16-31 (ids 16-31) only: those sixteen games must come back, each the oracle's game of its id."""
    import azhip
    want, _ = _oracle_a()
    _setenv(monkeypatch, WARM_ENV)
    got, collected = {}, 0
    with azhip.Engine(**_cfg_a()) as e:
        _warm(e)
        e.selfplay_begin(-1, 0)
        for _ in range(6):
            e.selfplay_step(300)
            games, moves, ng, nm = e.selfplay_collect(256)
            got.update(_by_id(games, moves, ng))
            collected += ng
        st = e.selfplay_stats()
        aborted = e.selfplay_aborted()
        e.selfplay_end()
    mine = sorted(gid for gid in got if gid < 32)
    print("case E: collected %d games, ids below 32: %s, aborted=%d %s" % (collected, mine, st.aborted_games, aborted))
    assert st.aborted_games == 0, aborted
    assert collected == len(got)
    for gid in mine:
        assert got[gid] == want[gid], gid
    assert len(mine) >= 16


# ------------------------------------------------------------------------------------------------------------------ G
ARENA_C = dict(oracle=R.ORACLE_HASH, nsims=3000, cpuct=2.0, noise_eps=0.05, noise_alpha=1.0, temp_xs=(0,), temp_ys=(0.2,))
ARENA_B = dict(oracle=R.ORACLE_HASH, nsims=2000, cpuct=1.0, noise_eps=0.25, noise_alpha=0.7, temp_xs=(0, 4), temp_ys=(1.0, 0.5))


@functools.lru_cache(maxsize=None)
def _oracle_arena(assignment):
    return R.arena(R.C4, 8, 4, ARENA_C, ARENA_B, alternate_colors=True, flip_probability=0.5, reset_every=0, seed=21,
                   assignment=np.array(assignment, dtype=np.int32))


def _arena_kw(pl, batch):
    return dict(game=R.C4, oracle=pl["oracle"], num_workers=4, batch_size=batch, num_iters_per_turn=pl["nsims"], cpuct=pl["cpuct"],
                dirichlet_noise_eps=pl["noise_eps"], dirichlet_noise_alpha=pl["noise_alpha"], temperature=(list(pl["temp_xs"]), list(pl["temp_ys"])),
                reset_every=0, flip_probability=0.5, seed=21)


@pytest.mark.parametrize("pool", ["mapped", "plain", "mapped, cache on"])
@pytest.mark.parametrize("batch", [4, 2])
def test_g_arena_on_a_mapped_pool(monkeypatch, batch, pool):
    """az_arena_run drives explore_begin / wave / explore_end itself: 3000 and 2000 simulations per ply on trees kept over a worker's two
    games pass node 16 384 within the first game.  Outside self-play nothing is retired: a tree that outgrows its chunks ends the call
    with AZ_ERR_CAPACITY.  Records, rewards and redundancy are the oracle's for the reported assignment, on both pools."""
    import azhip
    env = {"AZHIP_VMM": "0" if pool == "plain" else "1"}
    if pool.endswith("cache on"):
        env.update(AZHIP_EVAL_CACHE="1", AZHIP_EVAL_CACHE_LOG2="22")
    _setenv(monkeypatch, env)
    with azhip.Engine(**_arena_kw(ARENA_C, batch)) as ec, azhip.Engine(**_arena_kw(ARENA_B, batch)) as eb:
        games, moves, ng, nm, rew, red = ec.arena_run(eb, 8, alternate_colors=True)
        nodes = [[e.mcts_counters(s)[2] for s in range(4)] for e in (ec, eb)]
        held = [e.device_bytes() for e in (ec, eb)]
    print("case G batch=%d %s: ng=%d nm=%d, slots' nodes contender %s baseline %s, device_bytes %s" % (batch, pool, ng, nm, nodes[0], nodes[1], held))
    g_ref, m_ref, nm_ref, rew_ref, red_ref = _oracle_arena(tuple(int(x) for x in R.assignment_of(games, 8)))
    assert ng == 8 and nm == nm_ref
    for i in range(8):
        a, b = games[i], g_ref[i]
        assert (a.game_id, a.slot, a.num_moves, tuple(a.final_key)) == (b.game_id, b.slot, b.num_moves, tuple(b.final_key)), i
        for k in range(a.num_moves):
            x, y = moves[a.first_move + k], m_ref[b.first_move + k]
            assert (tuple(x.key), list(x.N), x.action, x.reward) == (tuple(y.key), list(y.N)[:len(list(x.N))], y.action, y.reward), (i, k)
    assert np.array_equal(rew, rew_ref) and red == red_ref
    assert max(nodes[0]) > CHUNK and max(nodes[1]) > CHUNK


# ------------------------------------------------------------------------------------------------------------------ H
def test_h_a_budget_that_runs_out_retires_slots_and_keeps_the_completed_games(monkeypatch):
    """AZHIP_POOL_GB = the first node chunk of every slot, the side-record granules those need (pieces of 16 384 x 32 B, four to a 2 MB
    granule) and four more 2 MB units: a few slots get a second chunk, the others stop growing at 16 384 nodes and are retired when a game
    needs more (a bounds test, DParams::retire).  The phase still returns; what completed is the oracle's; only games that need more than
    one chunk are aborted."""
    import azhip
    from azhip import _lib as L
    want, _ = _oracle_a()
    G = 16
    side_piece = CHUNK * 32
    first = G * CHUNK_BYTES + -(-G * side_piece // CHUNK_BYTES) * CHUNK_BYTES
    budget = first + 4 * CHUNK_BYTES
    _setenv(monkeypatch, dict(WARM_ENV, AZHIP_POOL_GB=repr(budget / float(1 << 30))))
    with azhip.Engine(**_cfg_a(workers=G, batch=G)) as e:
        before = e.device_bytes()                                    # the fixed allocations and the first chunks
        g, m, ng, nm, st = e.selfplay_run(32)                        # status OK: the phase is not lost
        aborted = e.selfplay_aborted()
        after = e.device_bytes() - C.sizeof(L.MoveRec) * 32 * e.max_moves()   # (the phase's move records are counted too)
    got = _by_id(g, m, ng)
    given_up = [a for a in aborted if a & BIT]
    orig_aborted = [a for a in aborted if not a & BIT]
    print("case H: budget %d B, mapped beyond the first chunks %d B, ng=%d aborted=%s" % (budget, after - before, ng, aborted))
    assert 0 < after - before <= 4 * CHUNK_BYTES                    # the budget held
    assert st.aborted_games == len(aborted) >= 1 and ng == 32 - len(given_up)
    for gid, rec in got.items():
        if not gid & BIT:
            assert rec == want[gid], gid
    assert not (set(got) & set(aborted))
    assert all(want[a][0][1] > CHUNK for a in orig_aborted), [(a, want[a][0][1]) for a in orig_aborted]
