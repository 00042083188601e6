"""az_comm_gather_push_planes with a world of ONE rank over the real collective library (the form of
test_native_comm_single_rank_gather_and_broadcast): the outbox's current batch -> the destination memory in ascending game id, bit for
bit what RefMemory (tests/test_plane_memory_gpu.py) holds after push_trace of the same traces in that order.  Ring wrap on both sides,
T above the destination's capacity, the three record shapes (Tic-tac-toe: 16-byte words; Connect Four: odd RW, the padding word; Go:
rows longer than 64 words, nA = 82), forced small rounds, no destination, the refusals, and a data set built from the result."""
import ctypes as C

import numpy as np
import pytest

from plane_gather_cases import C4, GAMMA, GO9, RECORD_BYTES, TTT, make_filler, make_trace, same_samples, same_state, spec, state
from test_plane_memory_gpu import RefMemory

pytestmark = pytest.mark.gpu
SEED = 11
BATCH = [(40, 5), (3, 9), (17, 1), (8, 7), (21, 6)]                  # (game id, positions) in push order: 28 samples


@pytest.fixture(scope="module")
def comm():
    from azhip import comm as CM
    with CM.Comm(0, 0, 1, CM.unique_id()) as c:
        yield c


def round_rows(c, rows):
    from azhip import _lib as L
    f = L.lib().az_debug_comm_plane_round_rows
    f.argtypes, f.restype = [C.c_void_p, C.c_int64], C.c_int
    L.check(f(c._h, rows))


def new_memory(game, capacity, filler=0, ref=None):
    """a PlaneMemoryBuffer holding `filler` samples pushed by push_samples (and the same in ref)"""
    import azhip
    mem = azhip.PlaneMemoryBuffer(spec(game), capacity)
    if filler:
        s = make_filler(game, SEED + capacity, filler)
        mem.push_samples(*s)
        for i in range(filler):
            if ref is not None:
                ref.push(*[a[i] for a in s])
    return mem


def outbox(game, capacity, filler, batch):
    src = new_memory(game, capacity, filler)
    src.new_batch()
    for gid, n in batch:
        src.push_trace(*make_trace(game, SEED, gid, n), GAMMA, game_id=gid)
    return src


def expected(game, capacity, filler, batch):
    ref = RefMemory(capacity)
    new_memory(game, capacity, filler, ref).close()
    for gid, n in sorted(batch):
        ref.push_trace(*make_trace(game, SEED, gid, n), GAMMA)
    es = ref.get_experience()
    arrays = (np.stack([e[0] for e in es]), np.stack([e[1] for e in es]), np.stack([e[2] for e in es]), np.array([e[3] for e in es], dtype=np.float64),
              np.array([e[4] for e in es], dtype=np.float64), np.array([e[5] for e in es], dtype=np.int64))
    return arrays, len(ref), ref.cur_batch_size()


def gather(comm, game, src_cap, src_filler, batch, dst_cap, dst_filler):
    src, dst = outbox(game, src_cap, src_filler, batch), new_memory(game, dst_cap, dst_filler)
    before = state(src)
    st = comm.gather_push_planes(src, dst)
    assert (st.games, st.moves, st.ranks) == (len(batch), sum(n for _, n in batch), 1)
    assert st.bytes >= st.moves * RECORD_BYTES[game] and st.total_ms >= st.gather_ms > 0
    assert (st.total_simulations, st.total_nodes_traversed, st.max_nodes, st.mean_game_depth, st.replaced_games) == (0, 0, 0, 0.0, 0)
    assert same_state(state(src), before)                                # the outbox is never modified
    got = state(dst)
    src.close(); dst.close()
    return got


def test_batch_straddling_the_ring_into_a_destination_that_wraps(comm):
    """src: capacity 40, 30 filler samples, then the batch of 28 -> slots 30..39, 0..17.  dst: capacity 25, 10 earlier samples"""
    got, want = gather(comm, TTT, 40, 30, BATCH, 25, 10), expected(TTT, 25, 10, BATCH)
    assert want[1:] == (25, 25) and same_state(got, want)


def test_more_samples_than_the_destination_holds(comm):
    got, want = gather(comm, TTT, 40, 30, BATCH, 20, 10), expected(TTT, 20, 10, BATCH)
    assert want[1:] == (20, 20) and same_state(got, want)


def test_destination_with_room_keeps_its_earlier_samples(comm):
    got, want = gather(comm, TTT, 40, 30, BATCH, 64, 10), expected(TTT, 64, 10, BATCH)
    assert want[1:] == (38, 28) and same_state(got, want)


def test_connect_four_geometry_has_a_live_padding_word(comm):
    got, want = gather(comm, C4, 40, 30, BATCH, 25, 10), expected(C4, 25, 10, BATCH)
    assert same_state(got, want)


def test_go_geometry_rows_longer_than_a_wavefront(comm):
    batch = [(5, 70), (2, 3)]
    got, want = gather(comm, GO9, 100, 60, batch, 64, 5), expected(GO9, 64, 5, batch)
    assert want[1:] == (64, 64) and same_state(got, want)


def test_forced_rounds_give_the_same_memory(comm):
    """3 rows per round: 28 rows in 10 rounds, the last one partial"""
    want = gather(comm, TTT, 40, 30, BATCH, 25, 10)
    round_rows(comm, 3)
    try:
        got = gather(comm, TTT, 40, 30, BATCH, 25, 10)
    finally:
        round_rows(comm, 0)
    assert same_state(got, want) and same_state(got, expected(TTT, 25, 10, BATCH))


def test_no_destination_takes_part_and_stores_nothing(comm):
    src = outbox(TTT, 40, 30, BATCH)
    before = state(src)
    st = comm.gather_push_planes(src, None)
    assert (st.games, st.moves, st.ranks) == (5, 28, 1) and st.bytes >= 28 * RECORD_BYTES[TTT]
    assert same_state(state(src), before)
    st = comm.gather_push_planes(new_memory(TTT, 8), None)              # an empty batch is a valid contribution
    assert (st.games, st.moves) == (0, 0)
    src.close()


def test_refusals_leave_both_memories_and_the_communicator_as_they_were(comm):
    import azhip
    src, dst = outbox(TTT, 40, 30, BATCH), new_memory(TTT, 25, 10)
    ids, lens = src.batch_games()
    assert ids.dtype == lens.dtype == np.int32 and list(zip(ids, lens)) == BATCH
    small = outbox(TTT, 20, 0, BATCH)                                   # 28 samples through a ring of 20: the batch was overwritten
    other = new_memory(C4, 25, 10)
    s0, d0 = state(src), state(dst)

    def change(a, k, v):
        a = a.copy()
        a[k] = v
        return a
    refused = [
        ("sum", lambda: comm.gather_push_planes(src, dst, ids, change(lens, 1, 8))),
        ("overwritten", lambda: comm.gather_push_planes(small, dst)),
        ("destination is the source", lambda: comm.gather_push_planes(src, src)),
        ("geometry", lambda: comm.gather_push_planes(src, other)),
        ("length 0", lambda: comm.gather_push_planes(src, dst, ids, change(change(lens, 0, 14), 1, 0))),
        ("negative id", lambda: comm.gather_push_planes(src, dst, change(ids, 2, -17), lens)),
        ("id 3 occurs twice", lambda: comm.gather_push_planes(src, dst, change(ids, 3, 3), lens)),
    ]
    for what, call in refused:
        with pytest.raises(azhip.AzError, match=what):
            call()
        assert same_state(state(src), s0) and same_state(state(dst), d0), what
        assert comm.gather_push_planes(src, None).moves == 28, what      # the communicator is still usable
    with pytest.raises(ValueError):
        comm.gather_push_planes(src, dst, ids.astype(np.float64), lens)
    with pytest.raises(ValueError):
        comm.gather_push_planes(src, dst, ids[:4], lens)
    with pytest.raises(ValueError):
        comm.gather_push_planes(src, dst, ids, None)
    src.push_trace(*make_trace(TTT, SEED, 99, 2), GAMMA)                # a trace without an id: the record cannot speak for the batch
    with pytest.raises(ValueError):
        comm.gather_push_planes(src, dst)
    src.new_batch()
    assert src.batch_games()[0].size == 0
    comm.gather_push_planes(outbox(TTT, 40, 30, BATCH), dst)
    assert same_state(state(dst), expected(TTT, 25, 10, BATCH))
    for m in (src, dst, small, other):
        m.close()


def test_data_set_built_from_the_gathered_memory(comm):
    """last_batch / get_experience with use_position_averaging: the tensors of a single-process memory holding the same games"""
    import azhip
    src, dst = outbox(TTT, 40, 30, BATCH), new_memory(TTT, 64, 10)
    one = new_memory(TTT, 64, 10)
    for gid, n in sorted(BATCH):
        one.push_trace(*make_trace(TTT, SEED, gid, n), GAMMA)
    comm.gather_push_planes(src, dst)
    for last_batch in (False, True):
        with dst.dataset(last_batch=last_batch, use_position_averaging=True, weighing_policy=azhip._lib.WEIGHT_LINEAR) as a, \
                one.dataset(last_batch=last_batch, use_position_averaging=True, weighing_policy=azhip._lib.WEIGHT_LINEAR) as b:
            assert len(a) == len(b) == (28 if last_batch else 38) and same_samples(a.tensors(), b.tensors())
            assert (a.sum_n, a.Wtot, a.Wmean, a.Hp) == (b.sum_n, b.Wtot, b.Wmean, b.Hp)
    for m in (src, dst, one):
        m.close()
