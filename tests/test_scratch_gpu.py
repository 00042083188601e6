"""The device scratch of a call is gone when the call returns, on the paths that succeed and on the paths that refuse half way.
csrc/engine.h Scratch owns it and counts what all live owners hold; the debug seam az_debug_scratch_live_bytes reads the count, and
every call below -- each one succeeds or is refused today, none provokes a fault -- must leave it at 0.  A refused call must also
keep today's status and message.

One process: a Tic-tac-toe az_memory and a Tic-tac-toe plane memory of capacity 8.  Two ranks on one GPU through tests/rccl_stub:
both gathers with a local refusal on rank 1 -- both ranks return, rank 1 with its own reason and rank 0 naming rank 1, and the next
correct collective on the same communicators succeeds (a local refusal aborts nothing)."""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch.multiprocessing as mp

from plane_gather_cases import GAMMA, TTT, make_filler, make_trace, spec

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "tests", "rccl_stub", "librccl_stub.so")
CAP = 8
PILLEGAL = "P > 0 where A == 0 (the loss takes the logarithm of the masked policy there)"


def live():
    """az_debug_scratch_live_bytes: declared here, like the other az_debug_* seams -- it is not in azhip.h"""
    from azhip import _lib as L
    f = L.lib().az_debug_scratch_live_bytes
    f.argtypes, f.restype = [C.POINTER(C.c_int64)], C.c_int
    n = C.c_int64(-1)
    L.check(f(C.byref(n)))
    return n.value


def refused(status, message, call, *args):
    """the call is refused with exactly this status and message, and leaves no scratch behind"""
    from azhip import _lib as L
    with pytest.raises(L.AzError) as ei:
        call(*args)
    assert str(ei.value) == "azhip status %d: %s" % (status, message)
    assert live() == 0


def ttt_trace(ngames, nmoves):
    """ngames identical Tic-tac-toe games of nmoves <= 9 positions as az_move_rec: the players fill cells 0, 1, 2, ... in turn, every free
    cell visited once.  key = (white's cells, black's cells), nobody's side bit set."""
    from azhip import _lib as L
    games, moves = (L.GameRec * ngames)(), (L.MoveRec * (ngames * nmoves))()
    for g in range(ngames):
        games[g].game_id, games[g].num_moves, games[g].first_move = g, nmoves, g * nmoves
        for i in range(nmoves):
            m = moves[g * nmoves + i]
            m.key[0] = sum(1 << c for c in range(0, i, 2))
            m.key[1] = sum(1 << c for c in range(1, i, 2))
            for a in range(i, 9):
                m.N[a] = 1
            m.action, m.reward = i, 0.0
    return games, moves


def test_the_replay_memory_leaves_no_scratch():
    import azhip
    from azhip import _lib as L
    assert live() == 0
    gspec = azhip.TicTacToeSpec()
    mem = azhip.MemoryBuffer(gspec, CAP)
    games, moves = ttt_trace(2, 6)
    mem.push_records(games, moves, 2, 12, GAMMA)                     # 12 samples into a ring of 8
    assert (len(mem), mem.cur_batch_size(), live()) == (CAP, CAP, 0)
    with mem.dataset(use_symmetries=True, use_position_averaging=True) as d:
        assert 0 < len(d) < CAP * 8 and d.sum_n == CAP * 8           # the two games are one game twice: images merge
        assert live() == 0
    mem.new_batch()
    with mem.dataset(last_batch=True) as d:                          # an empty batch is an empty data set here
        assert len(d) == 0 and live() == 0
    mem.close()
    # az_learning_status on 3 samples in loss batches of 2 (one partial)
    hp = azhip.ResNetHP(num_blocks=1, num_filters=64, num_policy_head_filters=32, num_value_head_filters=32)
    small = azhip.MemoryBuffer(gspec, CAP)
    games, moves = ttt_trace(1, 3)
    small.push_records(games, moves, 1, 3, GAMMA)
    with small.dataset() as d, azhip.Engine(game=TTT, oracle=azhip.ORACLE_RESNET, num_workers=8, batch_size=8, num_iters_per_turn=2, num_blocks=1,
                                            num_filters=64, num_policy_head_filters=32, num_value_head_filters=32) as e:
        assert len(d) == 3
        e.net_set_params(azhip.ResNet(gspec, hp, seed=1).params())
        out = L.LearningStatusRec()
        L.check(L.lib().az_learning_status(e._h, d._h, 1e-4, 1.0, 1.0, 2, C.byref(out)))
        assert np.isfinite(out.L) and out.Lreg > 0 and live() == 0
    small.close()
    # az_dataset_create_from_tensors refused for W <= 0 in sample 0 of 2
    X, A, P, z, _, _ = make_filler(TTT, 5, 2)
    W = np.array([0.0, 1.0], dtype=np.float32)
    refused(L.AZ_ERR_BAD_ARG, "sample 0: W <= 0", azhip.TensorDataset, gspec, W, X, A, P.astype(np.float32), z.astype(np.float32))
    with azhip.TensorDataset(gspec, np.ones(2, dtype=np.float32), X, A, P.astype(np.float32), z.astype(np.float32)) as d:
        assert len(d) == 2 and live() == 0


def test_the_plane_memory_leaves_no_scratch():
    import azhip
    from azhip import _lib as L
    assert live() == 0
    gspec = spec(TTT)
    mem = azhip.PlaneMemoryBuffer(gspec, CAP)
    mem.set_symmetries(*azhip.plane_symmetries(gspec))
    X, A, P, r, wp = make_trace(TTT, 3, 0, 12)
    mem.push_trace(X, A, P, r, wp, GAMMA)                            # 12 samples into a ring of 8
    assert (len(mem), mem.cur_batch_size(), live()) == (CAP, CAP, 0)
    with mem.dataset(use_symmetries=True, use_position_averaging=True) as d:
        assert 0 < len(d) <= CAP * 8 and d.sum_n == CAP * 8 and live() == 0
    mem.new_batch()
    refused(L.AZ_ERR_STATE, "the current batch is empty (push_trace advances it, new_batch resets it)", mem.dataset, True)
    # a push refused for sample 1 of 3: a policy weight on an action the mask forbids (another action stays legal)
    X, A, P, z, t, n = [a.copy() for a in make_filler(TTT, 4, 3)]
    A[1], P[1] = 0.0, 0.0
    A[1, 0], P[1, 0], P[1, 5] = 1.0, 0.5, 0.5
    before = mem.samples()
    refused(L.AZ_ERR_BAD_ARG, "sample 1: " + PILLEGAL, mem.push_samples, X, A, P, z, t, n)
    assert all(np.array_equal(a, b) for a, b in zip(mem.samples(), before))
    mem.close()
    # a build refused for a hash collision: 4 distinct rows on the 2 keys that 1 bit leaves
    four = azhip.PlaneMemoryBuffer(gspec, CAP)
    s = make_filler(TTT, 6, 4)
    assert len(np.unique(np.concatenate([s[0].reshape(4, -1), s[1]], axis=1), axis=0)) == 4
    four.push_samples(*s)
    f = L.lib().az_debug_plane_memory_hash_bits
    f.argtypes, f.restype = [C.c_void_p, C.c_int32], C.c_int
    L.check(f(four._h, 1))
    refused(L.AZ_ERR_STATE, "plane hash collision: two different (X, A) rows share their 1-bit key; no data set was built", four.dataset, False, False, True)
    L.check(f(four._h, 128))
    with four.dataset(use_position_averaging=True) as d:
        assert len(d) == 4 and live() == 0
    four.close()


# ---------------------------------------------------------------------------------------------------- two ranks, one GPU
def _expect(rank, call, own, own_status, what):
    """rank 1 is refused for its own reason, rank 0 learns that rank 1 cannot take part; nobody keeps scratch"""
    import azhip
    from azhip import _lib as L
    try:
        call()
        raise AssertionError("%s: rank %d was not refused" % (what, rank))
    except azhip.AzError as ex:
        if rank == 1:
            assert ex.status == own_status and own in str(ex), str(ex)
        else:
            assert ex.status == L.AZ_ERR_COMM and "rank 1 cannot take part in the " + what in str(ex), str(ex)
    assert live() == 0


def _worker(rank, world, port):
    sys.path[:0] = [os.path.join(ROOT, "alphazero.jl_amd")]
    os.environ["AZHIP_RCCL_LIB"] = STUB
    os.environ["AZSTUB_TIMEOUT_S"] = "30"                             # a rank that does not arrive is an error after 30 s, not a hang
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)       # carries the 128-byte unique id only
    import azhip
    from azhip import _lib as L
    from azhip import comm
    lib = L.lib()
    with comm.Comm(0, rank, world, comm.torch_broadcast_id(rank)) as c:
        # az_comm_gather_push: rank 1 passes no engine
        gspec = azhip.TicTacToeSpec()
        mem = azhip.MemoryBuffer(gspec, 64)
        with azhip.Engine(game=TTT, oracle=azhip.ORACLE_UNIFORM, num_workers=2, batch_size=2, num_iters_per_turn=4) as e:
            e.selfplay_run(2, first_game_id=2 * rank, device_only=True)
            st = L.GatherStats()
            _expect(rank, lambda: L.check(lib.az_comm_gather_push(c._h, None if rank == 1 else e._h, mem._h, 1.0, C.byref(st))),
                    "NULL engine", L.AZ_ERR_BAD_ARG, "gather")
            assert len(mem) == 0
            st = c.gather_push(e, mem, 1.0)                            # the same communicator, nothing was aborted
            assert (st.games, st.ranks, len(mem)) == (4, world, st.moves) and live() == 0
        mem.close()
        # az_comm_gather_push_planes: rank 1's table sums to the wrong batch
        src, dst = azhip.PlaneMemoryBuffer(spec(TTT), 16), azhip.PlaneMemoryBuffer(spec(TTT), 16)
        src.push_trace(*make_trace(TTT, 9, rank, 3 + rank), GAMMA, game_id=rank)
        ids, lens = src.batch_games()
        _expect(rank, lambda: c.gather_push_planes(src, dst, ids, lens + 1 if rank == 1 else lens), "lengths sum to", L.AZ_ERR_BAD_ARG, "plane gather")
        assert len(dst) == 0
        st = c.gather_push_planes(src, dst)
        assert (st.games, st.moves, st.ranks, len(dst)) == (2, 7, world, 7) and live() == 0
        src.close(); dst.close()
    dist.destroy_process_group()


def test_a_local_refusal_in_a_gather_returns_on_both_ranks_and_aborts_nothing():
    if not os.path.exists(STUB):
        subprocess.check_call(["make", "-C", os.path.dirname(STUB)])
    port = 30900 + os.getpid() % 2000
    ranks = mp.spawn(_worker, args=(2, port), nprocs=2, join=False)
    deadline = time.monotonic() + 120                                 # both ranks return, whatever the other one did: none may hang
    while not ranks.join(timeout=5):                                  # (raises as soon as a rank has failed)
        if time.monotonic() > deadline:
            for proc in ranks.processes:
                proc.kill()
            raise AssertionError("a rank did not return within 120 s")
