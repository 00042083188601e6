"""az_comm_gather_push_planes with several ranks: a world of 2 and 4 on the ONE GPU of the test box through tests/rccl_stub (launched as
test_native_comm_several_ranks_share_one_gpu_through_the_transport_seam launches its ranks), and two real ranks on two GPUs over RCCL
where two devices are visible.  Eleven games of 1 to 9 positions, ids dealt so that every rank's ids interleave with the others'; each
rank pushes its games in DESCENDING id; with a world of 4 one rank holds no game at all; rounds of 4 rows, so the ranks fill their
segments unevenly over several rounds.  Every rank's destination (capacity 30, the same 7 samples to begin with) must hold what a
single-process memory holds after push_trace of all games in ascending id -- bit for bit -- and the failure agreement must return on
every rank: the failing rank with its own message, the others naming it; a duplicate id is AZ_ERR_BAD_ARG everywhere."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp

from plane_gather_cases import C4, GAMMA, TTT, make_filler, make_trace, same_samples, spec

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "tests", "rccl_stub", "librccl_stub.so")
SEED, CAP, FILLER = 23, 30, 7
LENS = [1 + (4 * g) % 9 for g in range(11)]                          # 1 5 9 4 8 3 7 2 6 1 5: every length 1..9, 51 samples
GAMES = (TTT, C4)


def owner(world, gid):
    """world 2: ids alternate; world 4: ids go round ranks 0, 1, 3 and rank 2 holds no game"""
    return gid % 2 if world == 2 else (0, 1, 3)[gid % 3]


def fresh_destination(game, device=0):
    import azhip
    mem = azhip.PlaneMemoryBuffer(spec(game), CAP, device=device)
    mem.push_samples(*make_filler(game, SEED, FILLER))
    return mem


def _worker(rank, world, port, out_dir, stub):
    sys.path[:0] = [os.path.join(ROOT, "alphazero.jl_amd")]
    if stub:
        os.environ["AZHIP_RCCL_LIB"] = STUB
        os.environ["AZSTUB_TIMEOUT_S"] = "30"                         # a missing rank is an error after 30 s, not a hang
    dev = 0 if stub else rank
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)       # carries the 128-byte unique id only
    import azhip
    from azhip import _lib as L
    from azhip import comm
    with comm.Comm(dev, rank, world, comm.torch_broadcast_id(rank)) as c:
        f = L.lib().az_debug_comm_plane_round_rows
        f.argtypes, f.restype = [C.c_void_p, C.c_int64], C.c_int
        L.check(f(c._h, 4))
        for game in GAMES:
            src = azhip.PlaneMemoryBuffer(spec(game), 64, device=dev)
            src.push_samples(*make_filler(game, SEED + 1, 40))         # rank 0's batch straddles the outbox's end
            src.new_batch()
            for gid in reversed(range(len(LENS))):
                if owner(world, gid) == rank:
                    src.push_trace(*make_trace(game, SEED, gid, LENS[gid]), GAMMA, game_id=gid)
            ids, lens = src.batch_games()
            dst = fresh_destination(game, dev)
            before = dst.samples()
            # one rank passes a wrong sum of lengths: every rank raises, that rank its own message, the others name it
            try:
                c.gather_push_planes(src, dst, ids, lens + 1 if rank == 1 else lens)
                raise AssertionError("a wrong sum of lengths was accepted")
            except azhip.AzError as ex:
                assert ("lengths sum to" in str(ex)) if rank == 1 else ("rank 1 cannot take part" in str(ex) and ex.status == L.AZ_ERR_COMM), str(ex)
            # two ranks claim one id: AZ_ERR_BAD_ARG naming it on every rank
            taken = min(g for g in range(len(LENS)) if owner(world, g) == 0)
            try:
                c.gather_push_planes(src, dst, np.where(np.arange(ids.size) == 0, taken, ids).astype(np.int32) if rank == 1 else ids, lens)
                raise AssertionError("a duplicate game id was accepted")
            except azhip.AzError as ex:
                assert ex.status == L.AZ_ERR_BAD_ARG and "game id %d occurs twice" % taken in str(ex), str(ex)
            assert (len(dst), dst.cur_batch_size()) == (FILLER, 0) and same_samples(dst.samples(), before)   # nothing was pushed
            st = c.gather_push_planes(src, dst)                          # ... and the next call succeeds
            assert (st.games, st.moves, st.ranks) == (len(LENS), sum(LENS), world) and st.bytes >= sum(LENS) * 8
            got = dst.samples()
            np.savez(os.path.join(out_dir, "G%d_%d.npz" % (game, rank)), *got, meta=np.array([len(dst), dst.cur_batch_size()]))
            # a second call in which rank 0 passes no destination: it takes part and is unchanged
            st = c.gather_push_planes(src, None if rank == 0 else dst)
            assert st.moves == sum(LENS)
            if rank == 0:
                assert same_samples(dst.samples(), got) and (len(dst), dst.cur_batch_size()) == (CAP, CAP)
            else:
                assert (len(dst), dst.cur_batch_size()) == (CAP, CAP)
            src.close(); dst.close()
        L.check(f(c._h, 0))
    dist.destroy_process_group()


def check_ranks(tmp_path, world):
    for game in GAMES:
        one = fresh_destination(game)
        for gid in range(len(LENS)):
            one.push_trace(*make_trace(game, SEED, gid, LENS[gid]), GAMMA)
        want, meta = one.samples(), [len(one), one.cur_batch_size()]
        one.close()
        assert meta == [CAP, CAP]
        for r in range(world):
            z = np.load(tmp_path / ("G%d_%d.npz" % (game, r)))
            assert same_samples([z["arr_%d" % i] for i in range(6)], want), (game, r)
            assert list(z["meta"]) == meta, (game, r)


@pytest.mark.parametrize("world", [2, 4])
def test_plane_gather_several_ranks_share_one_gpu_through_the_transport_seam(tmp_path, world):
    if not os.path.exists(STUB):
        subprocess.check_call(["make", "-C", os.path.dirname(STUB)])
    port = 30500 + os.getpid() % 2000 + world
    mp.spawn(_worker, args=(world, port, str(tmp_path), True), nprocs=world, join=True)
    check_ranks(tmp_path, world)


def test_plane_gather_two_ranks_on_two_gpus(tmp_path):
    """the same over RCCL itself, one GPU per rank (RCCL refuses two ranks on one device): skipped on a 1-GPU box"""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs 2 GPUs (the 1-GPU box runs the ranks through tests/rccl_stub and a world of one over RCCL)")
    port = 30700 + os.getpid() % 2000
    mp.spawn(_worker, args=(2, port, str(tmp_path), False), nprocs=2, join=True)
    check_ranks(tmp_path, 2)
