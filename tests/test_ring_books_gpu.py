"""The books of the circular buffer (csrc/ring_books.h) as both device memories keep them: the scripts of tests/ring_books_cases.py
replayed through az_plane_memory_* and az_memory_* at Tic-tac-toe's geometry, every pushed sample carrying its number, and what
samples() / dataset() hand back compared with the deque model element for element -- get_experience and last_batch, after wraps,
over-capacity pushes, new_batch and empty.  Where the two memories differ on purpose the test says so: an empty selection is an
error for the plane memory (one text for an empty batch, one for an empty memory) and a data set of 0 samples for the keyed one."""
import ctypes as C

import numpy as np
import pytest

import memory_cases as MC
import ring_books_cases as RC

pytestmark = pytest.mark.gpu

NA = 9                                          # Tic-tac-toe: 3 planes of 3 x 3, 9 actions


def _plane_push(mem, first_tag, n, advance):
    """n samples numbered first_tag .. in push order: the number sits in X[0, 0, 0], in z and (samples) in t"""
    tags = np.arange(first_tag, first_tag + n, dtype=np.float64)
    X = np.zeros((n, 3, 3, 3), np.float32)
    A, P = np.ones((n, NA), np.float32), np.full((n, NA), 1.0 / NA)
    if not advance:
        X[:, 0, 0, 0] = tags
        mem.push_samples(X, A, P, tags, tags)
        return
    # push_trace! pushes the LAST position first: staged in playing order, position i is pushed as number n - 1 - i of the push.
    # gamma = 0 and white to move everywhere: z is the position's own reward
    X[:, 0, 0, 0] = tags[::-1]
    mem.push_trace(X, A, P, tags[::-1].copy(), np.ones(n, np.uint8), 0.0)


def _plane_selection(mem, last_batch):
    with mem.dataset(last_batch=last_batch) as d:
        W, X, A, P, V = d.tensors()
        assert d.num_samples == len(V) == d.sum_n
        assert np.array_equal(X[:, 0, 0, 0], V) and np.all(W == 1.0) and np.all(A == 1.0)
        return [int(v) for v in V]


@pytest.mark.parametrize("name", sorted(RC.CASES))
def test_plane_memory_against_the_deque(name):
    import azhip
    cap, script = RC.CASES[name]
    want = RC.model(cap, script)
    with azhip.PlaneMemoryBuffer(azhip.TicTacToeSpec(), cap) as mem:
        tag = 0
        for op in script:
            if op[0] == "push":
                _plane_push(mem, tag, op[1], op[2])
                tag += op[1]
            else:
                getattr(mem, op[0])()
        assert (len(mem), mem.cur_batch_size()) == (want["len"], want["batch"])
        X, A, P, z, t, n = mem.samples()
        assert [int(v) for v in z] == want["tags"] == [int(v) for v in X[:, 0, 0, 0]]
        assert np.all(n == 1) and np.all(t >= 1)
        if want["len"]:
            assert _plane_selection(mem, False) == want["tags"]
        else:
            with pytest.raises(azhip._lib.AzError, match="the plane memory is empty"):
                mem.dataset()
        if want["batch"]:
            assert _plane_selection(mem, True) == [want["base"] + q for q in want["last_batch"]]
        else:
            with pytest.raises(azhip._lib.AzError, match="the current batch is empty"):
                mem.dataset(last_batch=True)


def _keyed_push(L, mem, first_tag, n, advance):
    """as _plane_push, for the empty board (key 0, white to move): the number sits in z"""
    lib = L.lib()
    if not advance:
        s = np.zeros(n, MC.SAMPLE)
        s["pi"][:, :NA] = 1.0 / NA
        s["z"] = s["t"] = np.arange(first_tag, first_tag + n)
        s["n"] = 1
        L.check(lib.az_memory_push_samples(mem, MC.vp(s), n))
        return
    games, moves = (L.GameRec * 1)(), (L.MoveRec * n)()            # one game of n positions, as tests/test_memory_kernels_gpu.py makes it
    games[0].num_moves = n
    for i, m in enumerate(moves):
        for a in range(NA):
            m.N[a] = 1
        m.reward = float(first_tag + n - 1 - i)                      # the last position is pushed first; gamma = 0: z is the reward
    tb = L.TraceBuf()
    tb.games, tb.games_cap, tb.num_games, tb.moves, tb.moves_cap, tb.num_moves = games, 1, 1, moves, n, n
    L.check(lib.az_memory_push(mem, C.byref(tb), 0.0))


def _keyed_selection(L, mem, which):
    lib, ds, info = L.lib(), C.c_void_p(), L.DatasetInfo()
    L.check(lib.az_dataset_create(mem, which, 0, 0, 0, C.byref(ds)))
    try:
        L.check(lib.az_dataset_get_info(ds, C.byref(info)))
        n = info.num_samples
        s, V = np.zeros(max(n, 1), MC.SAMPLE), np.zeros(max(n, 1), np.float32)
        L.check(lib.az_dataset_read(ds, 0, n, MC.vp(s), None, None, None, None, MC.vp(V)))
        assert np.array_equal(s["z"][:n].astype(np.float32), V[:n]) and np.all(s["n"][:n] == 1) and info.sum_n == n
        return [int(v) for v in s["z"][:n]]
    finally:
        lib.az_dataset_destroy(ds)


@pytest.mark.parametrize("name", sorted(RC.CASES))
def test_keyed_memory_against_the_deque(name):
    from azhip import _lib as L
    cap, script = RC.CASES[name]
    want = RC.model(cap, script)
    lib, mem = L.lib(), C.c_void_p()
    L.check(lib.az_memory_create(1, 0, cap, C.byref(mem)))
    try:
        tag = 0
        for op in script:
            if op[0] == "push":
                _keyed_push(L, mem, tag, op[1], op[2])
                tag += op[1]
            else:
                L.check(getattr(lib, "az_memory_" + op[0])(mem))
        length, batch = C.c_int64(), C.c_int64()
        L.check(lib.az_memory_length(mem, C.byref(length), C.byref(batch)))
        assert (length.value, batch.value) == (want["len"], want["batch"])
        assert _keyed_selection(L, mem, 0) == want["tags"]          # an empty selection is a data set of 0 samples here
        assert _keyed_selection(L, mem, 1) == [want["base"] + q for q in want["last_batch"]]
    finally:
        lib.az_memory_destroy(mem)
