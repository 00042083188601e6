"""What the tests of az_comm_gather_push_planes share: traces built from (seed, game id) alone, so that any process can regenerate any
game, filler samples, and the bit-for-bit comparison of a PlaneMemoryBuffer's contents."""
import numpy as np

C4, TTT, GO9 = 0, 1, 3
SPECS = {C4: "ConnectFourSpec", TTT: "TicTacToeSpec", GO9: "Go9PlanesSpec"}
DIMS = {C4: (3, 6, 7), TTT: (3, 3, 3), GO9: (4, 9, 9)}            # (C, H, W)
NUM_ACTIONS = {C4: 7, TTT: 9, GO9: 82}
RECORD_BYTES = {C4: 616, TTT: 240, GO9: 2304}
GAMMA = 0.9


def spec(game):
    import azhip
    return getattr(azhip, SPECS[game])()


def make_trace(game, seed, gid, length):
    """(X, A, pi, rewards, white_playing) of game `gid`: planes in {0, 1}, a mask with a legal action, pi >= 0 on legal actions only"""
    rng = np.random.default_rng([seed, gid])
    nA = NUM_ACTIONS[game]
    X = rng.integers(0, 2, size=(length,) + DIMS[game]).astype(np.float32)
    A = (rng.random((length, nA)) < 0.6).astype(np.float32)
    A[np.arange(length), rng.integers(0, nA, length)] = 1.0
    P = rng.random((length, nA)) * A
    P /= P.sum(axis=1, keepdims=True)
    return X, A, P, rng.integers(-1, 2, length).astype(np.float64), rng.integers(0, 2, length).astype(np.uint8)


def make_filler(game, seed, count):
    """(X, A, pi, z, t, n) for push_samples: samples that are nobody's batch, some seen more than once"""
    X, A, P, _, _ = make_trace(game, seed, 1 << 20, count)
    rng = np.random.default_rng([seed, 7])
    return X, A, P, rng.uniform(-1, 1, count), rng.integers(1, 40, count).astype(np.float64), rng.integers(1, 6, count).astype(np.int64)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_samples(got, want):
    """two (X, A, pi, z, t, n) tuples, bit for bit"""
    return all(g.shape == w.shape and g.dtype == w.dtype and np.array_equal(bits(g), bits(w)) for g, w in zip(got, want))


def state(mem):
    return mem.samples(), len(mem), mem.cur_batch_size()


def same_state(a, b):
    return same_samples(a[0], b[0]) and a[1:] == b[1:]
