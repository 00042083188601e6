"""Inputs for the data-set build's kernels (csrc/prims.h: radix sort, scan, tiled sum; csrc/memory.hip: k_mem_heads,
k_mem_merge, k_mem_merge_long) that self-play cannot produce, as numpy records of az_sample's layout, and the oracle's
merge_by_state / convert_samples / augment_with_symmetries on the same bytes.  tests/test_memory_kernels_cpu.py checks with the
oracle alone that these inputs are what they claim to be; tests/test_memory_kernels_gpu.py holds the device to the oracle on them."""
import ctypes as C

import numpy as np

import azref as R

SAMPLE = np.dtype([("key", "<u8", (2,)), ("pi", "<f8", (9,)), ("z", "<f8"), ("t", "<f8"), ("n", "<i8")])
assert SAMPLE.itemsize == 112 == C.sizeof(R.Sample)
WORDS = 14                                  # key, key, pi[0..8], z, t, n
MERGE_LONG = 256                            # csrc/memory.hip: segments of this many samples take k_mem_merge_long
TILE = 2048                                 # csrc/prims.h RS_TILE: pairs per sort tile, ints per scan tile, doubles per sum tile
BIT63 = np.uint64(1 << 63)
LENGTHS = (1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 319, 320, 321, 383, 384, 385, 2047, 2048, 2049, 4500)
# ascending-key layouts of LENGTHS (sorted index of a segment = sum of the lengths before it):
#   ORDER_A: the 2048-segment fills scan tile 0, so the next head sits exactly at sorted index 2048; that next segment (2049, long)
#            runs over 4096; a one-sample segment is last (sorted index n1 - 1)
#   ORDER_B: segments that add up to 2040 first, then the short 63-segment over sorted indices 2040..2102, across the tile boundary
#            at 2048; the 4500-segment (long) is last and ends at n1
ORDER_A = (2048, 2049) + tuple(x for x in LENGTHS if x not in (1, 2048, 2049)) + (1,)


def _order_b():
    rest = [x for x in LENGTHS if x not in (63, 4500)]
    reach = {0: ()}                                               # subset of `rest` with sum 2040, by dynamic programming
    for x in rest:
        for s, used in list(reach.items()):
            if s + x <= 2040 and s + x not in reach:
                reach[s + x] = used + (x,)
    head = reach[2040]
    return head + (63,) + tuple(x for x in rest if x not in head) + (4500,)


ORDER_B = _order_b()


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


def words(s):
    """(n, 14) uint64 view of sample records"""
    return np.ascontiguousarray(s).view("<u8").reshape(len(s), WORDS)


def live_columns(num_actions):
    """the words both sides define: key, pi[:A], z, t, n (the device also averages the padding words pi[A:], the oracle does not)"""
    return [0, 1] + list(range(2, 2 + num_actions)) + [11, 12, 13]


def fill_values(rng, s, num_actions):
    """Order-revealing values: a Float64 sum over such a segment depends on the order of its members.  z, t: mantissa in [1, 2)
    times 2^e, e uniform in [-40, 40] (z with a random sign); pi in [0, 1] times 2^e, e in [-30, 0]; n uniform in [1, 2^40)."""
    n = len(s)
    s["z"] = rng.uniform(1.0, 2.0, n) * np.exp2(rng.integers(-40, 41, n)) * rng.choice([-1.0, 1.0], n)
    s["t"] = rng.uniform(1.0, 2.0, n) * np.exp2(rng.integers(-40, 41, n))
    s["pi"][:, :num_actions] = rng.uniform(0.0, 1.0, (n, num_actions)) * np.exp2(rng.integers(-30, 1, (n, num_actions)))
    s["n"] = rng.integers(1, 1 << 40, n)
    return s


def new_samples(rng, keys, num_actions=9):
    s = np.zeros(len(keys), SAMPLE)
    s["key"] = keys
    return fill_values(rng, s, num_actions)


def random_keys(rng, n):
    """n distinct 128-bit keys, both words uniform over all 64 bits (about half with bit 63 set in each)"""
    k = rng.integers(0, 1 << 64, (n, 2), dtype=np.uint64)
    assert len(np.unique(k, axis=0)) == n
    return k


def c4_keys(rng, n):
    """n distinct Connect-Four keys of gravity-filled boards (bit 7c + r = row r of column c, bit 63 of key[0] = black to move):
    the oracle's action mask looks for the first free cell of a column, the device's at the top cell, equal on such boards"""
    h = rng.integers(0, 7, (4 * n, 7))
    colour = rng.integers(0, 2, (4 * n, 7, 6))
    a = np.zeros(4 * n, np.uint64); b = np.zeros(4 * n, np.uint64)
    for c in range(7):
        for r in range(6):
            stone = h[:, c] > r
            bit = np.uint64(1 << (7 * c + r))
            a |= np.where(stone & (colour[:, c, r] == 0), bit, np.uint64(0))
            b |= np.where(stone & (colour[:, c, r] == 1), bit, np.uint64(0))
    a |= np.where(rng.integers(0, 2, 4 * n) == 1, BIT63, np.uint64(0))
    k = np.unique(np.stack([a, b], axis=1), axis=0)
    assert len(k) >= n
    return k[rng.permutation(len(k))[:n]]


# ---------------------------------------------------------------------------------------------------------------- the oracle
def oracle_merge(game, s):
    s = np.ascontiguousarray(s)
    out = np.zeros(max(len(s), 1), SAMPLE)
    f = R.lib().azr_merge_by_state
    f.restype = C.c_int64
    return out[:f(game, vp(s), C.c_int64(len(s)), vp(out))]


def oracle_augment(game, s):
    s = np.ascontiguousarray(s)
    out = np.zeros(max(len(s) * (1 + R.lib().azr_num_symmetries(game)), 1), SAMPLE)
    f = R.lib().azr_augment_with_symmetries
    f.restype = C.c_int64
    return out[:f(game, vp(s), C.c_int64(len(s)), vp(out))]


def oracle_convert(game, policy, s):
    s = np.ascontiguousarray(s)
    n, nA = len(s), R.NUM_ACTIONS[game]
    w, h, c = R.DIMS[game]
    W = np.zeros(n, np.float32); X = np.zeros((n, c, h, w), np.float32)
    A = np.zeros((n, nA), np.float32); P = np.zeros((n, nA), np.float32); V = np.zeros(n, np.float32)
    R.lib().azr_convert_samples(game, policy, vp(s), C.c_int64(n), vp(W), vp(X), vp(A), vp(P), vp(V))
    return W, X, A, P, V


def layout(s):
    """(starts, lengths) of the segments in sorted order (ascending key[0], key[1], unsigned), by numpy alone"""
    k = s["key"]
    o = np.lexsort((k[:, 1], k[:, 0]))
    ks = k[o]
    head = np.ones(len(s), bool)
    head[1:] = (ks[1:] != ks[:-1]).any(axis=1)
    starts = np.flatnonzero(head)
    return starts, np.diff(np.append(starts, len(s)))


# ---------------------------------------------------------------------------------------------------------------- the cases
SIZES = (1, 2, 255, 256, 257, 2047, 2048, 2049, 4096, 4097, 16384, 16385)


def case_sizes(n1, seed=1):
    """all keys distinct: the output is the sorted input.  n < 2^24, so that LINEAR_WEIGHT's W = Float32(n) and the Float64 sum of
    W are exact whatever the order of the sum"""
    rng = np.random.default_rng([seed, n1])
    s = new_samples(rng, random_keys(rng, n1))
    s["n"] = rng.integers(1, 1 << 24, n1)
    return s


def case_bytes(seed=2, per_set=5000):
    """16 sets, one per byte of the 128-bit key: the keys of set j are one fixed pattern with byte j replaced by a random value,
    so only the radix pass of that byte tells them apart.  (The samples that draw the pattern's own byte coincide over the sets.)"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 1 << 64, 2, dtype=np.uint64)
    keys = np.tile(base, (16 * per_set, 1))
    kb = keys.view(np.uint8).reshape(-1, 16)                       # little endian: byte j of word j // 8 is radix pass j % 8
    for j in range(16):
        kb[j * per_set:(j + 1) * per_set, j] = rng.integers(0, 256, per_set)
    return new_samples(rng, keys[rng.permutation(len(keys))]), base


DIGIT_PATTERNS = ("same", "mod256", "div64", "descending", "equal")


def case_digits(pattern, seed=3):
    """Digit patterns inside a sort tile, in both words: key[1] rises with the buffer index, so the sort by key[1] sees the pattern
    in buffer order and hands the sort by key[0] the same order; key[0] repeats (16 high parts), so the pairs of one key[0] digit
    keep the order of key[1] only if the second sort is stable."""
    rng = np.random.default_rng([seed, DIGIT_PATTERNS.index(pattern)])
    n = TILE if pattern == "equal" else 3 * TILE
    i = np.arange(n, dtype=np.uint64)
    if pattern == "equal":
        keys = np.tile(rng.integers(0, 1 << 64, 2, dtype=np.uint64), (n, 1))
    elif pattern == "descending":
        k0 = np.sort(rng.integers(0, 1 << 64, n // 4, dtype=np.uint64))[::-1].repeat(4)
        k1 = np.sort(rng.integers(0, 1 << 64, n, dtype=np.uint64))[::-1]
        keys = np.stack([k0, k1], axis=1)
    else:
        low = {"same": np.full(n, 0x5A, np.uint64), "mod256": i % np.uint64(256), "div64": i // np.uint64(64)}[pattern]
        high = rng.integers(0, 1 << 56, 16, dtype=np.uint64)[rng.integers(0, 16, n)]
        keys = np.stack([(high << np.uint64(8)) | low, (i << np.uint64(8)) | low], axis=1)
    return new_samples(rng, keys)


def case_lengths(order=None, game=R.TTT, seed=40, lengths=LENGTHS):
    """One segment of every length in `lengths`, the members scattered through the buffer by a fixed permutation.  order=None: random
    keys; otherwise the segments' keys ascend in the given order of lengths, so segment j starts at sorted index sum(order[:j])."""
    rng = np.random.default_rng(seed)
    lens = np.array(lengths if order is None else order)
    nA = R.NUM_ACTIONS[game]
    if game == R.C4:
        keys = c4_keys(rng, len(lens))
    else:
        keys = random_keys(rng, len(lens))
    if order is not None:
        keys = keys[np.lexsort((keys[:, 1], keys[:, 0]))]
    s = new_samples(rng, keys.repeat(lens, axis=0), nA)
    return s[rng.permutation(len(s))]


def case_capacity(count, length, seed=5):
    """`count` segments of exactly `length` samples each, scattered"""
    return case_lengths(lengths=(length,) * count, seed=[seed, length])


def case_zeros_and_counts(seed=6):
    """Segments of 5 (k_mem_merge) and of 300 (k_mem_merge_long) samples: every z and pi[3] -0.0; the same with the second sample
    +0.0; n near 2^31, so the sum passes 2^32.  Returns the samples and the keys of the six segments, in that order, short first."""
    rng = np.random.default_rng(seed)
    keys = random_keys(rng, 6 + 40)
    lens = np.array([5, 300, 5, 300, 5, 300] + [3] * 40)
    s = new_samples(rng, keys.repeat(lens, axis=0))               # buffer order = segment order here: "the second sample" is defined
    seg = np.arange(len(lens)).repeat(lens)
    for j in range(4):
        m = np.flatnonzero(seg == j)
        s["z"][m] = -0.0
        s["pi"][m, 3] = -0.0
        if j >= 2:
            s["z"][m[1]] = 0.0
            s["pi"][m[1], 3] = 0.0
    for j in (4, 5):
        m = np.flatnonzero(seg == j)
        s["n"][m] = (1 << 31) + np.arange(len(m))
    return s, keys[:6]


def case_ring(seed=7, total=7000, distinct=600):
    """TTT-style random keys with many repeats, for a ring smaller than what is pushed"""
    rng = np.random.default_rng(seed)
    keys = random_keys(rng, distinct)[rng.integers(0, distinct, total)]
    return new_samples(rng, keys)


def case_symmetric(seed=8, n=20000):
    """Tic-tac-toe boards (not necessarily reachable): disjoint 9-bit masks of the two colours, a random side to move"""
    rng = np.random.default_rng(seed)
    w = rng.integers(0, 512, n, dtype=np.uint64)
    b = rng.integers(0, 512, n, dtype=np.uint64) & ~w
    side = np.where(rng.integers(0, 2, n) == 1, BIT63, np.uint64(0))
    return new_samples(rng, np.stack([w | side, b], axis=1))
