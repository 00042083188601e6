"""merge_by_state on the device (csrc/prims.h: stable radix sort, recursive scan, tiled double sum; csrc/memory.hip: k_mem_heads,
k_mem_merge, k_mem_merge_long) against the oracle's sequential Float64 fold (oracle/azref.c azr_merge_by_state, src/memory.jl:89-114),
bit for bit, on inputs that self-play cannot produce: keys that use every byte, values whose sums reveal the order of the additions,
segment lengths around every switch of the merge kernels and sizes around every tile edge (tests/memory_cases.py; the inputs
themselves are checked in tests/test_memory_kernels_cpu.py).  Samples go up as raw az_sample records (az_memory_push_samples) and
come back through az_dataset_read; no per-sample Python."""
import ctypes as C

import numpy as np
import pytest

import azref as R
import memory_cases as MC

pytestmark = pytest.mark.gpu

CONSTANT, LOG, LINEAR = 0, 1, 2


class Built:
    """one az_dataset_create with use_position_averaging=1 over what was pushed into a fresh az_memory"""

    def __init__(self, game, pushes, capacity=None, which=0, use_symmetries=False, policy=LOG, trace_moves=0):
        from azhip import _lib as L
        self.L, self.game = L, game
        lib = L.lib()
        mem, ds = C.c_void_p(), C.c_void_p()
        cap = capacity if capacity is not None else max(1, sum(len(p) for p in pushes))
        L.check(lib.az_memory_create(game, 0, cap, C.byref(mem)))
        self.mem, self.ds = mem, None                              # the data set works on the memory's stream: the memory outlives it
        try:
            if trace_moves:                                        # az_memory_push: the only public call that advances cur_batch_size
                games, moves = (L.GameRec * 1)(), (L.MoveRec * trace_moves)()
                games[0].num_moves = trace_moves
                for m in moves:
                    for a in range(R.NUM_ACTIONS[game]):
                        m.N[a] = 1
                tb = L.TraceBuf()
                tb.games, tb.games_cap, tb.num_games, tb.moves, tb.moves_cap, tb.num_moves = games, 1, 1, moves, trace_moves, trace_moves
                L.check(lib.az_memory_push(mem, C.byref(tb), 1.0))
            for p in pushes:
                p = np.ascontiguousarray(p)
                assert p.dtype == MC.SAMPLE
                L.check(lib.az_memory_push_samples(mem, MC.vp(p), len(p)))
            L.check(lib.az_dataset_create(mem, which, 1 if use_symmetries else 0, 1, policy, C.byref(ds)))
        except Exception:
            self.close()
            raise
        self.ds = ds
        info = L.DatasetInfo()
        L.check(lib.az_dataset_get_info(ds, C.byref(info)))
        self.num_samples, self.sum_n, self.Wtot = info.num_samples, info.sum_n, info.Wtot

    def samples(self, first=0, count=None):
        count = self.num_samples - first if count is None else count
        out = np.zeros(max(count, 1), MC.SAMPLE)
        self.L.check(self.L.lib().az_dataset_read(self.ds, first, count, MC.vp(out), None, None, None, None, None))
        return out[:count]

    def tensors(self):
        n, nA = self.num_samples, R.NUM_ACTIONS[self.game]
        w, h, c = R.DIMS[self.game]
        W = np.zeros(n, np.float32); X = np.zeros((n, c, h, w), np.float32)
        A = np.zeros((n, nA), np.float32); P = np.zeros((n, nA), np.float32); V = np.zeros(n, np.float32)
        self.L.check(self.L.lib().az_dataset_read(self.ds, 0, n, None, MC.vp(W), MC.vp(X), MC.vp(A), MC.vp(P), MC.vp(V)))
        return W, X, A, P, V

    def close(self):
        if self.ds:
            self.L.lib().az_dataset_destroy(self.ds)
            self.ds = None
        if self.mem:
            self.L.lib().az_memory_destroy(self.mem)
            self.mem = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def same_bits(dev, ref, num_actions=9):
    """key, pi[:A], z, t, n as 64-bit words (so -0.0 != +0.0 and nothing rounds); pi[A:] is padding the oracle leaves alone"""
    assert len(dev) == len(ref), (len(dev), len(ref))
    cols = MC.live_columns(num_actions)
    a, b = MC.words(dev)[:, cols], MC.words(ref)[:, cols]
    if not np.array_equal(a, b):
        r, c = np.argwhere(a != b)[0]
        bad = (a != b).any(axis=1)
        raise AssertionError("%d of %d merged samples differ; first: sample %d word %d: device %#018x, oracle %#018x"
                             % (bad.sum(), len(a), r, cols[c], a[r, c], b[r, c]))


def check(game, surviving, built, policy=LOG, ref=None, with_X=False):
    """merged samples, num_samples, sum_n and (W, A, P, V) of `built` against the oracle on the samples that survive in the ring"""
    nA = R.NUM_ACTIONS[game]
    ref = MC.oracle_merge(game, surviving) if ref is None else ref
    assert built.num_samples == len(ref)
    same_bits(built.samples(), ref, nA)
    assert built.sum_n == int(surviving["n"].sum())                # Int64, exact
    W, X, A, P, V = built.tensors()
    Wr, Xr, Ar, Pr, Vr = MC.oracle_convert(game, policy, ref)
    assert np.array_equal(W, Wr) and np.array_equal(A, Ar) and np.array_equal(P, Pr) and np.array_equal(V, Vr)
    if with_X:
        assert np.array_equal(X, Xr)
    return ref


@pytest.mark.parametrize("n1", MC.SIZES)
def test_sizes_around_the_tile_edges(n1):
    """distinct keys over all 128 bits: one, two and nine sort tiles (16385: the per-pass histogram scan takes two scan tiles), last tile
    full, one short, one over.  The output is the sorted input; Wtot and sum_n are exact integers under LINEAR_WEIGHT."""
    s = MC.case_sizes(n1)
    with Built(R.TTT, [s], policy=LINEAR) as d:
        ref = check(R.TTT, s, d, policy=LINEAR)
        o = np.lexsort((s["key"][:, 1], s["key"][:, 0]))
        same_bits(ref, s[o])
        assert d.num_samples == n1 and d.Wtot == float(int(s["n"].sum()))


def test_every_key_byte_is_sorted_on():
    """16 sets of 5000 samples that differ in one byte of the key each: a wrong shift, digit mask or a dropped radix pass merges
    or misorders a set"""
    s, _ = MC.case_bytes()
    with Built(R.TTT, [s]) as d:
        check(R.TTT, s, d)


@pytest.mark.parametrize("pattern", MC.DIGIT_PATTERNS)
def test_digit_patterns_inside_a_sort_tile(pattern):
    """k_rs_scatter's ranks: a tile on one digit, rows of 256 different digits, wavefronts on one digit, descending keys, and 2048
    equal keys (one segment)"""
    s = MC.case_digits(pattern)
    with Built(R.TTT, [s]) as d:
        check(R.TTT, s, d)
        assert d.num_samples == (1 if pattern == "equal" else len(s))


@pytest.mark.parametrize("game,order,seed", [(R.TTT, None, 40), (R.C4, None, 40), (R.TTT, MC.ORDER_A, 41), (R.TTT, MC.ORDER_B, 42)],
                         ids=["ttt-scattered", "c4-scattered", "head-at-2048-one-last", "short-over-2048-long-last"])
def test_segment_lengths_around_every_switch(game, order, seed):
    """one segment of each length around 16, 64, 128, MERGE_LONG = 256, 320 = 5 x 64, 384, 2048 and 4500, the members scattered:
    k_mem_merge below 256, k_mem_merge_long from 256 (first-chunk rule, full chunks, tail loop).  The ordered layouts put a head on
    a scan-tile boundary, segments across boundaries, a one-sample segment at n1 - 1 and a long segment that ends at n1.  The
    Connect-Four case has num_actions 7 < 9 (its keys are gravity-filled boards, so X is compared too)."""
    s = MC.case_lengths(order=order, game=game, seed=seed)
    with Built(game, [s]) as d:
        ref = check(game, s, d, with_X=game == R.C4)
        assert d.num_samples == len(MC.LENGTHS) and len(s) == sum(MC.LENGTHS) and int(ref["n"].sum()) == d.sum_n


@pytest.mark.parametrize("count,length", [(40, 256), (41, 255)])
def test_long_list_at_capacity_and_empty(count, length):
    """40 segments of exactly 256 in n1 = 10240: 40 entries in a long_list of n1 / 256 + 1 = 41; 41 segments of 255: none"""
    s = MC.case_capacity(count, length)
    with Built(R.TTT, [s]) as d:
        check(R.TTT, s, d)
        assert d.num_samples == count


def test_signed_zero_and_counts_past_32_bits():
    """a sum that starts FROM the first sample keeps -0.0 (0.0 + -0.0 = +0.0 would lose it); n is summed in 64 bits; both in the short
    and in the long merge kernel"""
    s, keys = MC.case_zeros_and_counts()
    with Built(R.TTT, [s]) as d:
        check(R.TTT, s, d)
        m = d.samples()
    NEG, POS = 1 << 63, 0
    rows = [m[(m["key"] == k).all(axis=1)][0] for k in keys]
    for j, want in ((0, NEG), (1, NEG), (2, POS), (3, POS)):
        assert int(rows[j]["z"].view("<u8")) == want and int(rows[j]["pi"][3].view("<u8")) == want, j
    assert int(rows[4]["n"]) == 5 * (1 << 31) + 10 and int(rows[5]["n"]) == 300 * (1 << 31) + 299 * 150


@pytest.mark.parametrize("which", [0, 1])
def test_ring_order_after_a_wrap(which):
    """capacity 5000, 3000 + 4000 samples pushed: the surviving suffix, oldest first, is what is merged.  which=1 (last_batch): a
    trace of 1500 positions pushed first (az_memory_push) sets cur_batch_size = 1500 and is itself overwritten by the wrap, so the
    last batch is the newest 1500 samples of the ring."""
    s = MC.case_ring()
    with Built(R.TTT, [s[:3000], s[3000:]], capacity=5000, which=which, trace_moves=1500 if which else 0) as d:
        check(R.TTT, s[-1500:] if which else s[-5000:], d)


def test_symmetric_images_merge_with_their_samples():
    """20 000 boards and their 7 images each (k_mem_augment): 160 000 samples in tens of thousands of short segments, many of them
    images that coincide; the images come after all samples in buffer order, as in the oracle's augment_with_symmetries"""
    s = MC.case_symmetric()
    aug = MC.oracle_augment(R.TTT, s)
    ref = MC.oracle_merge(R.TTT, aug)
    assert len(aug) == 160000 and 10000 < len(ref) < len(aug)
    with Built(R.TTT, [s], use_symmetries=True) as d:
        check(R.TTT, aug, d, ref=ref, with_X=True)
