"""The inputs of tests/test_memory_kernels_gpu.py are sharp (oracle alone, no GPU): the generated values reveal the order of a
segment's Float64 sums, and every case has the layout -- sorted indices of segment heads, counts of long segments, digits per radix
pass -- that the GPU test relies on to reach the edges of csrc/prims.h and of k_mem_merge / k_mem_merge_long."""
import numpy as np

import azref as R
import memory_cases as MC


def _segments(s):
    """members of every segment in buffer order, keyed by position in the merged output"""
    k = s["key"]
    o = np.lexsort((np.arange(len(s)), k[:, 1], k[:, 0]))
    starts, lens = MC.layout(s)
    return [o[a:a + n] for a, n in zip(starts, lens)]


def test_sample_layout_is_the_oracles_and_the_librarys():
    import ctypes as C
    from azhip import _lib as L
    assert MC.SAMPLE.itemsize == 112 == C.sizeof(R.Sample) == C.sizeof(L.Sample)
    for name, _ in R.Sample._fields_:
        assert MC.SAMPLE.fields[name][1] == getattr(R.Sample, name).offset == getattr(L.Sample, name).offset


def test_oracle_merge_on_records_equals_a_python_fold():
    """the numpy seam hands the oracle the bytes it expects: a small mixed case against a Python-float fold in buffer order"""
    s = MC.case_lengths(lengths=(1, 2, 3, 7, 40), seed=11)
    got = MC.oracle_merge(R.TTT, s)
    segs = _segments(s)
    assert len(got) == len(segs)
    for row, m in zip(got, segs):
        acc = [float(x) for x in s["pi"][m[0]]] + [float(s["z"][m[0]]), float(s["t"][m[0]])]
        for i in m[1:]:
            acc = [a + float(b) for a, b in zip(acc, list(s["pi"][i]) + [s["z"][i], s["t"][i]])]
        acc = [a / float(len(m)) for a in acc]
        assert list(row["pi"]) + [row["z"], row["t"]] == acc and row["n"] == int(s["n"][m].sum()) and tuple(row["key"]) == tuple(s["key"][m[0]])


def test_one_swap_inside_a_segment_changes_the_merged_bits():
    """The generator's values reveal order: in the mixed-length case, swapping two members of a segment (the second and the last
    in buffer order; the first two would commute) changes the oracle's output for at least 95% of the segments of 3 or more.
    A segment of 2 cannot show it: a + b = b + a."""
    for game in (R.TTT, R.C4):
        s = MC.case_lengths(game=game)
        base = MC.words(MC.oracle_merge(game, s))
        segs = _segments(s)
        t = s.copy()
        for m in segs:
            if len(m) >= 3:
                t[[m[1], m[-1]]] = s[[m[-1], m[1]]]
        swapped = MC.words(MC.oracle_merge(game, t))
        cols = MC.live_columns(R.NUM_ACTIONS[game])
        changed = (base[:, cols] != swapped[:, cols]).any(axis=1)
        big = np.array([len(m) >= 3 for m in segs])
        assert big.sum() == 22 and changed[big].mean() >= 0.95, changed[big]
        assert not changed[~big].any()
        # no field is blind: each word is folded by a lane (wavefront) of its own on the device, and each one's sum shows the swap
        # in some segments (a swap of two same-signed values changes the rounding only now and then)
        for c in cols[2:-1]:
            assert (base[big, c] != swapped[big, c]).any(), c


def test_planned_layouts():
    assert sum(MC.LENGTHS) == 14151 and sorted(MC.ORDER_A) == sorted(MC.ORDER_B) == sorted(MC.LENGTHS)
    nlong = sum(1 for x in MC.LENGTHS if x >= MC.MERGE_LONG)
    assert nlong == 12
    for game in (R.TTT, R.C4):
        starts, lens = MC.layout(MC.case_lengths(game=game))
        assert sorted(lens) == sorted(MC.LENGTHS) and (lens >= MC.MERGE_LONG).sum() == nlong
    s = MC.case_lengths(game=R.C4)
    # Connect-Four keys: bits 0..48 and bit 63 only, key[1] without bit 63, pi[7:] zero
    assert not (s["key"][:, 0] & np.uint64(0x7FFE000000000000)).any() and not (s["key"][:, 1] >> np.uint64(49)).any() and not s["pi"][:, 7:].any()
    # scattered: no segment of 3 or more lies contiguous in the buffer
    assert all(np.ptp(m) >= len(m) for m in _segments(s) if len(m) >= 3)
    # A: a head exactly at 2048 (the 2048-segment fills tile 0), a long segment over 4096, a one-sample segment at n1 - 1
    a = MC.case_lengths(order=MC.ORDER_A, seed=41)
    starts, lens = MC.layout(a)
    assert tuple(lens) == MC.ORDER_A and (starts[0], lens[0], starts[1], lens[1]) == (0, 2048, 2048, 2049)
    assert starts[1] < 4096 < starts[1] + lens[1] and lens[1] >= MC.MERGE_LONG and (starts[-1], lens[-1]) == (len(a) - 1, 1)
    # B: a short segment over 2040..2102 (across 2048), the longest segment last, ending at n1
    b = MC.case_lengths(order=MC.ORDER_B, seed=42)
    starts, lens = MC.layout(b)
    j = list(starts).index(2040)
    assert tuple(lens) == MC.ORDER_B and lens[j] == 63 < MC.MERGE_LONG and 2040 < MC.TILE < 2040 + 63
    assert lens[-1] == 4500 and starts[-1] + 4500 == len(b) == 14151


def test_long_list_capacity_cases():
    full = MC.case_capacity(40, 256)
    starts, lens = MC.layout(full)
    assert len(full) == 10240 and (lens == 256).all() and len(lens) == 40 == len(full) // MC.MERGE_LONG     # 40 entries, a list of 41
    none = MC.case_capacity(41, 255)
    starts, lens = MC.layout(none)
    assert len(none) == 10455 and (lens == 255).all() and len(lens) == 41 and len(none) // MC.MERGE_LONG + 1 == 41


def test_sizes_case_has_distinct_keys_in_all_64_bits_and_exact_weights():
    for n1 in MC.SIZES:
        s = MC.case_sizes(n1)
        assert len(s) == n1 and len(MC.layout(s)[0]) == n1
        assert s["n"].max() < 1 << 24 and int(s["n"].sum()) < 1 << 53
        m = MC.oracle_merge(R.TTT, s)
        o = np.lexsort((s["key"][:, 1], s["key"][:, 0]))
        assert np.array_equal(MC.words(m), MC.words(s[o]))          # the output is the sorted input
        W = MC.oracle_convert(R.TTT, 2, m)[0]
        assert np.array_equal(W.astype(np.int64), m["n"])           # LINEAR_WEIGHT is integral and exact here
    s = MC.case_sizes(16385)
    for w in (0, 1):
        top = (s["key"][:, w] >> np.uint64(63)).mean()
        assert 0.45 < top < 0.55
        assert all(len(np.unique((s["key"][:, w] >> np.uint64(8 * p)) & np.uint64(255))) == 256 for p in range(8))


def test_byte_sets_differ_in_one_byte_each():
    s, base = MC.case_bytes()
    kb = np.ascontiguousarray(s["key"]).view(np.uint8).reshape(-1, 16)
    bb = base.view(np.uint8)
    diff = kb != bb
    assert len(s) == 80000 and (diff.sum(axis=1) <= 1).all()
    for j in range(16):
        rows = diff[:, j]
        assert 4900 <= rows.sum() <= 5000 and len(np.unique(kb[rows, j])) == 255      # all values but the pattern's own
    starts, lens = MC.layout(s)
    assert len(lens) == 16 * 255 + 1 and lens.max() >= MC.MERGE_LONG > np.median(lens)  # the pattern itself: ~16 x 20 samples


def test_digit_patterns():
    for p in MC.DIGIT_PATTERNS:
        s = MC.case_digits(p)
        k0, k1 = s["key"][:, 0], s["key"][:, 1]
        low0, low1 = k0 & np.uint64(255), k1 & np.uint64(255)
        if p == "equal":
            assert len(s) == MC.TILE and len(MC.layout(s)[0]) == 1
            continue
        assert len(s) == 3 * MC.TILE and len(np.unique(k1)) == len(s) and len(np.unique(k0)) <= len(s) * 2 // 3   # key[0] repeats: ties for the second sort
        if p == "descending":
            assert (k1[1:] < k1[:-1]).all() and (k0[1:] <= k0[:-1]).all()
            continue
        assert (k1[1:] > k1[:-1]).all() and np.array_equal(low0, low1)
        rows = low1.reshape(-1, 256)
        waves = low1.reshape(-1, 64)
        if p == "same":
            assert len(np.unique(low1)) == 1
        if p == "mod256":
            assert all(len(np.unique(r)) == 256 for r in rows)
        if p == "div64":
            assert all(len(np.unique(w)) == 1 for w in waves) and all(len(np.unique(r)) == 4 for r in rows)


def test_zero_and_count_segments():
    s, keys = MC.case_zeros_and_counts()
    m = MC.oracle_merge(R.TTT, s)
    NEG = np.uint64(1 << 63)
    rows = [m[(m["key"] == k).all(axis=1)][0] for k in keys]
    for j, want in ((0, NEG), (1, NEG), (2, np.uint64(0)), (3, np.uint64(0))):
        assert rows[j]["z"].view("<u8") == want and rows[j]["pi"][3].view("<u8") == want
    assert rows[4]["n"] > 1 << 32 and rows[5]["n"] > 1 << 32
    starts, lens = MC.layout(s)
    assert sorted(lens)[-3:] == [300, 300, 300] and (lens >= MC.MERGE_LONG).sum() == 3


def test_symmetric_case_merges_coinciding_images():
    s = MC.case_symmetric(n=2000)
    assert not (s["key"][:, 0] & s["key"][:, 1] & np.uint64(511)).any()
    aug = MC.oracle_augment(R.TTT, s)
    assert len(aug) == 8 * len(s)
    starts, lens = MC.layout(aug)
    assert len(lens) < len(aug) and (lens >= 2).sum() > 100
