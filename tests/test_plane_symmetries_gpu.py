"""Declared symmetries of a plane memory (az_plane_memory_set_symmetries, az_dataset_create_from_plane_memory_sym): the build over
[samples ; images] whose images are never stored, against the SAME build over a memory into which the images were pushed as samples of
their own, gathered on the host with numpy (gather_images below; tests/test_plane_symmetries_cpu.py holds that gather and the tables of
azhip.plane_symmetries to the oracle's augment_with_symmetries).  Image k of sample i is row n0 + i * nsym + k of the sequence
(memory.jl:126-130).  Every comparison is BIT FOR BIT."""
import ctypes as C

import numpy as np
import pytest

import test_plane_memory_gpu as G
from test_plane_memory_gpu import CONSTANT, LINEAR, LOG, _bits, _vp

pytestmark = pytest.mark.gpu

C4, TTT, MANCALA, GO9 = 0, 1, 2, 3
SPECS = {C4: "ConnectFourSpec", TTT: "TicTacToeSpec", MANCALA: "MancalaSpec", GO9: "Go9PlanesSpec"}
DIMS = {C4: (3, 6, 7), TTT: (3, 3, 3), MANCALA: (5, 1, 14), GO9: (4, 9, 9)}        # (C, H, W): rows of 133, 36, 76, 406 words
NUM_ACTIONS = {C4: 7, TTT: 9, MANCALA: 6, GO9: 82}
IDS = {C4: "c4", TTT: "ttt", MANCALA: "mancala", GO9: "go9"}


# ---------------------------------------------------------------------------------------------------- helpers
def random_tables(game, nsym, seed):
    """nsym pairs of random bijections, none of them its own inverse: a scatter in place of the gather gives another result"""
    rng = np.random.default_rng(seed)
    xs, nA = int(np.prod(DIMS[game])), NUM_ACTIONS[game]

    def rows(length):
        out = []
        while len(out) < nsym:
            p = rng.permutation(length)
            if not np.array_equal(p[p], np.arange(length)):
                out.append(p)
        return np.array(out, dtype=np.int32).reshape(nsym, length)
    return rows(xs), rows(nA)


def gather_images(xperm, aperm, s):
    """augment_with_symmetries (memory.jl:114-130) over plane samples s = (X, A, pi, z, t, n): [samples ; images], image k of sample i
    at n0 + i * nsym + k, X'[w] = X[xperm[k][w]], A'[j] = A[aperm[k][j]], pi'[j] = pi[aperm[k][j]], z / t / n the sample's"""
    X, A, P, z, t, n = s
    n0, nsym = len(z), len(xperm)
    Xi = X.reshape(n0, -1)[:, xperm].reshape((n0 * nsym,) + X.shape[1:])           # [i, k, w] -> row i * nsym + k
    Ai, Pi = A[:, aperm].reshape(n0 * nsym, -1), P[:, aperm].reshape(n0 * nsym, -1)
    rep = lambda v: np.repeat(v, nsym)
    return tuple(np.concatenate(p) for p in ((X, Xi), (A, Ai), (P, Pi), (z, rep(z)), (t, rep(t)), (n, rep(n))))


def make_samples(game, n0, seed, distinct=0.7, nmax=5):
    """n0 samples over about distinct * n0 different (X, A) rows (G.make_rows / G.make_samples for any of the four geometries)"""
    rng = np.random.default_rng(seed)
    nrows, nA = max(1, int(distinct * n0)), NUM_ACTIONS[game]
    X = rng.integers(0, 3, size=(nrows,) + DIMS[game]).astype(np.float32)
    X.reshape(nrows, -1)[:, :16] = (np.arange(nrows)[:, None] >> np.arange(16)) & 1
    A = (rng.random((nrows, nA)) < 0.6).astype(np.float32)
    A[np.arange(nrows), rng.integers(0, nA, nrows)] = 1.0
    ids = rng.integers(0, nrows, n0) if nrows < n0 else rng.permutation(n0)
    P = rng.random((n0, nA)) * A[ids]
    P /= P.sum(axis=1, keepdims=True)
    return (X[ids], A[ids], P, rng.uniform(-1, 1, n0), rng.integers(1, 40, n0).astype(np.float64), rng.integers(1, nmax + 1, n0).astype(np.int64))


def new_memory(game, capacity, tables=None):
    import azhip
    mem = azhip.PlaneMemoryBuffer(getattr(azhip, SPECS[game])(), capacity)
    if tables is not None:
        mem.set_symmetries(*tables)
    return mem


def read(d):
    return (d.num_samples, d.sum_n, d.Wtot, d.Wmean, d.Hp), d.tensors()


def assert_same_dataset(a, b, what):
    (ia, ta), (ib, tb) = a, b
    print(what, "declared", ia, "pushed", ib)
    assert ia == ib, what
    for name, x, y in zip("WXAPV", ta, tb):
        assert x.shape == y.shape and np.array_equal(_bits(x), _bits(y)), (what, name)


def compare_builds(memA, memB, last_batch=False, policies=(CONSTANT, LOG, LINEAR)):
    """memA with the symmetries declared against memB holding [samples ; images]"""
    for policy in policies:
        for merge in (False, True):
            with memA.dataset(last_batch=last_batch, use_symmetries=True, use_position_averaging=merge, weighing_policy=policy) as da, \
                    memB.dataset(use_position_averaging=merge, weighing_policy=policy) as db:
                assert_same_dataset(read(da), read(db), (last_batch, merge, policy))


# ---------------------------------------------------------------------------------------------------- 1. declared == pushed
@pytest.mark.parametrize("nsym", [1, 7, 15])
@pytest.mark.parametrize("n0", [1, 3, 37, 257, 2049])
@pytest.mark.parametrize("game", [TTT, MANCALA, C4, GO9], ids=[IDS[g] for g in (TTT, MANCALA, C4, GO9)])
def test_declared_symmetries_are_pushed_images(game, n0, nsym):
    xperm, aperm = random_tables(game, nsym, seed=1000 * game + nsym)
    for p in list(xperm) + list(aperm):
        assert sorted(p) == list(range(len(p))) and not np.array_equal(p[p], np.arange(len(p)))       # a bijection; scatter != gather
    s = make_samples(game, n0, seed=n0 + game)
    memA, memB = new_memory(game, n0, (xperm, aperm)), new_memory(game, n0 * (1 + nsym))
    assert (memA.num_symmetries, memB.num_symmetries) == (nsym, 0)
    memA.push_samples(*s)
    memB.push_samples(*gather_images(xperm, aperm, s))
    compare_builds(memA, memB)
    with memA.dataset(use_symmetries=True, use_position_averaging=True, weighing_policy=LINEAR) as d:
        assert d.sum_n == (1 + nsym) * int(s[5].sum()) and d.num_samples <= n0 * (1 + nsym)
        if n0 > 3:
            assert d.num_samples < n0 * (1 + nsym)                   # the repeated rows and their images did merge
    # use_symmetries = 0 through the new entry point is the old entry point
    with memA.dataset(use_position_averaging=True, weighing_policy=LOG) as d0:
        from azhip import _lib as L
        h = C.c_void_p()
        L.check(L.lib().az_dataset_create_from_plane_memory(memA._h, 0, 1, LOG, C.byref(h)))
        import azhip
        with azhip.TensorDataset._adopt(memA.gspec, h) as d1:
            assert_same_dataset(read(d0), read(d1), "use_symmetries=0")
    memA.close()
    memB.close()


# ---------------------------------------------------------------------------------------------------- 2. ring and batch
def test_a_wrapped_ring_and_the_last_batch():
    """capacity 100 after 250 samples: the selection starts at sample 150 = slot 50 and crosses slot 0; then which = 1 over a batch of
    two traces that crosses it again"""
    game, nsym = MANCALA, 7
    tables = random_tables(game, nsym, seed=5)
    s = make_samples(game, 250, seed=6)
    memA = new_memory(game, 100, tables)
    for k in range(0, 250, 50):
        memA.push_samples(*[a[k:k + 50] for a in s])
    assert len(memA) == 100
    kept = tuple(a[150:] for a in s)
    for a, b in zip(memA.samples(), kept):
        assert np.array_equal(a, b)
    memB = new_memory(game, 100 * (1 + nsym))
    memB.push_samples(*gather_images(*tables, kept))
    compare_builds(memA, memB, policies=(LINEAR,))
    memB.close()
    rng = np.random.default_rng(7)
    memA.push_trace(s[0][:30], s[1][:30], s[2][:30], rng.integers(-1, 2, 30).astype(np.float64), rng.integers(0, 2, 30).astype(np.uint8), 0.9)
    memA.new_batch()
    for lo, hi in ((30, 70), (70, 95)):                               # 65 samples after 280 pushed: slots 80 .. 99, 0 .. 44
        memA.push_trace(s[0][lo:hi], s[1][lo:hi], s[2][lo:hi], rng.integers(-1, 2, hi - lo).astype(np.float64), rng.integers(0, 2, hi - lo).astype(np.uint8), 0.9)
    assert (len(memA), memA.cur_batch_size()) == (100, 65)
    batch = tuple(a[-65:] for a in memA.samples())
    memB = new_memory(game, 65 * (1 + nsym))
    memB.push_samples(*gather_images(*tables, batch))
    compare_builds(memA, memB, last_batch=True, policies=(LOG,))
    whole = new_memory(game, 100 * (1 + nsym))
    whole.push_samples(*gather_images(*tables, memA.samples()))
    compare_builds(memA, whole, policies=(CONSTANT,))
    for m in (memA, memB, whole):
        m.close()


# ---------------------------------------------------------------------------------------------------- 3. groups across originals and images
def test_a_sample_that_is_its_own_image_under_every_symmetry():
    import azhip
    gspec = azhip.Go9PlanesSpec()
    xperm, aperm = azhip.plane_symmetries(gspec)
    nsym = len(xperm)
    rng = np.random.default_rng(8)
    X, A = np.full((1, 4, 9, 9), 2.0, dtype=np.float32), np.ones((1, 82), dtype=np.float32)
    P = rng.random((1, 82))
    P /= P.sum()
    mem = azhip.PlaneMemoryBuffer(gspec, 4)
    mem.set_symmetries(xperm, aperm)
    mem.push_samples(X, A, P, [0.25], [3.0], [5])
    with mem.dataset(use_symmetries=True, use_position_averaging=True, weighing_policy=LINEAR) as d:
        W, gX, gA, gP, gV = d.tensors()
        assert (d.num_samples, d.sum_n) == (1, 5 * (1 + nsym)) and W[0] == np.float32(5 * (1 + nsym))
        acc = P[0].copy()
        for k in range(nsym):
            acc += P[0][aperm[k]]
        assert np.array_equal(_bits(gP[0]), _bits((acc / np.float64(1 + nsym)).astype(np.float32)))
        assert np.array_equal(gX, X) and np.array_equal(gA, A) and gV[0] == np.float32(0.25)
    with mem.dataset(use_symmetries=True) as d:
        assert (d.num_samples, d.sum_n) == (1 + nsym, 5 * (1 + nsym))
    mem.close()


def test_an_original_that_equals_an_earlier_sample_s_image_sums_in_augmented_buffer_order():
    """samples j = 4 and l = 6 carry the row of image k = 2 of sample i = 1: the group is (4, 6, n0 + 1 * nsym + 2) in that order, since
    4 < 6 < n0 + i * nsym + k.  Three members, so the Float64 sums tell the order; -0.0 in X and in every member's z."""
    game, nsym, n0, i, j, l, k = GO9, 3, 8, 1, 4, 6, 2
    xperm, aperm = random_tables(game, nsym, seed=9)
    X, A, P, z, t, n = [a.copy() for a in make_samples(game, n0, seed=10, distinct=1.0)]
    X[i].reshape(-1)[100] = -0.0
    for m in (j, l):
        X[m], A[m] = X[i].reshape(-1)[xperm[k]].reshape(X[i].shape), A[i][aperm[k]]
    rng = np.random.default_rng(11)
    for m in (j, l):
        P[m] = rng.random(82) * A[m]
        P[m] /= P[m].sum()
    z[[i, j, l]] = -0.0
    s = (X, A, P, z, t, n)
    assert np.signbit(X[j].reshape(-1)).sum() == 1
    aug = gather_images(xperm, aperm, s)
    es = [tuple(a[r] for a in aug) for r in range(len(aug[3]))]
    want = G.ref_merge(es)                                           # the numpy loop: groups by row bytes, sums one by one in list order
    assert len(want) == n0 * (1 + nsym) - 2 - nsym                  # and image k' of j IS image k' of l, for every k'
    img = n0 + i * nsym + k
    row = want[j]                                                    # first occurrence: position j (no earlier rows merged)
    assert np.array_equal(row[0], X[j]) and row[5] == n[j] + n[l] + n[i]
    pim = P[i][aperm[k]]
    assert np.array_equal(row[2], ((P[j] + P[l]) + pim) / 3.0) and not np.array_equal(row[2], ((P[j] + pim) + P[l]) / 3.0)
    assert np.array_equal(aug[2][img], pim)
    mem = new_memory(game, n0, (xperm, aperm))
    mem.push_samples(*s)
    for policy in (CONSTANT, LINEAR):
        with mem.dataset(use_symmetries=True, use_position_averaging=True, weighing_policy=policy) as d:
            got = d.tensors()
            assert d.num_samples == len(want) and d.sum_n == (1 + nsym) * int(n.sum())
            for name, g, w in zip("WXAPV", got, G.ref_convert(want, policy)):
                assert np.array_equal(_bits(g), _bits(w)), (name, policy)
            assert np.signbit(got[4][j]) and got[4][j] == 0.0 and np.signbit(got[1][j].reshape(-1)).sum() == 1
    mem.close()


# ---------------------------------------------------------------------------------------------------- 4. the keyed path
def _positions(game, ngames):
    """state keys of random games played by the CPU oracle (G._ttt_positions for either game)"""
    import azref as R
    keys = []
    for g in range(ngames):
        rng = np.random.default_rng(100 + g)
        env = R.Game(game)
        while not env.terminated():
            keys.append(env.key())
            env.play(rng.choice(env.available_actions()))
    return np.array(keys, dtype=np.uint64)


@pytest.mark.parametrize("game", [TTT, C4], ids=["ttt", "c4"])
def test_conventions_against_the_keyed_memory(game):
    """real positions by key into az_memory (whose device twin knows GI.symmetries and is held to the oracle) and by their planes into
    a plane memory with azhip.plane_symmetries declared: unmerged the same tensors in the same order, merged the same rows"""
    import azhip
    from azhip import _lib as L
    keys = _positions(game, 40 if game == TTT else 12)
    rng = np.random.default_rng(12)
    keys = keys[rng.permutation(len(keys))]
    n, nA = len(keys), NUM_ACTIONS[game]
    assert n > 200
    gspec = getattr(azhip, SPECS[game])()
    with azhip.Engine(game=game, oracle=azhip.ORACLE_HASH, num_workers=8, batch_size=8, num_iters_per_turn=2) as e:
        X, A = e.encode(keys)
    P = rng.random((n, nA)) * A
    P /= P.sum(axis=1, keepdims=True)
    z, t, nv = rng.uniform(-1, 1, n), rng.integers(1, 10, n).astype(np.float64), rng.integers(1, 301, n).astype(np.int64)
    raw = (L.Sample * n)()
    for i in range(n):
        raw[i].key[0], raw[i].key[1] = int(keys[i, 0]), int(keys[i, 1])
        for a in range(nA):
            raw[i].pi[a] = P[i, a]
        raw[i].z, raw[i].t, raw[i].n = z[i], t[i], int(nv[i])
    kmem = azhip.MemoryBuffer(gspec, n)
    L.check(L.lib().az_memory_push_samples(kmem._h, raw, n))
    pmem = azhip.PlaneMemoryBuffer(gspec, n)
    xperm, aperm = azhip.plane_symmetries(gspec)
    assert len(xperm) == (7 if game == TTT else 1)
    pmem.set_symmetries(xperm, aperm)
    pmem.push_samples(X, A, P, z, t, nv)
    with kmem.dataset(use_symmetries=True, weighing_policy=LINEAR) as kd, pmem.dataset(use_symmetries=True, weighing_policy=LINEAR) as pd:
        assert len(kd) == len(pd) == n * (1 + len(xperm)) and kd.sum_n == pd.sum_n
        for name, a, b in zip("WXAPV", kd.tensors(), pd.tensors()):
            assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), name
    with kmem.dataset(use_symmetries=True, use_position_averaging=True, weighing_policy=LOG) as kd, \
            pmem.dataset(use_symmetries=True, use_position_averaging=True, weighing_policy=LOG) as pd:
        assert len(kd) == len(pd) < n * (1 + len(xperm)) and kd.sum_n == pd.sum_n == (1 + len(xperm)) * int(nv.sum())
        rows = lambda ts: np.concatenate([_bits(np.ascontiguousarray(x.reshape(len(x), -1))) for x in ts], axis=1)
        assert sorted(map(bytes, rows(kd.tensors()))) == sorted(map(bytes, rows(pd.tensors())))
    kmem.close()
    pmem.close()


# ---------------------------------------------------------------------------------------------------- 5. collisions
def test_a_hash_collision_among_virtual_rows_is_an_error():
    from azhip import _lib as L
    f = L.lib().az_debug_plane_memory_hash_bits
    f.argtypes, f.restype = [C.c_void_p, C.c_int32], C.c_int
    tables = random_tables(GO9, 3, seed=13)
    s = make_samples(GO9, 50, seed=14, distinct=1.0)
    mem = new_memory(GO9, 64, tables)
    mem.push_samples(*s)
    L.check(f(mem._h, 4))                                            # 200 distinct virtual rows on 16 keys
    with pytest.raises(L.AzError, match="plane hash collision") as ei:
        mem.dataset(use_symmetries=True, use_position_averaging=True)
    assert ei.value.status == L.AZ_ERR_STATE
    L.check(f(mem._h, 128))
    with mem.dataset(use_symmetries=True, use_position_averaging=True) as d:
        assert len(d) == 200
    mem.close()


# ---------------------------------------------------------------------------------------------------- 6. training
def test_trainer_over_a_plane_memory_with_symmetries():
    import azhip
    gspec = azhip.Go9PlanesSpec()
    tables = azhip.plane_symmetries(gspec)
    s = make_samples(GO9, 64, seed=15)
    memA, memB = new_memory(GO9, 64, tables), new_memory(GO9, 64 * 8)
    memA.push_samples(*s)
    memB.push_samples(*gather_images(*tables, s))
    hp = azhip.ResNetHP(num_blocks=1, num_filters=64, num_policy_head_filters=32, num_value_head_filters=32)
    nn = azhip.ResNet(gspec, hp, seed=7)
    kw = dict(samples_weighing_policy=LOG, l2_regularization=1e-4, loss_computation_batch_size=64, batch_size=64)
    with azhip.Trainer(gspec, nn, memA, azhip.LearningParams(use_position_averaging=True, **kw), use_symmetries=True) as tra, \
            memB.dataset(use_position_averaging=True, weighing_policy=LOG) as bd, \
            azhip.Trainer(gspec, nn, bd, azhip.LearningParams(use_position_averaging=False, **kw)) as trb:
        assert isinstance(tra.data, azhip.TensorDataset) and tra.num_samples() == trb.num_samples() == len(bd) and len(bd) > 64
        la, lb = tra.batch_updates(2, seed=3), trb.batch_updates(2, seed=3)
        print("losses", la, lb)
        assert np.all(np.isfinite(la)) and np.array_equal(_bits(la), _bits(lb))
        assert np.array_equal(_bits(tra.trained_params()), _bits(trb.trained_params()))
    with pytest.raises(ValueError, match="use_symmetries"):
        azhip.Trainer(gspec, nn, memB, azhip.LearningParams(**kw), use_symmetries=True)
    with pytest.raises(ValueError, match="was made for"):
        azhip.Trainer(azhip.TicTacToeSpec(), nn, memB, azhip.LearningParams(**kw))
    memA.close()
    memB.close()


# ---------------------------------------------------------------------------------------------------- 7. bad calls
def test_bad_calls_leave_the_declared_set_intact():
    import azhip
    from azhip import _lib as L
    lib = L.lib()
    xs, nA = 324, 82
    good = random_tables(GO9, 3, seed=16)
    mem = new_memory(GO9, 8, good)
    s = make_samples(GO9, 8, seed=17)
    mem.push_samples(*s)                                             # on a full memory too: the symmetries are the game's
    with mem.dataset(use_symmetries=True, use_position_averaging=True, weighing_policy=LINEAR) as d:
        before = read(d)

    def refused(nsym, xperm, aperm, message):
        assert lib.az_plane_memory_set_symmetries(mem._h, nsym, _vp(xperm), _vp(aperm)) == L.AZ_ERR_BAD_ARG
        assert message in lib.az_last_error().decode(), lib.az_last_error().decode()
        assert mem.num_symmetries == 3
    ident = (np.tile(np.arange(xs, dtype=np.int32), (2, 1)), np.tile(np.arange(nA, dtype=np.int32), (2, 1)))
    refused(-1, *ident, "nsym must be in 0..15")
    refused(16, np.tile(ident[0][:1], (16, 1)), np.tile(ident[1][:1], (16, 1)), "nsym must be in 0..15")
    refused(2, None, ident[1], "NULL xperm table")
    refused(2, ident[0], None, "NULL aperm table")
    for table, length, name in ((0, xs, "xperm"), (1, nA, "aperm")):
        for value, what in ((length, "is outside 0..%d" % (length - 1)), (-1, "is outside 0..%d" % (length - 1))):
            bad = [a.copy() for a in ident]
            bad[table][1, 5] = value
            refused(2, *bad, "symmetry 1: %s[5] = %d %s" % (name, value, what))
        bad = [a.copy() for a in ident]
        bad[table][1, 9] = 4                                         # index 9 takes the source index 4 already took
        refused(2, *bad, "symmetry 1: %s[9] = 4 repeats the source of %s[4]" % (name, name))
    with mem.dataset(use_symmetries=True, use_position_averaging=True, weighing_policy=LINEAR) as d:
        assert_same_dataset(read(d), before, "after the refusals")
    with pytest.raises(ValueError, match="xperm must have shape"):
        mem.set_symmetries(ident[0][:, :300], ident[1])
    with pytest.raises(ValueError, match="aperm must have shape"):
        mem.set_symmetries(ident[0], ident[1][:1])
    assert mem.num_symmetries == 3
    # NULL memory, NULL result
    k, h = C.c_int32(), C.c_void_p()
    assert lib.az_plane_memory_set_symmetries(None, 0, None, None) == L.AZ_ERR_BAD_ARG
    assert lib.az_plane_memory_num_symmetries(None, C.byref(k)) == L.AZ_ERR_BAD_ARG and lib.az_plane_memory_num_symmetries(mem._h, None) == L.AZ_ERR_BAD_ARG
    assert lib.az_dataset_create_from_plane_memory_sym(None, 0, 1, 0, 0, C.byref(h)) == L.AZ_ERR_BAD_ARG
    assert lib.az_dataset_create_from_plane_memory_sym(mem._h, 0, 1, 0, 0, None) == L.AZ_ERR_BAD_ARG
    assert lib.az_dataset_create_from_plane_memory_sym(mem._h, 2, 1, 0, 0, C.byref(h)) == L.AZ_ERR_BAD_ARG and "which must be" in lib.az_last_error().decode()
    assert lib.az_dataset_create_from_plane_memory_sym(mem._h, 0, 1, 0, 3, C.byref(h)) == L.AZ_ERR_BAD_ARG and not h.value
    # an identity permutation is a symmetry like another (the reference does not refuse one): every sample merges with its image
    mem.set_symmetries(ident[0][:1], ident[1][:1])
    with mem.dataset(use_symmetries=True, use_position_averaging=True) as d, mem.dataset(use_position_averaging=True) as d0:
        assert mem.num_symmetries == 1 and len(d) == len(d0) and d.sum_n == 2 * d0.sum_n
    # nsym = 0 clears, with or without tables; use_symmetries is then refused by the library and by the Python mirror
    for args in ((None, None), (ident[0][:0], ident[1][:0])):
        mem.set_symmetries(*good)
        assert lib.az_plane_memory_set_symmetries(mem._h, 0, _vp(args[0]), _vp(args[1])) == L.AZ_OK and mem.num_symmetries == 0
    assert lib.az_dataset_create_from_plane_memory_sym(mem._h, 0, 1, 1, 0, C.byref(h)) == L.AZ_ERR_BAD_ARG and not h.value
    assert "no symmetries were declared for this memory" in lib.az_last_error().decode()
    with pytest.raises(ValueError, match="use_symmetries"):
        mem.dataset(use_symmetries=True)
    mem.set_symmetries(np.zeros((0, xs)), np.zeros((0, nA)))
    with mem.dataset(use_position_averaging=True) as d:
        assert len(d) == len(d0)
    # declared on an empty memory, before any sample
    empty = azhip.PlaneMemoryBuffer(azhip.MancalaSpec(), 4)
    empty.set_symmetries(*random_tables(MANCALA, 15, seed=18))
    assert empty.num_symmetries == 15
    assert lib.az_dataset_create_from_plane_memory_sym(empty._h, 0, 1, 0, 0, C.byref(h)) == L.AZ_ERR_STATE and "empty" in lib.az_last_error().decode()
    assert azhip.plane_symmetries(azhip.MancalaSpec())[0].shape == (0, 70)
    empty.set_symmetries(*azhip.plane_symmetries(azhip.MancalaSpec()))
    assert empty.num_symmetries == 0
    empty.close()
    mem.close()
