"""az_plane_memory_*: the replay memory of a host-stepped game (planes, mask, pi, z, t, n per sample) and the data set built from it
on the device (az_dataset_create_from_plane_memory), against a numpy restatement of MemoryBuffer / push_trace! / merge_by_state
(src/memory.jl:35-112) and convert_samples (src/learning.jl:17-51) over rows.

The restatement (RefMemory, ref_merge, ref_convert below) does what the header states: a state is a bit-identical (X, A) row, a
merged row's pi / z / t are Float64 sums taken one by one in buffer order starting from the first sample, divided by the count, n
is summed, rows come out in order of first occurrence, P = Float32(pi), V = Float32(z).  Every comparison with it is BIT FOR BIT.
tests/test_plane_memory_cpu.py holds the restatement itself to the oracle's merge_by_state.  LOG_WEIGHT's W is not restated in numpy:
it is pinned against the keyed path (az_memory + az_dataset_create), which the oracle validates."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TTT, MANCALA, GO9 = 1, 2, 3
SPECS = {1: "TicTacToeSpec", 2: "MancalaSpec", 3: "Go9PlanesSpec"}
DIMS = {1: (3, 3, 3), 2: (5, 1, 14), 3: (4, 9, 9)}            # (C, H, W)
NUM_ACTIONS = {1: 9, 2: 6, 3: 82}
CONSTANT, LOG, LINEAR = 0, 1, 2


# ---------------------------------------------------------------------------------------------------- the numpy restatement
class RefMemory:
    """MemoryBuffer (memory.jl:35-65) over samples (X, A, pi, z, t, n): a circular buffer, cur_batch_size advanced by push_trace"""

    def __init__(self, capacity):
        self.capacity, self.pushed, self.cur = capacity, [], 0

    def push(self, X, A, pi, z, t, n=1):
        self.pushed.append((np.array(X, dtype=np.float32), np.array(A, dtype=np.float32), np.array(pi, dtype=np.float64), float(z), float(t), int(n)))

    def push_trace(self, X, A, P, rewards, white_playing, gamma):
        """push_trace! (memory.jl:74-87): the last position first"""
        n, wr = len(rewards), 0.0
        for i in reversed(range(n)):
            wr = gamma * wr + float(rewards[i])
            self.push(X[i], A[i], P[i], wr if white_playing[i] else -wr, float(n - i), 1)
        self.cur += n

    def __len__(self):
        return min(len(self.pushed), self.capacity)

    def cur_batch_size(self):
        return min(self.cur, len(self))                              # memory.jl:53

    def get_experience(self):
        return self.pushed[len(self.pushed) - len(self):]             # oldest first

    def last_batch(self):
        return self.get_experience()[len(self) - self.cur_batch_size():]


def ref_merge(samples):
    """merge_by_state (memory.jl:89-112) with the (X, A) row's bytes as the state; a dict keeps the order of first insertion"""
    groups = {}
    for e in samples:
        groups.setdefault(e[0].tobytes() + e[1].tobytes(), []).append(e)
    out = []
    for es in groups.values():
        pi, z, t, n = es[0][2].copy(), np.float64(es[0][3]), np.float64(es[0][4]), es[0][5]
        for e in es[1:]:
            pi += e[2]
            z = z + np.float64(e[3])
            t = t + np.float64(e[4])
            n += e[5]
        cnt = np.float64(len(es))
        out.append((es[0][0], es[0][1], pi / cnt, z / cnt, t / cnt, n))
    return out


def ref_convert(samples, policy):
    """convert_samples (learning.jl:17-51); LOG_WEIGHT is pinned elsewhere (module docstring)"""
    assert policy in (CONSTANT, LINEAR)
    W = np.array([1.0 if policy == CONSTANT else float(e[5]) for e in samples], dtype=np.float32)
    X = np.stack([e[0] for e in samples])
    A = np.stack([e[1] for e in samples])
    P = np.stack([e[2] for e in samples]).astype(np.float32)
    V = np.array([e[3] for e in samples], dtype=np.float64).astype(np.float32)
    return W, X, A, P, V


# ---------------------------------------------------------------------------------------------------- helpers
def _vp(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def make_rows(game, nrows, seed):
    """nrows DISTINCT (X, A) rows: small integers in the planes, a mask with at least one legal action"""
    rng = np.random.default_rng(seed)
    nA = NUM_ACTIONS[game]
    X = rng.integers(0, 3, size=(nrows,) + DIMS[game]).astype(np.float32)
    X.reshape(nrows, -1)[:, :16] = (np.arange(nrows)[:, None] >> np.arange(16)) & 1      # the row's number in binary: no two alike
    A = (rng.random((nrows, nA)) < 0.6).astype(np.float32)
    A[np.arange(nrows), rng.integers(0, nA, nrows)] = 1.0
    return X, A


def make_samples(game, row_of_sample, X, A, seed, nmax=5):
    """one sample per entry of row_of_sample: pi over the row's legal actions, z, t, n"""
    rng = np.random.default_rng(seed)
    ids = np.asarray(row_of_sample)
    n = len(ids)
    P = rng.random((n, NUM_ACTIONS[game])) * A[ids]
    P /= P.sum(axis=1, keepdims=True)
    return (X[ids], A[ids], P, rng.uniform(-1, 1, n), rng.integers(1, 40, n).astype(np.float64), rng.integers(1, nmax + 1, n).astype(np.int64))


def push_both(mem, ref, s, lo=0, hi=None):
    X, A, P, z, t, n = [a[lo:hi] for a in s]
    mem.push_samples(X, A, P, z, t, n)
    for i in range(len(z)):
        ref.push(X[i], A[i], P[i], z[i], t[i], n[i])


def check_dataset(mem, ref, last_batch, merge, policy):
    """the device's data set == the restatement's, bit for bit, and its sums == those of a data set made from the same tensors"""
    import azhip
    es = ref.last_batch() if last_batch else ref.get_experience()
    if merge:
        es = ref_merge(es)
    want = ref_convert(es, policy)
    with mem.dataset(last_batch=last_batch, use_position_averaging=merge, weighing_policy=policy) as d:
        assert isinstance(d, azhip.TensorDataset)
        got = d.tensors()
        assert len(d) == d.num_samples == len(es) and d.sum_n == sum(e[5] for e in es)
        for name, g, w in zip("WXAPV", got, want):
            assert g.shape == w.shape and np.array_equal(_bits(g), _bits(w)), (name, last_batch, merge, policy)
        with azhip.TensorDataset(mem.gspec, *want) as td:
            assert (d.Wtot, d.Wmean, d.Hp) == (td.Wtot, td.Wmean, td.Hp)
    return got


def new_pair(game, capacity):
    import azhip
    return azhip.PlaneMemoryBuffer(getattr(azhip, SPECS[game])(), capacity), RefMemory(capacity)


# ---------------------------------------------------------------------------------------------------- 1. geometries
@pytest.mark.parametrize("count", [1, 63, 64, 65, 2049])
@pytest.mark.parametrize("game", [TTT, MANCALA, GO9], ids=["ttt", "mancala", "go9"])
def test_geometries_policies_and_sizes(game, count):
    """half the samples by push_samples (with n), the rest as one trace (the batch), about 30 % duplicates"""
    X, A = make_rows(game, max(1, int(0.7 * count)), seed=count)
    rng = np.random.default_rng(100 + count)
    s = make_samples(game, rng.integers(0, len(X), count), X, A, seed=game)
    k = count // 2
    mem, ref = new_pair(game, 4096)
    push_both(mem, ref, s, 0, k)
    rewards, wp = rng.integers(-1, 2, count - k).astype(np.float64), rng.integers(0, 2, count - k).astype(np.uint8)
    mem.push_trace(s[0][k:], s[1][k:], s[2][k:], rewards, wp, 0.9)
    ref.push_trace(s[0][k:], s[1][k:], s[2][k:], rewards, wp, 0.9)
    assert (len(mem), mem.cur_batch_size()) == (len(ref), ref.cur_batch_size()) == (count, count - k)
    for policy in (CONSTANT, LINEAR):
        for last_batch in (False, True):
            for merge in (False, True):
                check_dataset(mem, ref, last_batch, merge, policy)
    mem.close()


# ---------------------------------------------------------------------------------------------------- 2. groups
def _run_groups(game, ids, X, A, capacity=None, policy=LINEAR):
    s = make_samples(game, ids, X, A, seed=len(ids))
    mem, ref = new_pair(game, capacity or len(ids))
    push_both(mem, ref, s)
    got = check_dataset(mem, ref, False, True, policy)
    check_dataset(mem, ref, False, False, policy)
    mem.close()
    return got


def test_groups_all_distinct_all_identical_pairs_and_one_of_300():
    X, A = make_rows(GO9, 700, seed=1)
    rng = np.random.default_rng(2)
    assert len(_run_groups(GO9, rng.permutation(700), X, A)[0]) == 700             # all rows distinct
    assert len(_run_groups(GO9, np.zeros(5000, dtype=int), X, A)[0]) == 1           # one group of 5000
    assert len(_run_groups(GO9, rng.permutation(np.repeat(np.arange(350), 2)), X, A)[0]) == 350      # groups of two
    ids = rng.permutation(np.concatenate([np.full(300, 7), np.arange(100, 500)]))    # a group of 300 among singles
    got = _run_groups(GO9, ids, X, A)
    assert len(got[0]) == 401 and got[0].max() == np.float32(make_samples(GO9, ids, X, A, seed=len(ids))[5][ids == 7].sum())


def test_groups_straddle_the_wrap_point():
    """capacity 100, 250 samples pushed as 5 traces: length and cur_batch_size as memory.jl:54-56, groups on both sides of slot 0"""
    X, A = make_rows(MANCALA, 30, seed=3)
    rng = np.random.default_rng(4)
    s = make_samples(MANCALA, rng.integers(0, 30, 250), X, A, seed=5)
    mem, ref = new_pair(MANCALA, 100)
    for g in range(5):
        sl = slice(50 * g, 50 * g + 50)
        r, wp = rng.integers(-1, 2, 50).astype(np.float64), rng.integers(0, 2, 50).astype(np.uint8)
        mem.push_trace(s[0][sl], s[1][sl], s[2][sl], r, wp, 1.0)
        ref.push_trace(s[0][sl], s[1][sl], s[2][sl], r, wp, 1.0)
        assert (len(mem), mem.cur_batch_size()) == (len(ref), ref.cur_batch_size())
    assert (len(mem), mem.cur_batch_size()) == (100, 100)
    for merge in (False, True):
        check_dataset(mem, ref, False, merge, LINEAR)
    mem.new_batch()
    ref.cur = 0
    sl = slice(0, 30)
    mem.push_trace(s[0][sl], s[1][sl], s[2][sl], np.ones(30), np.ones(30, dtype=np.uint8), 1.0)
    ref.push_trace(s[0][sl], s[1][sl], s[2][sl], np.ones(30), np.ones(30, dtype=np.uint8), 1.0)
    assert (len(mem), mem.cur_batch_size()) == (100, 30) == (len(ref), ref.cur_batch_size())
    for last_batch in (False, True):
        assert len(check_dataset(mem, ref, last_batch, True, CONSTANT)[0]) <= 30
    # a single push larger than the buffer keeps its newest samples
    push_both(mem, ref, s)
    assert (len(mem), mem.cur_batch_size()) == (100, 30)
    check_dataset(mem, ref, False, True, LINEAR)
    mem.empty()
    assert (len(mem), mem.cur_batch_size()) == (0, 0)
    mem.close()


@pytest.mark.parametrize("game", [TTT, GO9], ids=["ttt", "go9"])
def test_rows_that_look_alike_stay_apart(game):
    """equal X with different A (the LAST mask word included), a difference in the last plane word only, 0.0 against -0.0"""
    X0, A0 = make_rows(game, 1, seed=6)
    X0[0].reshape(-1)[-1] = 0.0
    A0[0, -1], A0[0, 0] = 0.0, 1.0
    X, A = np.repeat(X0, 5, axis=0), np.repeat(A0, 5, axis=0)
    A[1, -1] = 1.0                                                   # row 1: the mask's last word
    A[2, 1] = 1.0 - A[2, 1]                                          # row 2: another mask word (a legal action remains: A[., 0] = 1)
    X[3].reshape(-1)[-1] = 1.0                                       # row 3: the last plane word
    X[4].reshape(-1)[-1] = -0.0                                      # row 4: -0.0 where row 0 has 0.0
    ids = np.array([0, 1, 2, 3, 4, 4, 3, 2, 1, 0, 0, 4])
    got = _run_groups(game, ids, X, A)
    assert len(got[0]) == 5
    assert np.signbit(got[1][4].reshape(-1)[-1]) and not np.signbit(got[1][0].reshape(-1)[-1])


# ---------------------------------------------------------------------------------------------------- 3. push_trace
def _ttt_game(seed):
    """a random Tic-tac-toe game played by the CPU oracle: keys, planes, masks, white's rewards, who moved"""
    import azref as R
    rng = np.random.default_rng(seed)
    g = R.Game(R.TTT)
    keys, X, A, rewards, wp = [], [], [], [], []
    while not g.terminated():
        keys.append(g.key()); X.append(g.vectorize().reshape(3, 3, 3)); A.append(g.actions_mask().astype(np.float32)); wp.append(g.white_playing())
        g.play(rng.choice(g.available_actions()))
        rewards.append(float(g.white_reward()))
    return keys, np.stack(X), np.stack(A), np.array(rewards), np.array(wp, dtype=np.uint8)


@pytest.mark.parametrize("gamma", [1.0, 0.9])
def test_push_trace_z_t_and_order(gamma):
    """a Go-geometry trace with a free turn (white moves twice running) and rewards along the way"""
    X, A = make_rows(GO9, 7, seed=8)
    s = make_samples(GO9, np.arange(7), X, A, seed=9)
    wp = np.array([1, 0, 1, 1, 0, 1, 0], dtype=np.uint8)
    rewards = np.array([0.0, 0.5, 0.0, -0.25, 0.0, 0.0, 1.0])
    mem, ref = new_pair(GO9, 16)
    mem.push_trace(s[0], s[1], s[2], rewards, wp, gamma)
    ref.push_trace(s[0], s[1], s[2], rewards, wp, gamma)
    gX, gA, gP, gz, gt, gn = mem.samples()
    want = ref.get_experience()
    assert np.array_equal(gX, s[0][::-1]) and np.array_equal(gA, s[1][::-1])        # the last position was pushed first
    assert np.array_equal(_bits(gP), _bits(np.stack([e[2] for e in want])))
    assert np.array_equal(_bits(gz), _bits(np.array([e[3] for e in want])))
    assert list(gt) == [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0] == [e[4] for e in want] and list(gn) == [1] * 7
    assert mem.cur_batch_size() == 7
    check_dataset(mem, ref, True, False, CONSTANT)
    mem.close()


def test_push_trace_agrees_with_az_push_trace_on_tictactoe():
    from azhip import _lib as L
    keys, X, A, rewards, wp = _ttt_game(11)
    n = len(keys)
    moves = (L.MoveRec * n)()
    for i in range(n):
        moves[i].key[0], moves[i].key[1], moves[i].reward = keys[i][0], keys[i][1], rewards[i]
    z, t = np.zeros(n), np.zeros(n)
    L.check(L.lib().az_push_trace(moves, n, 1.0, _vp(z), _vp(t)))
    mem, _ = new_pair(TTT, 16)
    P = A.astype(np.float64) / A.sum(axis=1, keepdims=True)
    mem.push_trace(X, A, P, rewards, wp, 1.0)
    _, _, _, gz, gt, _ = mem.samples()
    assert np.array_equal(_bits(gz[::-1].copy()), _bits(z)) and np.array_equal(gt[::-1], t) and np.abs(z).max() == abs(rewards[-1])
    mem.close()


# ---------------------------------------------------------------------------------------------------- 4. the keyed path
def _ttt_positions(ngames):
    keys = []
    for g in range(ngames):
        keys += _ttt_game(100 + g)[0]
    return np.array(keys, dtype=np.uint64)


@pytest.mark.parametrize("key_order", [False, True], ids=["random-order", "key-order"])
def test_against_the_keyed_memory(key_order):
    """the same Tic-tac-toe samples by key into az_memory and by the planes of az_game_encode into the plane memory, merged under
    LOG_WEIGHT with n up to 300: the same rows bit for bit.  key_order: the samples arrive sorted by key, so first occurrence IS the
    keyed path's key order and everything -- row order, sums, learning status -- is equal exactly; otherwise the rows are compared as
    multisets and the sums within 1e-6 relative (their summation order differs).  The random order evaluates the loss in ONE batch:
    `losses` scales a batch's loss by mean(W of the batch) / Wmean (learning.jl:86), so with several batches L depends on which rows
    share a batch -- on the row order -- by far more than rounding (6e-4 here with batches of 64), in the reference too."""
    import azhip
    from azhip import _lib as L
    keys = _ttt_positions(40)
    rng = np.random.default_rng(12)
    keys = keys[rng.permutation(len(keys))]
    if key_order:
        keys = keys[np.lexsort((keys[:, 1], keys[:, 0]))]
    n = len(keys)
    assert n > 200 and len({tuple(k) for k in keys.tolist()}) < 0.8 * n            # plenty of repeated positions
    gspec = azhip.TicTacToeSpec()
    with azhip.Engine(game=TTT, oracle=azhip.ORACLE_HASH, num_workers=8, batch_size=8, num_iters_per_turn=2) as e:
        X, A = e.encode(keys)
    P = rng.random((n, 9)) * A
    P /= P.sum(axis=1, keepdims=True)
    z, t, nv = rng.uniform(-1, 1, n), rng.integers(1, 10, n).astype(np.float64), rng.integers(1, 301, n).astype(np.int64)
    raw = (L.Sample * n)()
    for i in range(n):
        raw[i].key[0], raw[i].key[1] = int(keys[i, 0]), int(keys[i, 1])
        for a in range(9):
            raw[i].pi[a] = P[i, a]
        raw[i].z, raw[i].t, raw[i].n = z[i], t[i], int(nv[i])
    kmem = azhip.MemoryBuffer(gspec, n)
    L.check(L.lib().az_memory_push_samples(kmem._h, raw, n))
    pmem = azhip.PlaneMemoryBuffer(gspec, n)
    pmem.push_samples(X, A, P, z, t, nv)
    hp = azhip.ResNetHP(num_blocks=1, num_filters=64, num_policy_head_filters=32, num_value_head_filters=32)
    nn = azhip.ResNet(gspec, hp, seed=5)
    batch = 64 if key_order else 1 << 20
    lp = azhip.LearningParams(samples_weighing_policy=LOG, l2_regularization=1e-4, loss_computation_batch_size=batch, use_position_averaging=True)
    lpt = azhip.LearningParams(samples_weighing_policy=LOG, l2_regularization=1e-4, loss_computation_batch_size=batch, use_position_averaging=False)
    with azhip.Trainer(gspec, nn, kmem, lp) as trk, pmem.dataset(use_position_averaging=True, weighing_policy=LOG) as pd:
        kd = trk.data
        kt, pt = kd.tensors(), pd.tensors()
        assert len(kd) == len(pd) and kd.sum_n == pd.sum_n == int(nv.sum()) and kt[0].max() > 8.0     # log2(n) + 1 of a merged n > 128
        rows = lambda ts: np.concatenate([_bits(np.ascontiguousarray(x.reshape(len(x), -1))) for x in ts], axis=1)
        rk, rp = rows(kt), rows(pt)
        if key_order:
            assert np.array_equal(rk, rp)
        assert sorted(map(bytes, rk)) == sorted(map(bytes, rp))
        with azhip.Trainer(gspec, nn, pd, lpt) as trp:
            sk, sp = trk.learning_status(), trp.learning_status()
        a = np.array([kd.Wtot, kd.Wmean, kd.Hp, sk.loss.L, sk.loss.Lp, sk.loss.Lv, sk.loss.Lreg, sk.loss.Linv, sk.Hp, sk.Hpnet], dtype=np.float64)
        b = np.array([pd.Wtot, pd.Wmean, pd.Hp, sp.loss.L, sp.loss.Lp, sp.loss.Lv, sp.loss.Lreg, sp.loss.Linv, sp.Hp, sp.Hpnet], dtype=np.float64)
        print("keyed ", a, "\nplanes", b)
        assert np.allclose(a, b, rtol=1e-6, atol=0), (a, b)
        if key_order:                                                # the same rows in the same order: the same sums
            assert np.array_equal(a, b), (a, b)
    kmem.close()
    pmem.close()


# ---------------------------------------------------------------------------------------------------- 5. training
def test_training_on_a_plane_memory_data_set_is_training_on_its_tensors():
    import azhip
    X, A = make_rows(GO9, 96, seed=13)
    s = make_samples(GO9, np.arange(96), X, A, seed=14)
    mem, ref = new_pair(GO9, 128)
    push_both(mem, ref, s)
    gspec = mem.gspec
    hp = azhip.ResNetHP(num_blocks=2, num_filters=64, num_policy_head_filters=32, num_value_head_filters=32)
    nn = azhip.ResNet(gspec, hp, seed=6)
    lp = azhip.LearningParams(samples_weighing_policy=LINEAR, l2_regularization=1e-4, loss_computation_batch_size=32, batch_size=32,
                              use_position_averaging=False)
    out = []
    with mem.dataset(weighing_policy=LINEAR) as pd, azhip.TensorDataset(gspec, *ref_convert(ref.get_experience(), LINEAR)) as td:
        for d in (pd, td):
            with azhip.Trainer(gspec, nn, d, lp) as tr:
                out.append((tr.batch_updates(3), tr.trained_params()))
    (l0, p0), (l1, p1) = out
    assert np.all(np.isfinite(l0)) and np.array_equal(_bits(l0), _bits(l1)) and np.array_equal(_bits(p0), _bits(p1))
    assert not np.array_equal(p0, nn.params())
    mem.close()


# ---------------------------------------------------------------------------------------------------- 6. collisions
def test_a_hash_collision_is_an_error_never_a_merged_row():
    from azhip import _lib as L
    f = L.lib().az_debug_plane_memory_hash_bits
    f.argtypes, f.restype = [C.c_void_p, C.c_int32], C.c_int
    X, A = make_rows(GO9, 200, seed=15)
    s = make_samples(GO9, np.arange(200), X, A, seed=16)
    mem, ref = new_pair(GO9, 256)
    push_both(mem, ref, s)
    L.check(f(mem._h, 4))                                            # 200 distinct rows on 16 keys
    with pytest.raises(L.AzError, match="plane hash collision") as ei:
        mem.dataset(use_position_averaging=True)
    assert ei.value.status == L.AZ_ERR_STATE
    check_dataset(mem, ref, False, False, CONSTANT)                  # no hashing without merging
    assert f(mem._h, 0) == L.AZ_ERR_BAD_ARG and f(mem._h, 129) == L.AZ_ERR_BAD_ARG and f(None, 4) == L.AZ_ERR_BAD_ARG
    L.check(f(mem._h, 128))
    assert len(check_dataset(mem, ref, False, True, CONSTANT)[0]) == 200
    # equal rows are still found through a truncated key when no two DIFFERENT rows share one
    mem2, ref2 = new_pair(GO9, 16)
    push_both(mem2, ref2, make_samples(GO9, np.zeros(9, dtype=int), X, A, seed=17))
    L.check(f(mem2._h, 1))
    assert len(check_dataset(mem2, ref2, False, True, LINEAR)[0]) == 1
    mem.close()
    mem2.close()


# ---------------------------------------------------------------------------------------------------- 7. errors
def _spoil(which, index, value):
    def f(s):
        s[which][index] = value
    return f


def _no_legal(s):
    s[1][3, :] = 0.0
    s[2][3, :] = 0.0


REFUSALS = [
    ("nan in X", _spoil(0, (4, 3, 8, 8), np.nan), "sample 4: a non-finite value"),
    ("inf in A", _spoil(1, (5, 81), np.inf), "sample 5: a non-finite value"),
    ("nan in pi", _spoil(2, (6, 80), np.nan), "sample 6: a non-finite value"),
    ("inf in z", _spoil(3, 2, np.inf), "sample 2: a non-finite value"),
    ("nan in t", _spoil(4, 7, np.nan), "sample 7: a non-finite value"),
    ("n zero", _spoil(5, 1, 0), "sample 1: n < 1"),
    ("A half", _spoil(1, (1, 81), 0.5), "sample 1: an entry of A outside {0, 1}"),
    ("no legal action", _no_legal, "sample 3: no legal action"),
    ("pi negative", _spoil(2, (2, 81), -0.25), "sample 2: P < 0"),
    ("pi on an illegal action", _spoil(1, (5, 81), 0.0), "sample 5: P > 0 where A == 0"),
]


@pytest.mark.parametrize("name,spoil,message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_push_refuses_and_leaves_the_buffer_unchanged(name, spoil, message):
    from azhip import _lib as L
    X, A = make_rows(GO9, 8, seed=18)
    A[:, 81] = 1.0
    good = make_samples(GO9, np.arange(8), X, A, seed=19)
    mem, ref = new_pair(GO9, 12)
    push_both(mem, ref, good)
    bad = [a.copy() for a in good]
    spoil(bad)
    with pytest.raises(L.AzError, match=message.replace("{", r"\{").replace("}", r"\}")) as ei:
        mem.push_samples(*bad)
    assert ei.value.status == L.AZ_ERR_BAD_ARG
    if name != "n zero":                                             # a trace has no n
        with pytest.raises(L.AzError, match=message.replace("{", r"\{").replace("}", r"\}") if name not in ("inf in z", "nan in t") else "non-finite") as ei:
            mem.push_trace(bad[0], bad[1], bad[2], bad[3] if name == "inf in z" else np.where(np.isfinite(bad[4]), 0.0, np.nan), np.ones(8, dtype=np.uint8), 1.0)
        assert ei.value.status == L.AZ_ERR_BAD_ARG
    assert (len(mem), mem.cur_batch_size()) == (8, 0)
    for a, b in zip(mem.samples(), good):
        assert np.array_equal(a, b)
    check_dataset(mem, ref, False, True, LINEAR)
    mem.close()


def test_bad_calls():
    import azhip
    from azhip import _lib as L
    lib = L.lib()
    h = C.c_void_p()
    assert lib.az_plane_memory_create(GO9, 0, 16, None) == L.AZ_ERR_BAD_ARG
    for game, device, cap, what in ((9, 0, 16, "unknown game"), (GO9, 0, 0, "capacity"), (GO9, 0, -5, "capacity"), (GO9, 99, 16, "device 99 not available")):
        assert lib.az_plane_memory_create(game, device, cap, C.byref(h)) == L.AZ_ERR_BAD_ARG and what in lib.az_last_error().decode() and not h.value
    X, A = make_rows(GO9, 4, seed=20)
    s = list(make_samples(GO9, np.arange(4), X, A, seed=21))
    for f, args in ((lib.az_plane_memory_destroy, ()), ):
        assert f(None, *args) == L.AZ_OK
    assert lib.az_plane_memory_length(None, None, None) == L.AZ_ERR_BAD_ARG and lib.az_plane_memory_new_batch(None) == L.AZ_ERR_BAD_ARG
    assert lib.az_plane_memory_empty(None) == L.AZ_ERR_BAD_ARG
    assert lib.az_plane_memory_push_samples(None, 4, *[_vp(a) for a in s]) == L.AZ_ERR_BAD_ARG
    assert lib.az_dataset_create_from_plane_memory(None, 0, 0, 0, C.byref(h)) == L.AZ_ERR_BAD_ARG
    mem = azhip.PlaneMemoryBuffer(azhip.Go9PlanesSpec(), 8)
    for k in range(5):                                               # nvis alone may be NULL
        assert lib.az_plane_memory_push_samples(mem._h, 4, *[None if i == k else _vp(a) for i, a in enumerate(s)]) == L.AZ_ERR_BAD_ARG
        assert "NULL" in lib.az_last_error().decode()
    r, wp = np.zeros(4), np.ones(4, dtype=np.uint8)
    tr = [s[0], s[1], s[2], r, wp]
    for k in range(5):
        assert lib.az_plane_memory_push_trace(mem._h, 4, *[None if i == k else _vp(a) for i, a in enumerate(tr)], 1.0) == L.AZ_ERR_BAD_ARG
    assert lib.az_plane_memory_push_samples(mem._h, -1, *[_vp(a) for a in s]) == L.AZ_ERR_BAD_ARG
    assert lib.az_plane_memory_push_trace(mem._h, -1, *[_vp(a) for a in tr], 1.0) == L.AZ_ERR_BAD_ARG
    assert lib.az_plane_memory_push_trace(mem._h, 4, *[_vp(a) for a in tr], float("nan")) == L.AZ_ERR_BAD_ARG
    assert lib.az_plane_memory_push_samples(mem._h, 0, None, None, None, None, None, None) == L.AZ_OK
    assert lib.az_plane_memory_push_trace(mem._h, 0, None, None, None, None, None, 1.0) == L.AZ_OK
    assert len(mem) == 0
    # nothing to build from: an empty memory, then which = 1 with an empty batch
    for fill in (False, True):
        if fill:
            mem.push_samples(*s)
        assert lib.az_dataset_create_from_plane_memory(mem._h, 1, 0, 0, C.byref(h)) == L.AZ_ERR_STATE and not h.value
        assert ("batch is empty" if fill else "empty") in lib.az_last_error().decode()
    assert lib.az_dataset_create_from_plane_memory(mem._h, 0, 0, 0, None) == L.AZ_ERR_BAD_ARG
    assert lib.az_dataset_create_from_plane_memory(mem._h, 2, 0, 0, C.byref(h)) == L.AZ_ERR_BAD_ARG
    assert lib.az_dataset_create_from_plane_memory(mem._h, 0, 0, 3, C.byref(h)) == L.AZ_ERR_BAD_ARG
    assert lib.az_plane_memory_read(mem._h, 2, 3, None, None, None, None, None, None) == L.AZ_ERR_BAD_ARG
    with pytest.raises(ValueError, match="use_symmetries"):
        mem.dataset(use_symmetries=True)
    with pytest.raises(ValueError, match="shape"):
        mem.push_samples(s[0][:, :3], *s[1:])
    # a data set of one geometry is refused by an engine of another (the device / game check of az_learning_status)
    with mem.dataset() as d, azhip.Engine(game=TTT, oracle=azhip.ORACLE_RESNET, num_workers=8, batch_size=8, num_iters_per_turn=2,
                                          num_blocks=1, num_filters=64, num_policy_head_filters=32, num_value_head_filters=32) as e:
        hp = azhip.ResNetHP(num_blocks=1, num_filters=64, num_policy_head_filters=32, num_value_head_filters=32)
        e.net_set_params(azhip.ResNet(azhip.TicTacToeSpec(), hp, seed=1).params())
        out = L.LearningStatusRec()
        assert lib.az_learning_status(e._h, d._h, 0.0, 1.0, 1.0, 32, C.byref(out)) == L.AZ_ERR_BAD_ARG
        assert "differ in game or device" in lib.az_last_error().decode()
        raw = (L.Sample * 4)()
        assert lib.az_dataset_read(d._h, 0, 4, raw, None, None, None, None, None) == L.AZ_ERR_BAD_ARG       # no az_sample records behind it
    mem.close()
