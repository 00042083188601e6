"""az_dataset_create_from_tensors: a Trainer's data from (W, X, A, P, V) tensors the caller converted itself.

(a) For the three games with a device twin a data set made from the tensors of a memory-made data set IS that data set: the
    tensors come back bit for bit, Wtot / Wmean are bit-equal (the same reducer over the same doubles), Hp and the learning status
    agree within the bounds tests/test_memory_gpu.py::test_learning_status_matches_oracle holds the memory path to, and the
    gradient of a batch -- which does not depend on Hp -- is bit-identical.
(b) Every clause of the entry point's validation refuses with AZ_ERR_BAD_ARG and says which sample and why; az_dataset_read
    refuses `samples` on such a data set; the replay memory still refuses the 9x9x4 geometry."""
import ctypes as C

import numpy as np
import pytest

from test_train_gpu import _memory

pytestmark = pytest.mark.gpu


def _vp(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


@pytest.mark.parametrize("game,policy", [(0, 1), (1, 2), (2, 0)], ids=["c4", "ttt", "mancala"])
def test_tensor_dataset_equals_memory_dataset(game, policy):
    """Gradient equality: two trainers over ONE memory-made data set were run on the parent commit first (Connect-Four, Tic-tac-toe
    and Mancala, this network, these indices, each trainer three times): every pair of gradient arrays was bit-identical (largest
    difference 0.0), so equality is what is asserted here."""
    import azhip
    gspec, mem = _memory(game, 12, 7)
    hp = azhip.ResNetHP(num_blocks=1, num_filters=64, num_policy_head_filters=32, num_value_head_filters=32)
    nn = azhip.ResNet(gspec, hp, seed=4)
    lp = azhip.LearningParams(samples_weighing_policy=policy, l2_regularization=1e-4, loss_computation_batch_size=32, batch_size=24)
    with azhip.Trainer(gspec, nn, mem, lp, use_symmetries=game != 2) as trm:
        md = trm.data
        tensors = md.tensors()
        n = len(md)
        assert n >= 24
        idx = (np.arange(24) * 5) % n
        stm = trm.learning_status()
        repm = trm.samples_report()
        lossm, partsm, gradm = trm.gradients(idx)
        lpt = azhip.LearningParams(samples_weighing_policy=policy, l2_regularization=1e-4, loss_computation_batch_size=32, batch_size=24,
                                   use_position_averaging=False)
        with azhip.TensorDataset(gspec, *tensors) as td:
            assert len(td) == n == td.num_samples == td.sum_n
            for a, b in zip(td.tensors(), tensors):
                assert a.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
            assert td.Wtot == md.Wtot and np.float32(td.Wmean) == np.float32(md.Wmean)
            assert np.isclose(td.Hp, md.Hp, rtol=2e-6, atol=0), (td.Hp, md.Hp)
            with pytest.raises(TypeError):
                td.samples()
            with pytest.raises(TypeError):
                td.raw_samples()
            with azhip.Trainer(gspec, nn, td, lpt) as trt:
                assert trt.data is td and trt.num_samples() == n and trt.batch_size() == 24
                stt = trt.learning_status()
                rept = trt.samples_report()
                losst, partst, gradt = trt.gradients(idx)
            assert td._h is not None                                # the trainer does not own the caller's data set
            td.tensors()
    got = np.array([stt.loss.L, stt.loss.Lp, stt.loss.Lv, stt.loss.Lreg, stt.loss.Linv, stt.Hp, stt.Hpnet])
    want = np.array([stm.loss.L, stm.loss.Lp, stm.loss.Lv, stm.loss.Lreg, stm.loss.Linv, stm.Hp, stm.Hpnet])
    assert np.allclose(got, want, rtol=2e-6, atol=1e-7), (got, want)
    assert rept.num_boards == rept.num_samples == n and rept.Wtot == repm.Wtot
    assert np.abs(gradm).max() > 0
    assert np.array_equal(gradt.view(np.uint32), gradm.view(np.uint32)), np.abs(gradt - gradm).max()
    assert np.allclose(partst[[1, 3, 4]], partsm[[1, 3, 4]], rtol=0, atol=0) and np.isclose(partst[0], partsm[0], rtol=2e-6, atol=1e-7)
    mem.close()


def _go_arrays(n, seed=1):
    rng = np.random.default_rng(seed)
    W = rng.uniform(0.5, 2.0, n).astype(np.float32)
    X = rng.integers(0, 2, size=(n, 4, 9, 9)).astype(np.float32)
    A = (rng.random((n, 82)) < 0.6).astype(np.float32)
    A[:, 81] = 1.0
    P = (rng.random((n, 82)) * A).astype(np.float32)
    P /= P.sum(axis=1, keepdims=True)
    V = rng.uniform(-1, 1, n).astype(np.float32)
    return [W, X, A, P, V]


def _create(game, n, arrays):
    from azhip import _lib as L
    h = C.c_void_p()
    st = L.lib().az_dataset_create_from_tensors(game, 0, n, *[_vp(a) for a in arrays], C.byref(h))
    msg = L.lib().az_last_error().decode()
    if st == 0:
        L.lib().az_dataset_destroy(h)
    return st, msg, h


def _poke(which, index, value):
    def f(arrays):
        arrays["WXAPV".index(which)][index] = value
    return f


def _no_legal(arrays):
    arrays[2][3, :] = 0.0
    arrays[3][3, :] = 0.0


REFUSALS = [
    ("nan in X", _poke("X", (4, 2, 3, 3), np.nan), "sample 4: a non-finite value"),
    ("inf in V", _poke("V", 5, np.inf), "sample 5: a non-finite value"),
    ("inf in W", _poke("W", 0, np.inf), "sample 0: a non-finite value"),
    ("nan in P", _poke("P", (6, 81), np.nan), "sample 6: a non-finite value"),
    ("W zero", _poke("W", 2, 0.0), "sample 2: W <= 0"),
    ("W negative", _poke("W", 7, -1.0), "sample 7: W <= 0"),
    ("A half", _poke("A", (1, 81), 0.5), "sample 1: an entry of A outside {0, 1}"),
    ("A two", _poke("A", (1, 81), 2.0), "sample 1: an entry of A outside {0, 1}"),
    ("no legal action", _no_legal, "sample 3: no legal action"),
    ("P negative", _poke("P", (2, 81), -0.25), "sample 2: P < 0"),
    ("P on an illegal action", lambda a: (a[2].__setitem__((5, 81), 0.0)), "sample 5: P > 0 where A == 0"),
]


@pytest.mark.parametrize("name,spoil,message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_create_from_tensors_refuses(name, spoil, message):
    from azhip import _lib as L
    arrays = _go_arrays(8)
    st, msg, _ = _create(L.GAME_GO9_PLANES, 8, arrays)
    assert st == L.AZ_OK, msg                                        # the untouched arrays are fine
    spoil(arrays)
    st, msg, h = _create(L.GAME_GO9_PLANES, 8, arrays)
    assert st == L.AZ_ERR_BAD_ARG and message in msg and not h.value, (st, msg)


def test_create_from_tensors_refuses_bad_calls_and_read_refuses_samples():
    import azhip
    from azhip import _lib as L
    arrays = _go_arrays(8)
    for n in (0, -3):
        st, msg, _ = _create(L.GAME_GO9_PLANES, n, arrays)
        assert st == L.AZ_ERR_BAD_ARG and "n must be" in msg
    for k in range(5):
        st, msg, _ = _create(L.GAME_GO9_PLANES, 8, [None if i == k else a for i, a in enumerate(arrays)])
        assert st == L.AZ_ERR_BAD_ARG and "NULL" in msg
    assert L.lib().az_dataset_create_from_tensors(L.GAME_GO9_PLANES, 0, 8, *[_vp(a) for a in arrays], None) == L.AZ_ERR_BAD_ARG
    st, msg, _ = _create(9, 8, arrays)
    assert st == L.AZ_ERR_BAD_ARG and "unknown game" in msg
    h = C.c_void_p()
    assert L.lib().az_dataset_create_from_tensors(L.GAME_GO9_PLANES, 99, 8, *[_vp(a) for a in arrays], C.byref(h)) == L.AZ_ERR_BAD_ARG
    # a sample record has room for AZ_MAX_ACTIONS = 9 actions: none stand behind a tensor data set, for any game
    with azhip.TensorDataset(azhip.Go9PlanesSpec(), *arrays) as td:
        out = (L.Sample * 8)()
        assert L.lib().az_dataset_read(td._h, 0, 8, out, None, None, None, None, None) == L.AZ_ERR_BAD_ARG
        assert b"no az_sample records" in L.lib().az_last_error()
        assert len(td) == 8 and td.Wtot == pytest.approx(float(arrays[0].astype(np.float64).sum()), rel=1e-12)
        hp_want = -(arrays[3].astype(np.float64) * np.log(arrays[3].astype(np.float64) + float(np.finfo(np.float32).eps)) * arrays[0][:, None]).sum() / arrays[0].astype(np.float64).sum()
        assert td.Hp == pytest.approx(hp_want, rel=2e-6)             # entropy_wmean(P, W), learning.jl:63,111
        W2 = np.zeros(3, dtype=np.float32)
        L.check(L.lib().az_dataset_read(td._h, 2, 3, None, _vp(W2), None, None, None, None))
        assert np.array_equal(W2, arrays[0][2:5])
    # the replay memory keeps refusing the geometry: it stores state keys and re-encodes them with the game's device twin
    with pytest.raises(L.AzError, match="network-only tensor geometry"):
        azhip.MemoryBuffer(azhip.Go9PlanesSpec(), 16)
