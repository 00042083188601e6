"""azhip.TensorDataset / Go9PlanesSpec without a GPU: what Python checks before the library is loaded.

A TensorDataset takes the (W, X, A, P, V) arrays of convert_samples (src/learning.jl:17-51) from the caller.  Ranks, shapes against
the game's geometry, one sample count and a float32-convertible dtype are checked in Python (ValueError); the values are checked
on the device (tests/test_tensor_dataset_gpu.py)."""
import numpy as np
import pytest


def _arrays(n=3, nA=82, dims=(4, 9, 9)):
    return dict(W=np.ones(n), X=np.zeros((n,) + dims), A=np.ones((n, nA)), P=np.full((n, nA), 1.0 / nA), V=np.zeros(n))


def test_go9_planes_spec_is_geometry_only():
    import azhip
    g = azhip.Go9PlanesSpec()
    assert g.game_id == azhip.GAME_GO9_PLANES == 3 and g.num_actions() == 82 and g.state_dim() == (9, 9, 4)
    assert len(g.actions()) == 82 and g == azhip.Go9PlanesSpec() and g != azhip.TicTacToeSpec()
    with pytest.raises(NotImplementedError):
        g.init()
    hp = azhip.ResNetHP(num_blocks=1, num_filters=64, num_policy_head_filters=32, num_value_head_filters=32)
    nn = azhip.ResNet(g, hp, seed=1)                                # the parameter blob only: no engine until it evaluates
    from azhip.network import num_parameters
    assert nn.params().size == num_parameters(3, hp)


def test_validate_accepts_the_geometry_and_converts_to_float32():
    import azhip
    for spec, dims, nA in ((azhip.Go9PlanesSpec(), (4, 9, 9), 82), (azhip.ConnectFourSpec(), (3, 6, 7), 7), (2, (5, 1, 14), 6)):
        a = _arrays(5, nA, dims)
        a["X"] = a["X"].astype(np.int8)                             # integers and float64 convert
        gspec, out = azhip.TensorDataset.validate(spec, **a)
        assert gspec.num_actions() == nA and [x.dtype for x in out] == [np.float32] * 5 and all(x.flags.c_contiguous for x in out)
        assert [x.shape for x in out] == [(5,), (5,) + dims, (5, nA), (5, nA), (5,)]


@pytest.mark.parametrize("change,match", [
    (dict(X=np.zeros((3, 4, 81))), "X must have 4 dimensions"),              # wrong rank
    (dict(W=np.ones((3, 1))), "W must have 1 dimensions"),
    (dict(A=np.ones(3 * 82)), "A must have 2 dimensions"),
    (dict(X=np.zeros((3, 9, 9, 4))), "X must have shape"),                   # right rank, not (C, H, W)
    (dict(P=np.ones((3, 81))), "P must have shape"),
    (dict(V=np.zeros(4)), "V holds 4 samples, W holds 3"),                  # sample counts differ
    (dict(A=np.ones((2, 82))), "A holds 2 samples, W holds 3"),
    (dict(W=np.array(["1", "1", "1"])), "W cannot be converted to float32"),
    (dict(V=np.array([None, 1.0, 2.0], dtype=object)), "V cannot be converted to float32"),
    (dict(P=np.ones((3, 82), dtype=np.complex64)), "P cannot be converted to float32"),
    (dict(W=np.ones(0), X=np.zeros((0, 4, 9, 9)), A=np.ones((0, 82)), P=np.ones((0, 82)), V=np.zeros(0)), "at least one sample"),
])
def test_tensor_dataset_rejects_bad_arrays_before_the_library_is_loaded(change, match, monkeypatch):
    import azhip
    from azhip import _lib

    def no_library():
        raise AssertionError("the library was loaded before the arrays were checked")
    monkeypatch.setattr(_lib, "lib", no_library)
    a = dict(_arrays(), **change)
    with pytest.raises(ValueError, match=match):
        azhip.TensorDataset(azhip.Go9PlanesSpec(), a["W"], a["X"], a["A"], a["P"], a["V"])
    with pytest.raises(ValueError, match="unknown game id"):
        azhip.TensorDataset(17, **_arrays())


@pytest.mark.parametrize("kw,params_kw,match", [(dict(use_symmetries=True), {}, "use_symmetries"), (dict(last_batch=True), {}, "last_batch"),
                                                ({}, dict(use_position_averaging=True), "use_position_averaging")])
def test_trainer_refuses_memory_options_with_tensors(kw, params_kw, match):
    """augment_with_symmetries, last_batch and merge_by_state act on a MemoryBuffer's samples; with tensors they are an error,
    raised before anything touches the device"""
    import azhip
    g = azhip.Go9PlanesSpec()
    data = azhip.TensorDataset.__new__(azhip.TensorDataset)         # no device here: the check looks at the type only
    data.gspec, data._h = g, None
    hp = azhip.ResNetHP(num_blocks=1, num_filters=64, num_policy_head_filters=32, num_value_head_filters=32)
    lp = azhip.LearningParams(samples_weighing_policy=0, l2_regularization=1e-4, loss_computation_batch_size=64,
                              **dict(dict(use_position_averaging=False), **params_kw))
    with pytest.raises(ValueError, match=match):
        azhip.Trainer(g, azhip.ResNet(g, hp, seed=1), data, lp, **kw)


def test_the_new_entry_point_is_declared_everywhere():
    """include/azhip.h, the ctypes table and the Julia glue name az_dataset_create_from_tensors; the ABI version is unchanged"""
    import os
    import re
    from azhip import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "azhip.h")).read()
    assert re.search(r"int az_dataset_create_from_tensors\(int32_t game, int32_t device, int64_t n,", hdr)
    assert len(_lib.SYMBOLS["az_dataset_create_from_tensors"]) == 9 and _lib.ABI_VERSION == 4 and "#define AZ_ABI_VERSION 4" in hdr
    assert "az_dataset_create_from_tensors" in open(os.path.join(root, "julia", "AlphaZeroHIPExtras.jl")).read()
