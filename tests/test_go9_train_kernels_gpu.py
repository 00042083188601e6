"""The optimiser step's MFMA kernels on the 9x9 geometry (AZ_GAME_GO9_PLANES: 81 positions), BIT FOR BIT -- the method and the helpers
of tests/test_train_kernels_gpu.py (small-integer inputs, float64 references, the az_debug_trainer_* seams), on a trainer whose data
set was made from tensors.

What is new for an 81-cell board, and the smallest batches that reach it (CUs = the device's count, 256 on an MI355X):
  k_conv16_layer   T16<Go9Planes, F, 11> = 176 rows = 2 boards per workgroup, T16<.., 6> = 96 rows = 1 board.
      128 filters, 11 tiles: B = 1 is not a trainer (batch statistics need two samples), so the half-empty workgroup is the LAST one
      of B = 3 and 5; B = 2 one full workgroup; B = 2 CUs + 1 more workgroups than CUs with a half-empty last one.
      64 filters: the 6-tile form while ceil(B / 2) <= CUs (B = 3), the 11-tile form above (B = 2 CUs + 1).
  k_wgrad16        one board per LDS chunk of 96 rows (NBC = 1); 128 filters: input channels split in two, CUs / 3 workgroups per tap
      group: B = 2 (one board per workgroup, most workgroups idle), CUs / 3 (every workgroup one board), CUs / 3 + 1 (the first
      workgroup loops: two chunks), 2 (CUs / 3) + 1 (two full rounds and a third chunk for the first).  64 filters: CUs workgroups,
      B = CUs + 1.
Every case asserts the plan it reached, so on another chip it fails instead of quietly testing something else."""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from azhip.network import param_layout, random_params
from test_train_kernels_gpu import (_bn_consts, _check_exact, _chunks, _conv, _int_weights, _ints, _nchw, _rows, _torch_w, _wgrad, _wgrad_ref,
                                    conv_plan)

pytestmark = pytest.mark.gpu
GO, P = 3, 81
NSAMPLES = 600                                                      # >= the largest batch here (2 x 256 + 1)


@functools.lru_cache(maxsize=None)
def _cus():
    import azhip
    with azhip.Engine(game=0, oracle=azhip.ORACLE_UNIFORM, num_workers=1, batch_size=1, num_iters_per_turn=2) as e:
        return e.device_info()[1]


@functools.lru_cache(maxsize=None)
def _data():
    """one tensor data set for every trainer here: the seams never read the samples, the trainer takes min(batch_size, #samples) from it"""
    import atexit
    import azhip
    rng = np.random.default_rng(0)
    n = NSAMPLES
    A = np.ones((n, 82), dtype=np.float32)
    td = azhip.TensorDataset(azhip.Go9PlanesSpec(), np.ones(n), rng.integers(0, 2, size=(n, 4, 9, 9)), A, A / 82.0, np.zeros(n))
    atexit.register(td.close)
    return td


@contextlib.contextmanager
def _trainer(F, B):
    """a 1-block Go trainer of batch B whose two F -> F convolutions carry integer weights: (handle, {layer: Flux W}, CU count)"""
    import azhip
    gspec = azhip.Go9PlanesSpec()
    hp = azhip.ResNetHP(num_blocks=1, num_filters=F, num_policy_head_filters=32, num_value_head_filters=32)
    blob = random_params(GO, hp, seed=1)
    Wl, off = {}, 0
    for name, shape in param_layout(GO, hp):
        n = int(np.prod(shape))
        for layer, nm in ((1, "block0.conv1.W"), (2, "block0.conv2.W")):
            if name == nm:
                Wl[layer] = _int_weights(F, 300 + layer)
                blob[off:off + n] = Wl[layer].reshape(-1, order="F")
        off += n
    lp = azhip.LearningParams(samples_weighing_policy=0, l2_regularization=0.0, loss_computation_batch_size=64, batch_size=B,
                              use_position_averaging=False)
    assert 2 <= B <= NSAMPLES
    with azhip.Trainer(gspec, azhip.ResNet(gspec, hp, params=blob), _data(), lp) as tr:
        h = tr._trainer()
        assert tr.batch_size() == B
        yield h, Wl, tr._eng.device_info()[1]


def go_wgrad_plan(F, B, ncu):
    """trainer_build's wg_splits and the kernel's even spread of the boards; a chunk is one board (96 rows) at either filter count"""
    splits = max(1, min(B, ncu // (3 if F == 128 else 1)))
    bq, br = divmod(B, splits)
    return splits, sorted(({bq + 1} if br else set()) | ({bq} if br < splits else set()))


# (filters, batch as a function of the CU count, boards per workgroup the case is named for)
WGRAD_CASES = [
    (128, "2", lambda cu: 2, [1]),                          # one board per workgroup, most workgroups without a board
    (128, "cu/3", lambda cu: cu // 3, [1]),                 # 85 on 256 CUs: every workgroup one board
    (128, "cu/3+1", lambda cu: cu // 3 + 1, [1, 2]),        # 86: the first workgroup holds two = the chunk loop iterates
    (128, "2cu/3+1", lambda cu: 2 * (cu // 3) + 1, [2, 3]),  # 171: two full rounds, a third chunk for the first workgroup
    (64, "cu+1", lambda cu: cu + 1, [1, 2]),                # 257: 64 filters, all nine taps per workgroup
]


@pytest.mark.parametrize("F,name,batch,boards", WGRAD_CASES, ids=["%d-%s" % c[:2] for c in WGRAD_CASES])
def test_go9_wgrad16_is_exact(F, name, batch, boards):
    """B = 2, 85, 86, 171 at 128 filters and 257 at 64 on 256 CUs.  The fp32 sums run over rows in board order, boards in batch order
    inside a workgroup, workgroup partials in index order -- with integer inputs below 2^24 any order gives the same bits, so the
    reference does not depend on the chunk form"""
    B = batch(_cus())
    assert 9 * B * P < 2 ** 24                                      # hard bound of any partial sum: |a| |dg| <= 9 per row
    with _trainer(F, B) as (h, _, ncu):
        splits, got_boards = go_wgrad_plan(F, B, ncu)
        assert got_boards == boards, "on %d CUs B = %d gives %d workgroups per tap group with %s boards: not what the case is named for" % (ncu, B, splits, got_boards)
        print("go9 wgrad F=%d B=%d: %d workgroups per tap group, chunks %s" % (F, B, splits, [_chunks(1, n) for n in boards]))
        rng = np.random.default_rng(1000 * B + F)
        for rep in range(2):                                        # twice: a stale LDS chunk or partial buffer is a bit difference
            a, dg = _ints(rng, (B * P, F)), _ints(rng, (B * P, F))
            want = _wgrad_ref(GO, a, dg, B, F)
            assert 0 < np.abs(want).max() < 2 ** 24
            _check_exact("weight gradient, pass %d" % rep, _wgrad(h, a, dg, F), want)


def _conv_case(F, B, layer, tiles, reps):
    """forward (BnIn, column sums; layer 2 with the skip input) and data gradient (without and with addend) against fp64 conv2d / autograd"""
    with _trainer(F, B) as (h, Wl, ncu):
        nt, nparts = conv_plan(GO, F, B, ncu)
        assert nt == tiles, "on %d CUs this batch runs the %d-tile form, the case is named for the %d-tile form" % (ncu, nt, tiles)
        assert nparts == -(-B // (2 if tiles == 11 else 1))
        w = _torch_w(Wl[layer])
        rng = np.random.default_rng(7 * B + F + layer)
        assert 2 * 12 * 2 * 9 * F < 2 ** 24 and 3 * 2 * 9 * F + 3 < 2 ** 24      # hard bounds of any partial sum (test_train_kernels_gpu.py)
        for rep in range(reps):
            g, bn = _ints(rng, (B * P, F)), _bn_consts(rng, F)
            res = _ints(rng, (B * P, F)) if layer == 2 else None
            b64 = bn.astype(np.float64)
            a_want = b64[2] * ((g.astype(np.float64) - b64[0]) * b64[1]) + b64[3]
            if res is not None:
                a_want = a_want + res
            a_want = np.maximum(a_want, 0.0)
            out_want = _rows(torch.nn.functional.conv2d(_nchw(GO, a_want, B), w, None, padding=1))
            sums_want = np.stack([out_want.sum(axis=0), (out_want ** 2).sum(axis=0)])
            assert 0 < np.abs(out_want).max() < 2 ** 24 and 4 * np.abs(sums_want).max() < 2 ** 53
            out, a_out, sums, np_got = _conv(h, layer, 0, g, res, bn, F)
            assert np_got == nparts, (np_got, nparts)
            _check_exact("a_out", a_out, a_want)
            _check_exact("forward", out, out_want)
            _check_exact("column sums", sums, sums_want)
            dg, addend = _ints(rng, (B * P, F)), _ints(rng, (B * P, F))
            x = torch.zeros(B, F, 9, 9, dtype=torch.float64, requires_grad=True)
            (da,) = torch.autograd.grad(torch.nn.functional.conv2d(x, w, None, padding=1), x, grad_outputs=_nchw(GO, dg, B))
            da_want = _rows(da)
            assert 0 < np.abs(da_want).max() and np.abs(da_want).max() + 3 < 2 ** 24
            out, np_got = _conv(h, layer, 1, dg, None, None, F)
            assert np_got == nparts
            _check_exact("data gradient", out, da_want)
            out, np_got = _conv(h, layer, 1, dg, addend, None, F)
            _check_exact("data gradient + addend", out, da_want + addend)


@pytest.mark.parametrize("B", [2, 3, 5, 513])
def test_go9_conv16_layer_128_filters_is_exact(B):
    """11 tiles, 2 boards per workgroup: one full workgroup (2), a half-empty last one (3, 5; a trainer of ONE board does not exist),
    2 CUs + 1 boards = more workgroups than CUs (513 on 256 CUs; one pass, the small cases two)"""
    big = B == 513
    _conv_case(128, 2 * _cus() + 1 if big else B, layer=1 + B % 2, tiles=11, reps=1 if big else 2)


def test_go9_conv16_layer_64_filters_6_tiles_is_exact():
    _conv_case(64, 3, layer=2, tiles=6, reps=2)


def test_go9_conv16_layer_64_filters_11_tiles_by_batch_is_exact():
    """ceil(B / 2) > CUs: tr_conv16 leaves the 6-tile form by itself"""
    _conv_case(64, 2 * _cus() + 1, layer=1, tiles=11, reps=1)
