"""The optimiser step's three MFMA kernels one at a time, BIT FOR BIT, at the batches where their inner loops iterate.

tests/test_train_gpu.py holds the step end to end to 1e-3 of each gradient array's largest entry.  One dropped or doubled board among
1024 moves an entry by a few percent of THAT entry and passes there by luck.  Here the arithmetic is exact instead (the method of
tests/exact_nets.py): inputs are integers in [-3, 3], weights integers in [-2, 2], the batch-norm constants powers of two and
integers, so every fp32 partial sum is a small integer (or a multiple of 1/2) far below 2^24 in ANY summation order, and a wrong row,
tap, channel, chunk or split is a bit difference against a float64 reference.  The kernels run through the debug seams of
csrc/train.hip (az_debug_trainer_wgrad / _conv / _gemm): the trainer's own launch helpers, geometry tables, partial buffers, fragment
maps, workspace and split rule.  The step's other kernels -- column sums and their second stages, batch-norm apply / backward, the dense
epilogues, the stem's im2col, the loss, the step sums -- are held the same way in tests/test_train_passes_gpu.py.

Shapes are DERIVED from the device's CU count with the launch arithmetic of trainer_build / tr_wgrad16_f / tr_conv16 / gemm_f32
(restated below), and every case asserts that it reaches what it is named for: on a chip with another CU count a case fails instead
of quietly testing something smaller.

Smallest batch that makes each loop iterate (256 CUs):
  k_wgrad16, chunk loop `for (b0 = b_begin; b0 < b_end; b0 += NBC)`; a tap group has min(B, CUs / tg) workgroups, tg = 3 at 128 filters, 1 at 64
    128 filters, 4-wavefront form (every game here: P <= 48; one 48-row chunk = NBC boards: Connect-Four 1, Mancala 3, Tic-tac-toe 5)
      Connect-Four   NBC 1   B = 86 gives the first workgroup 2 boards = 2 chunks.  (The chunk is ONE board, not three: the batches 203 of
                             test_train_gpu.py already ran this loop three times.  The cases 255 ... 1027 run it 3 ... 13 times.)
      Mancala        NBC 3   B = 256 (85 workgroups, the first holds 4 boards = 3 + 1); tested: 345 (3+1, 3+2), 1024 (3+3+3+3 (+1))
      Tic-tac-toe    NBC 5   B = 426 (6 boards = 5 + 1); tested: 600 (5+2, 5+3)
    64 filters, 8-wavefront form (128-row chunk: Connect-Four 3, Mancala 9, Tic-tac-toe 14), 256 workgroups
      Connect-Four   NBC 3   B = 769 (4 boards = 3 + 1); tested: 1024 (3+1), 1028 (3+1, 3+2)
      Mancala        NBC 9   B = 2305 (10 boards = 9 + 1); tested: 2400 (9, 9+1)
  k_conv16_layer: no loop over boards; its forms are chosen by the batch.  64 filters: the 6-tile form while ceil(B / TB11) <= CUs
      (Connect-Four B <= 1024), else the 11-tile form: first at Connect-Four B = 1025 (tested: 1028), or at any batch with AZHIP_TRAIN_NT6=0.
  k_gemm_f32, split reduction: K >= 1024 with fewer than 256 output tiles (the dense heads' weight gradients have K = B: first at B = 1024);
      recomputed split count != first estimate: needs ceil(512 / tiles) < ceil(K / 256), e.g. 25 tiles with K = 5400 (21 -> 19 splits).
  k_gemm_reduce: 16-stride loop from 13 splits on, 4-stride tail for the rest: splits 3 ... 21 are all tested (the rule cannot give 2).
"""
import atexit
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from azhip.network import _DIMS, param_layout, random_params

pytestmark = pytest.mark.gpu
SPECS = {0: "ConnectFourSpec", 1: "TicTacToeSpec", 2: "MancalaSpec"}
NAMES = {0: "c4", 1: "ttt", 2: "mancala"}
MEM_SAMPLES = 2500                                                   # every trainer here draws its batch size from one data set per game


def _vp(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


# ---------------------------------------------------------------------------------------------- the launch arithmetic, restated
def _tb(game, nt):
    """boards of an nt-tile workgroup of k_conv16_layer (T16::TB)"""
    W, H = _DIMS[game][:2]
    return 16 * nt // (W * H)


def wgrad_plan(game, F, B, ncu):
    """(workgroups per tap group, NBC, sorted boards-per-workgroup values) of k_wgrad16: trainer_build's wg_splits, tr_wgrad16_f's form
    (128 filters and at most 48 positions: 48-row chunks, else 128-row chunks) and the kernel's even spread of the boards"""
    W, H = _DIMS[game][:2]
    P = W * H
    tg = 3 if F == 128 else 1
    splits = max(1, min(B, ncu // tg))
    rpc = 48 if (F == 128 and P <= 48) else 128
    nbc = max(1, rpc // P)
    bq, br = divmod(B, splits)
    boards = sorted(({bq + 1} if br else set()) | ({bq} if br < splits else set()))
    return splits, nbc, boards


def _chunks(nbc, n):
    return tuple(min(nbc, n - i) for i in range(0, n, nbc))


def conv_plan(game, F, B, ncu, nt6_on=True):
    """(row tiles per workgroup, workgroups) of k_conv16_layer as tr_conv16 chooses them"""
    tb11, tb6 = _tb(game, 11), _tb(game, 6)
    small = F == 64 and nt6_on and -(-B // tb11) <= (ncu if ncu > 0 else 256)
    return (6, -(-B // tb6)) if small else (11, -(-B // tb11))


GEMM_WS_FLOATS = 4 << 20                                             # az_trainer_create: gemm_ws_floats


def gemm_plan(M, N, K):
    """(first estimate of the split count, split count after ksplit is rounded up to 32, ksplit): gemm_f32"""
    tiles = -(-M // 64) * -(-N // 64)
    splits = 1
    if tiles < 256 and K >= 1024:
        splits = min(-(-512 // tiles), -(-K // 256))
        while splits > 1 and splits * M * N > GEMM_WS_FLOATS:
            splits -= 1
    ksplit = -(-K // splits)
    ksplit = -(-ksplit // 32) * 32
    return splits, max(1, -(-K // ksplit)), ksplit


# ---------------------------------------------------------------------------------------------- trainers on exact networks
@functools.lru_cache(maxsize=None)
def _mem(game):
    """one replay memory per game with MEM_SAMPLES samples (the records of a few self-play games, pushed repeatedly: the seams never
    read the samples, the trainer only takes its batch size from min(batch_size, #samples))"""
    import azhip
    gspec = getattr(azhip, SPECS[game])()
    with azhip.Engine(game=game, oracle=azhip.ORACLE_HASH, num_workers=8, batch_size=8, num_iters_per_turn=16,
                      dirichlet_noise_eps=0.25, cpuct=1.0, reset_every=1, temperature=([0], [1.0]), seed=3,
                      max_moves_per_game=200 if game == 2 else 0) as e:
        games, moves, ng, nm, _ = e.selfplay_run(12)
    mem = azhip.MemoryBuffer(gspec, MEM_SAMPLES + nm)
    while len(mem) < MEM_SAMPLES:
        mem.push_records(games, moves, ng, nm, 1.0)
    atexit.register(mem.close)
    return gspec, mem


def _int_weights(F, seed):
    """Flux W[kw, kh, ci, co] of one 3x3 F -> F convolution, integers in [-2, 2]"""
    return np.random.default_rng(seed).integers(-2, 3, size=(3, 3, F, F)).astype(np.float32)


@contextlib.contextmanager
def _trainer(game, F, B):
    """a 1-block trainer of batch B whose two F -> F convolutions (tower layers 1 and 2) carry integer weights; yields
    (Trainer, handle, {layer: Flux W}, CU count)"""
    import azhip
    gspec, mem = _mem(game)
    assert 2 <= B <= MEM_SAMPLES
    hp = azhip.ResNetHP(num_blocks=1, num_filters=F, num_policy_head_filters=32, num_value_head_filters=32)
    blob = random_params(game, hp, seed=1)
    Wl, off = {}, 0
    for name, shape in param_layout(game, hp):
        n = int(np.prod(shape))
        for layer, nm in ((1, "block0.conv1.W"), (2, "block0.conv2.W")):
            if name == nm:
                Wl[layer] = _int_weights(F, 100 * game + layer)
                blob[off:off + n] = Wl[layer].reshape(-1, order="F")
        off += n
    nn = azhip.ResNet(gspec, hp, params=blob)
    lp = azhip.LearningParams(samples_weighing_policy=0, l2_regularization=0.0, loss_computation_batch_size=64, batch_size=B,
                              use_position_averaging=False)
    with azhip.Trainer(gspec, nn, mem, lp, use_symmetries=False) as tr:
        h = tr._trainer()
        assert tr.batch_size() == B
        yield tr, h, Wl, tr._eng.device_info()[1]


def _ints(rng, shape, lo=-3, hi=3):
    """integers in [lo, hi] as fp32 rows, no all-zero row"""
    a = rng.integers(lo, hi + 1, size=shape).astype(np.float32)
    a[~a.any(axis=1), 0] = 1.0
    return a


def _fn(name, *argtypes):
    from azhip import _lib as L
    f = getattr(L.lib(), name)
    f.restype, f.argtypes = C.c_int, list(argtypes)
    return lambda *a: L.check(f(*a))


# ---------------------------------------------------------------------------------------------- weight gradient
def _wgrad(h, a, dg, F):
    f = _fn("az_debug_trainer_wgrad", C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64)
    out = np.full((9, F, F), np.nan, dtype=np.float32)
    f(h, _vp(a), _vp(dg), a.size, _vp(out), out.size)
    return out


def _wgrad_ref(game, a, dg, B, F):
    """out[tap][ci][co] = a_shifted.T @ dg over the rows whose neighbour at the tap's offset is on the board (float64: exact integers)"""
    W, H = _DIMS[game][:2]
    a4, d4 = a.astype(np.float64).reshape(B, H, W, F), dg.astype(np.float64).reshape(B, H, W, F)
    out = np.zeros((9, F, F))
    for tap in range(9):
        dy, dx = tap // 3 - 1, tap % 3 - 1
        y0, y1, x0, x1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
        if y1 > y0 and x1 > x0:
            out[tap] = a4[:, y0 + dy:y1 + dy, x0 + dx:x1 + dx].reshape(-1, F).T @ d4[:, y0:y1, x0:x1].reshape(-1, F)
    return out


# (game, filters, batch, NBC, boards per workgroup on 256 CUs) -- what the case is named for; chunks of a workgroup = NBC, NBC, ..., rest
WGRAD_CASES = [
    (0, 128, 50, 1, [1]),              # fewer boards than workgroups: 50 workgroups of one board
    (0, 128, 255, 1, [3]),             # 85 workgroups x 3 boards, every one the same
    (0, 128, 256, 1, [3, 4]),          # the first workgroup holds one more
    (0, 128, 345, 1, [4, 5]),
    (0, 128, 515, 1, [6, 7]),
    (0, 128, 1024, 1, [12, 13]),       # the shipped batch (params.jl: batch_size = 1024 at 5 x 128)
    (0, 128, 1027, 1, [12, 13]),
    (2, 128, 345, 3, [4, 5]),          # chunks 3+1 and 3+2: the zero fill of a partial last chunk, the store into LDS just consumed
    (2, 128, 1024, 3, [12, 13]),       # 3+3+3+3 and 3+3+3+3+1: the prefetch's steady state, a last chunk of one board
    (1, 128, 600, 5, [7, 8]),          # 5+2 and 5+3
    (0, 64, 1024, 3, [4]),             # 256 workgroups, 3+1
    (0, 64, 1028, 3, [4, 5]),          # 3+1 and 3+2
    (2, 64, 100, 9, [1]),              # fewer boards than workgroups, the 8-wavefront form
    (2, 64, 2400, 9, [9, 10]),         # 9 and 9+1
]


@pytest.mark.parametrize("game,F,B,nbc,boards", WGRAD_CASES, ids=["%s-%d-%d" % (NAMES[c[0]], c[1], c[2]) for c in WGRAD_CASES])
def test_wgrad16_is_exact(game, F, B, nbc, boards):
    """k_wgrad16 + k_wgrad_reduce against float64 sums of integer products, twice on one trainer with different inputs: stale LDS rows
    (a partial last chunk must not keep the boards of the chunk before), a stale partial buffer or a wrong board range are bit differences"""
    W, H = _DIMS[game][:2]
    R = B * W * H
    assert 9 * (B * W * H) < 2 ** 24                                # hard bound of any partial sum: |a| |dg| <= 9 per row
    with _trainer(game, F, B) as (tr, h, _, ncu):
        splits, got_nbc, got_boards = wgrad_plan(game, F, B, ncu)
        assert (got_nbc, got_boards) == (nbc, boards), "on %d CUs this case gives %d workgroups, NBC %d, boards per workgroup %s: not what it is named for" % (ncu, splits, got_nbc, got_boards)
        print("wgrad %s F=%d B=%d: %d workgroups per tap group, chunks %s" % (NAMES[game], F, B, splits, [_chunks(nbc, n) for n in boards]))
        rng = np.random.default_rng(1000 * B + F + game)
        for rep in range(2):
            a, dg = _ints(rng, (R, F)), _ints(rng, (R, F))
            want = _wgrad_ref(game, a, dg, B, F)
            assert np.abs(want).max() < 2 ** 24 and np.abs(want).max() > 0
            got = _wgrad(h, a, dg, F).astype(np.float64)
            bad = np.argwhere(got != want)
            assert bad.size == 0, (rep, len(bad), bad[:4].tolist(), [(got[tuple(i)], want[tuple(i)]) for i in bad[:4]])


# ---------------------------------------------------------------------------------------------- convolution
def _conv(h, layer, dgrad, x, second, bn, F):
    f = _fn("az_debug_trainer_conv", C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
            C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32))
    out = np.full(x.shape, np.nan, dtype=np.float32)
    nparts = C.c_int32(-1)
    if dgrad:
        f(h, layer, 1, _vp(x), _vp(second), None, None, x.size, _vp(out), None, None, C.byref(nparts))
        return out, nparts.value
    a_out, sums = np.full(x.shape, np.nan, dtype=np.float32), np.full((2, F), np.nan)
    f(h, layer, 0, _vp(x), None, _vp(bn), _vp(second), x.size, _vp(out), _vp(a_out), _vp(sums), C.byref(nparts))
    return out, a_out, sums, nparts.value


def _torch_w(Wflux):
    """the kernel flip of TorchNet._conv (tests/test_train_gpu.py): Flux W[kw, kh, ci, co] of a true convolution -> conv2d's (co, ci, ky, kx)"""
    return torch.tensor(Wflux, dtype=torch.float64).flip(0, 1).permute(3, 2, 1, 0).contiguous()


def _nchw(game, rows, B):
    W, H = _DIMS[game][:2]
    return torch.tensor(rows.astype(np.float64)).reshape(B, H, W, -1).permute(0, 3, 1, 2).contiguous()


def _rows(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).numpy()


def _bn_consts(rng, F):
    """[4][F]: integer mean, invstd in {0.5, 1}, gamma in {+-1, +-2}, integer beta -- every operation of BnIn is then exact in fp32"""
    return np.stack([rng.integers(-1, 2, F), rng.choice([0.5, 1.0], F), rng.choice([-2.0, -1.0, 1.0, 2.0], F), rng.integers(-1, 2, F)]).astype(np.float32)


def _check_exact(what, got, want):
    got = np.asarray(got, dtype=np.float64)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, len(bad), bad[:4].tolist(), [(got[tuple(i)], want[tuple(i)]) for i in bad[:4]])


def _conv_case(game, F, B, layer, tiles, ncu_for_plan=None, nt6_on=True):
    """forward (BnIn + column sums; layer 2 with the skip input) and data gradient (without and with addend) of one tower layer against
    fp64 conv2d / autograd, twice on one trainer with different inputs; asserts the tile count the seam reports"""
    with _trainer(game, F, B) as (tr, h, Wl, ncu):
        nt, nparts = conv_plan(game, F, B, ncu, nt6_on)
        assert nt == tiles, "on %d CUs this batch runs the %d-tile form, the case is named for the %d-tile form" % (ncu, nt, tiles)
        W, H = _DIMS[game][:2]
        R = B * W * H
        w = _torch_w(Wl[layer])
        rng = np.random.default_rng(7 * B + F + game + layer)
        # hard bounds of any partial sum: |a_out| <= 2 * (3 + 1) * 1 + 1 + 3 = 12 in halves, |w| <= 2, 9 F products
        assert 2 * 12 * 2 * 9 * F < 2 ** 24 and 3 * 2 * 9 * F + 3 < 2 ** 24
        for rep in range(2):
            # forward
            g, bn = _ints(rng, (R, F)), _bn_consts(rng, F)
            res = _ints(rng, (R, F)) if layer == 2 else None
            b64 = bn.astype(np.float64)
            a_want = b64[2] * ((g.astype(np.float64) - b64[0]) * b64[1]) + b64[3]
            if res is not None:
                a_want = a_want + res
            a_want = np.maximum(a_want, 0.0)
            out_want = _rows(torch.nn.functional.conv2d(_nchw(game, a_want, B), w, None, padding=1))
            sums_want = np.stack([out_want.sum(axis=0), (out_want ** 2).sum(axis=0)])
            assert np.abs(out_want).max() < 2 ** 24 and 4 * np.abs(sums_want).max() < 2 ** 53 and np.abs(out_want).max() > 0
            out, a_out, sums, np_got = _conv(h, layer, 0, g, res, bn, F)
            assert np_got == nparts, (np_got, nparts, nt)
            _check_exact("a_out", a_out, a_want)
            _check_exact("forward", out, out_want)
            _check_exact("column sums", sums, sums_want)
            # data gradient: the vector-Jacobian product of the same convolution
            dg, addend = _ints(rng, (R, F)), _ints(rng, (R, F))
            x = torch.zeros(B, F, H, W, dtype=torch.float64, requires_grad=True)
            (da,) = torch.autograd.grad(torch.nn.functional.conv2d(x, w, None, padding=1), x, grad_outputs=_nchw(game, dg, B))
            da_want = _rows(da)
            assert np.abs(da_want).max() + 3 < 2 ** 24 and np.abs(da_want).max() > 0
            out, np_got = _conv(h, layer, 1, dg, None, None, F)
            assert np_got == nparts
            _check_exact("data gradient", out, da_want)
            out, np_got = _conv(h, layer, 1, dg, addend, None, F)
            _check_exact("data gradient + addend", out, da_want + addend)


def _ragged(game, nt):
    tb = _tb(game, nt)
    return [b for b in (tb - 1, tb, tb + 1, 2 * tb + 1) if b >= 2]      # a trainer needs two samples (batch statistics)


CONV128 = [(g, b) for g in (0, 1, 2) for b in _ragged(g, 11) + [1024]]
CONV64 = [(g, b) for g in (0, 1, 2) for b in _ragged(g, 6) + [1024]]


@pytest.mark.parametrize("game,B", CONV128, ids=["%s-%d" % (NAMES[g], b) for g, b in CONV128])
def test_conv16_layer_128_filters_is_exact(game, B):
    """the 11-tile form at TB - 1, TB, TB + 1, 2 TB + 1 boards (TB = boards of a workgroup: a ragged last workgroup, a second one) and at 1024"""
    _conv_case(game, 128, B, layer=1 + B % 2, tiles=11)


@pytest.mark.parametrize("game,B", CONV64, ids=["%s-%d" % (NAMES[g], b) for g, b in CONV64])
def test_conv16_layer_64_filters_6_tiles_is_exact(game, B):
    """the 6-tile form (chosen while the 11-tile form would have at most one workgroup per CU) at its ragged batches and at 1024"""
    _conv_case(game, 64, B, layer=1 + B % 2, tiles=6)


@pytest.mark.parametrize("game", [0, 1, 2], ids=[NAMES[g] for g in (0, 1, 2)])
def test_conv16_layer_64_filters_11_tiles_by_switch_is_exact(game, monkeypatch):
    """AZHIP_TRAIN_NT6=0: the 64-filter 11-tile form at a small ragged batch (2 TB + 1: two full workgroups and one board)"""
    monkeypatch.setenv("AZHIP_TRAIN_NT6", "0")
    _conv_case(game, 64, 2 * _tb(game, 11) + 1, layer=2, tiles=11, nt6_on=False)


def test_conv16_layer_64_filters_11_tiles_by_batch_is_exact():
    """Connect-Four B = 1028 with the switch unset: ceil(1028 / 4) = 257 workgroups > 256 CUs, so tr_conv16 takes the 11-tile form by itself"""
    _conv_case(0, 64, 1028, layer=1, tiles=11)


# ---------------------------------------------------------------------------------------------- GEMM
def _gemm(h, ta, tb, M, N, K, alpha, beta, rng, pad=(3, 5, 2)):
    """one call of the seam on integer matrices with leading dimensions larger than the rows; returns (got, want) of the whole C
    buffer: the padding columns of C must come back untouched"""
    f = _fn("az_debug_trainer_gemm", C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_int32, C.c_int64,
            C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_void_p, C.c_int32, C.c_int64)
    ra, ca, rb, cb = (K, M, N, K) if ta and tb else (K, M, K, N) if ta else (M, K, N, K) if tb else (M, K, K, N)
    lda, ldb, ldc = ca + pad[0], cb + pad[1], N + pad[2]
    A, Bm, Cm = (rng.integers(-3, 4, size=s).astype(np.float32) for s in ((ra, lda), (rb, ldb), (M, ldc)))
    opA = (A[:, :ca].T if ta else A[:, :ca]).astype(np.float64)
    opB = (Bm[:, :cb].T if tb else Bm[:, :cb]).astype(np.float64)
    assert 9 * K + 3 < 2 ** 23                                        # hard bound of any partial sum; alpha = 0.5 makes halves
    want = Cm.astype(np.float64)
    want[:, :N] = alpha * (opA @ opB) + beta * want[:, :N]
    got = Cm.copy()
    f(h, int(ta), int(tb), M, N, K, alpha, _vp(A), lda, A.size, _vp(Bm), ldb, Bm.size, beta, _vp(got), ldc, got.size)
    return got.astype(np.float64), want


EDGES_MN = (1, 63, 64, 65, 130)
EDGES_K = (1, 27, 31, 32, 33, 1023, 1024, 1025, 4097)
AB = ((1.0, 0.0), (0.5, 1.0), (1.0, 1.0), (0.5, 0.0))


@pytest.mark.parametrize("ta,tb", [(0, 0), (1, 0), (0, 1), (1, 1)], ids=["NN", "TN", "NT", "TT"])
def test_gemm_tile_edges_are_exact(ta, tb):
    """every M, N in {1, 63, 64, 65, 130} with every K in {1, 27, 31, 32, 33, 1023, 1024, 1025, 4097}; (alpha, beta) walks through
    {1, 0.5} x {0, 1} along the list, so each K and each M meets all four"""
    with _trainer(1, 64, 2) as (tr, h, _, ncu):
        rng = np.random.default_rng(10 + 2 * ta + tb)
        i, split_seen = 0, set()
        for K in EDGES_K:
            for M in EDGES_MN:
                for N in EDGES_MN:
                    alpha, beta = AB[i % 4]
                    i += 1
                    got, want = _gemm(h, ta, tb, M, N, K, alpha, beta, rng)
                    split_seen.add(gemm_plan(M, N, K)[1])
                    assert np.array_equal(got, want), (M, N, K, alpha, beta, gemm_plan(M, N, K), np.argwhere(got != want)[:4].tolist())
        assert {1, 4, 5, 17} <= split_seen                           # unsplit, K = 1024, 1025 (a short last split of 129), 4097 (a last split of 1)


def test_gemm_split_count_recomputed_and_reduce_tails_are_exact():
    """(a) shapes whose split count changes when ksplit is rounded up to 32 (the first estimate would leave empty splits at the end);
    (b) every split count 3 ... 21 (the rule cannot give 2) through k_gemm_reduce: its 16-stride loop (from 13 splits on) and its 4-stride tail"""
    with _trainer(1, 64, 2) as (tr, h, _, ncu):
        rng = np.random.default_rng(99)
        for (ta, tb, M, N, K), (alpha, beta) in zip([(1, 0, 130, 130, 15000), (0, 0, 320, 320, 5400), (0, 1, 130, 130, 15000), (1, 1, 320, 320, 5400)], AB):
            first, final, ksplit = gemm_plan(M, N, K)
            assert final < first and (final - 1) * ksplit < K, (first, final, ksplit)
            got, want = _gemm(h, ta, tb, M, N, K, alpha, beta, rng)
            assert np.array_equal(got, want), (M, N, K, first, final, np.argwhere(got != want)[:4].tolist())
        seen = set()
        for s in range(3, 22):
            # K >= 1024 gives at least 4 splits unless the tiles limit them: 196 tiles -> ceil(512 / 196) = 3 (two splits need 256 tiles, which never split)
            M, N, K = (896, 896, 1024) if s == 3 else (65, 63, 1024) if s == 4 else (65, 63, 256 * s - 3)
            first, final, ksplit = gemm_plan(M, N, K)
            assert first == final == s
            seen.add(final)
            alpha, beta = AB[s % 4]
            got, want = _gemm(h, s % 2, (s // 2) % 2, M, N, K, alpha, beta, rng)
            assert np.array_equal(got, want), (s, K, np.argwhere(got != want)[:4].tolist())
        assert seen == set(range(3, 22))


@pytest.mark.parametrize("game", [0, 1, 2], ids=[NAMES[g] for g in (0, 1, 2)])
def test_gemm_shapes_of_the_step_at_batch_1024_are_exact(game):
    """the optimiser step's own products at B = 1024, 128 filters, 32 head filters: the weight gradients (transposed A, K = B or K = B x positions:
    split reductions), the forward products and the data gradients (transposed B, one of them accumulating)"""
    W, H, Cin, A = _DIMS[game]
    P, F, nf, B = W * H, 128, 32, 1024
    R = B * P
    shapes = [(1, 0, P * nf, A, B, 0.0), (1, 0, F, 1, B, 0.0), (1, 0, P * nf, F, B, 0.0), (1, 0, F, nf, R, 0.0), (1, 0, 9 * Cin, F, R, 0.0),      # weight gradients
              (0, 0, R, F, 9 * Cin, 0.0), (0, 0, R, nf, F, 0.0), (0, 0, B, A, P * nf, 0.0), (0, 0, B, F, P * nf, 0.0), (0, 0, B, 1, F, 0.0),      # forward
              (0, 1, B, P * nf, A, 0.0), (0, 1, B, F, 1, 0.0), (0, 1, B, P * nf, F, 0.0), (0, 1, R, F, nf, 0.0), (0, 1, R, F, nf, 1.0)]           # data gradients
    with _trainer(game, 64, 2) as (tr, h, _, ncu):
        rng = np.random.default_rng(5 + game)
        nsplit = 0
        for ta, tb, M, N, K, beta in shapes:
            nsplit += gemm_plan(M, N, K)[1] > 1
            got, want = _gemm(h, ta, tb, M, N, K, 1.0, beta, rng)
            assert np.array_equal(got, want), (ta, tb, M, N, K, gemm_plan(M, N, K), np.argwhere(got != want)[:4].tolist())
        assert nsplit >= 5                                           # every weight gradient is a split reduction at this batch


# ---------------------------------------------------------------------------------------------- the seams check their arguments
def test_seams_refuse_wrong_sizes():
    from azhip import _lib as L
    with _trainer(1, 64, 4) as (tr, h, _, ncu):
        n = 4 * 9 * 64
        x = np.ones(n, dtype=np.float32)
        out = np.zeros(9 * 64 * 64, dtype=np.float32)
        for call in (lambda: _fn("az_debug_trainer_wgrad", C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64)(h, _vp(x), _vp(x), n - 1, _vp(out), out.size),
                     lambda: _fn("az_debug_trainer_wgrad", C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64)(h, _vp(x), _vp(x), n, _vp(out), out.size + 1),
                     lambda: _conv(h, 3, 1, x.reshape(-1, 64), None, None, 64),
                     lambda: _conv(h, 1, 1, x[:-64].reshape(-1, 64), None, None, 64)):
            with pytest.raises(L.AzError):
                call()
        f = _fn("az_debug_trainer_gemm", C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_int32, C.c_int64,
                C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_void_p, C.c_int32, C.c_int64)
        a = np.ones(64, dtype=np.float32)
        with pytest.raises(L.AzError):
            f(h, 0, 0, 8, 8, 8, 1.0, _vp(a), 7, 56, _vp(a), 8, 64, 0.0, _vp(a), 8, 64)      # lda shorter than a row
        with pytest.raises(L.AzError):
            f(h, 0, 0, 8, 8, 8, 1.0, _vp(a), 8, 64, _vp(a), 8, 64, 0.0, _vp(a), 8, 63)      # C one float short
