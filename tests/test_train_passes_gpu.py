"""The optimiser step's reductions and pointwise passes one at a time against the exact references of tests/train_pass_refs.py, at the
shapes where they can go wrong.  tests/test_train_gpu.py (and its SimpleNet and 9x9 twins) hold the step end to end to 1e-3 of each
gradient array's largest entry: a column sum over 43 008 rows that drops one row moves a batch mean by 2e-5 of a typical value and
passes there.  Here the kernels run through the debug seams of csrc/train.hip (az_debug_trainer_colsum / _bn / _im2col / _loss): the
trainer's own launch helpers with their dispatch rules, t->part, t->sums, t->bn_mf, the counter of tr_finish and AZHIP_TRAIN_FINISH_INSIDE
as a step has them.

Exactness by construction (tests/exact_nets.py, train_pass_refs.py): small-integer inputs, means of integers and halves, invstd / gamma /
momentum powers of two, integer running statistics -- every fp32 product is exact, the double partial sums are exact in any order, the
comparison is `==`.  Two places are not exact by construction and say so where they are tested: the batch statistics at a row count
that is no power of two (invstd and the running variance: 1 fp32 ulp), and the loss (below).

Every case asserts what it reaches from the launch arithmetic restated in train_pass_refs.py -- which first-stage kernel tr_colsum
dispatched and with how many chunks and column blocks (the seam reports them), which row loops of k_tr_colsum1v lane 0 and the last live
lane ran, nsub of tr_finish, the strides of k_tr_colsum_final, which loss kernel ran -- so a changed constant in train.hip makes a case
fail instead of quietly testing something smaller.  Every column-sum call is made twice on the same trainer with different inputs: stale
partials or a counter of tr_finish not back at zero are bit differences.

The loss.  k_tr_loss and k_tr_loss_wide are held to each other with `==` on identical inputs (the wide kernel's comment promises the same
operations in the same order) and to the float64 loss with its analytic gradient within 4 e, where e is the largest deviation of the
Float32 restatement of k_tr_loss (train_pass_refs.loss32: one rounding per operation, the oracle's expf / logf / tanhf) from the float64
reference over the same cases, per figure -- dlogits relative to each row's largest reference entry, dt and the four per-sample terms
relative to the value with a floor of 1e-6.  The bound comes from the reference's own error, computed when the test runs; the device may
round single operations differently, it does not perform more of them.  Measured e (CPU):
    dlogits 4.9e-5   dt 5.9e-4   w 0   kl 7.7e-2   mse 3.7e-5   inv 4.9e-1
(kl and inv: rows whose value lies at the 1e-6 floor -- q = 1 gives log(1 + eps), S = 1 within a rounding -- where one fp32 rounding
is a tenth of the floor; on every other row a dropped action or a swapped sample is orders of magnitude above the bound.)
Device vs float64 (MI355X), the largest over all cases and both kernels:
    dlogits 4.9e-5   dt 5.9e-4   w 0   kl 7.7e-2   mse 3.7e-5   inv 4.9e-1
-- the same as e in every figure: the library is built with -ffp-contract=off, so the device rounds as the restatement does.  The test
prints the device's figures of every case.
"""
import atexit
import contextlib
import ctypes as ct
import functools

import numpy as np
import pytest

import train_pass_refs as T
from azhip.network import _DIMS, param_layout, random_params, simple_param_layout

pytestmark = pytest.mark.gpu
f32 = np.float32
SPECS = {0: "ConnectFourSpec", 1: "TicTacToeSpec", 2: "MancalaSpec", 3: "Go9PlanesSpec"}
NAMES = {0: "c4", 1: "ttt", 2: "mancala", 3: "go9"}
NSAMPLES = 1100                                                      # >= the largest batch here (1025)
R_SET = (2, 63, 64, 65, 129, 64 * 5 + 3)


def _vp(a):
    return a.ctypes.data_as(ct.c_void_p) if a is not None else None


def _fn(name, *argtypes):
    from azhip import _lib as L
    f = getattr(L.lib(), name)
    f.restype, f.argtypes = ct.c_int, list(argtypes)
    return lambda *a: L.check(f(*a))


# ---------------------------------------------------------------------------------------------- trainers
@functools.lru_cache(maxsize=None)
def _data(game):
    """one tensor data set per game: the seams never read the samples, a trainer takes min(batch_size, #samples) from it"""
    import azhip
    W, H, C, A = _DIMS[game]
    rng = np.random.default_rng(game)
    n = NSAMPLES
    Am = np.ones((n, A), dtype=f32)
    td = azhip.TensorDataset(getattr(azhip, SPECS[game])(), np.ones(n), rng.integers(0, 2, size=(n, C, H, W)), Am, Am / A, np.zeros(n))
    atexit.register(td.close)
    return td


@contextlib.contextmanager
def _trainer(game, B, F=64, simple=None, blob=None, l2=0.0):
    """(Trainer, handle) of batch B: a 1-block ResNet of F filters, or the SimpleNet `simple`"""
    import azhip
    gspec = getattr(azhip, SPECS[game])()
    if simple is not None:
        nn = azhip.SimpleNet(gspec, simple, params=blob, seed=3)
    else:
        hp = azhip.ResNetHP(num_blocks=1, num_filters=F, num_policy_head_filters=32, num_value_head_filters=32)
        nn = azhip.ResNet(gspec, hp, params=blob if blob is not None else random_params(game, hp, seed=1))
    lp = azhip.LearningParams(samples_weighing_policy=0, l2_regularization=l2, loss_computation_batch_size=64, batch_size=B, use_position_averaging=False)
    assert 2 <= B <= NSAMPLES
    with azhip.Trainer(gspec, nn, _data(game), lp) as tr:
        h = tr._trainer()
        assert tr.batch_size() == B
        yield tr, h


def _big():
    """Connect-Four, 1 x 128 filters, batch 1024: partials for 1025 x 2 x 128 >= 672 chunks of 128 columns, sums and means for 128 columns"""
    return _trainer(0, 1024, F=128)


def _dense():
    """a SimpleNet of width 256 at batch 384: R = batch -> 6 chunks, sums and means for 256 columns (the widths 129 and 200)"""
    from azhip.network import SimpleNetHP
    return _trainer(1, 384, simple=SimpleNetHP(width=256, depth_common=1, use_batch_norm=True))


# ---------------------------------------------------------------------------------------------- column sums
_COLSUM = (ct.c_void_p, ct.c_int32, ct.c_int64, ct.c_int32, ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.c_int64, ct.c_void_p, ct.c_int32, ct.c_float,
           ct.c_int32, ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.c_void_p)


def _colsum(h, mode, case, fin_mode=0, fc=None, with_bias=True):
    """one call of az_debug_trainer_colsum: (sums[2][C], fin_out[4][C] or None, (chunks, vectorised, inside, gridDim.y))"""
    x = case["x"]
    R, Cc = x.shape
    stat = np.stack([case["mean"], case["invstd"]]) if mode == 1 else None
    fin_in = np.stack([fc["bias"], fc["run_mean"], fc["run_var"]]) if fin_mode == 1 else None
    sums = np.full((2, Cc), 7.0)
    fin_out = np.full((4, Cc), np.nan, dtype=f32) if fin_mode else None
    info = np.full(4, -1, dtype=np.int32)
    _fn("az_debug_trainer_colsum", *_COLSUM)(h, mode, R, Cc, _vp(x), _vp(case.get("out_act")), _vp(case.get("g")), x.size, _vp(stat), fin_mode,
                                             fc["momentum"] if fc else 0.0, int(with_bias), _vp(fin_in), _vp(sums), _vp(fin_out), _vp(info))
    return sums, fin_out, (int(info[0]), bool(info[1]), bool(info[2]), int(info[3]))


def _eq(what, got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, len(bad), bad[:4].tolist(), [(got[tuple(i)], want[tuple(i)]) for i in bad[:4]])


def _check_colsum(h, rng, mode, R, Cc, fin_mode, inside=False, case=None, with_bias=True, want=None):
    """one seam call against colsum + finish; asserts the plan the seam reports; returns the plan"""
    case = case if case is not None else T.colsum_case(rng, mode, R, Cc)
    fc = T.finish_case(rng, Cc) if fin_mode == 1 else None
    plan = T.colsum_plan(mode, R, Cc, inside)
    sums, fin_out, info = _colsum(h, mode, case, fin_mode, fc, with_bias)
    what = "mode %d R %d C %d fin %d %s" % (mode, R, Cc, fin_mode, plan)
    assert info == plan, (what, info)
    want = want if want is not None else T.colsum(mode, **case)
    if plan[2]:
        assert np.isnan(sums).all(), what                            # tr_finish keeps the sums in LDS: what it derives from them is held below
    else:
        _eq(what + " sums", sums, want)
    if fin_mode == 1:
        fcb = dict(fc, bias=fc["bias"] if with_bias else None)
        mean, invstd, rm, rv = T.finish(want, 1, R, **fcb)
        _eq(what + " mean", fin_out[0], mean)
        _eq(what + " run_mean", fin_out[2], rm)
        if R & (R - 1) == 0:                                         # m = s0 / R a short dyadic: s1 / R - m m is exact, whatever is fused
            _eq(what + " invstd", fin_out[1], invstd)
            _eq(what + " run_var", fin_out[3], rv)
        else:
            # a ragged R: m is a rounded quotient, and a compiler free to fuse s1 / R - m * m into one operation rounds that double once
            # instead of twice; the difference of one double ulp can only move the rounding to float of invstd and of the variance: 1 fp32 ulp
            assert T.ulps32(fin_out[1], invstd).max() <= 1 and T.ulps32(fin_out[3], rv).max() <= 1, (what, T.ulps32(fin_out[1], invstd).max(), T.ulps32(fin_out[3], rv).max())
    elif fin_mode == 2:
        dbeta, dgamma, mf = T.finish(want, 2, R)
        _eq(what + " dbeta", fin_out[0], dbeta)
        _eq(what + " dgamma", fin_out[1], dgamma)
        _eq(what + " mf", fin_out[2:], mf)
    elif fin_mode == 3:
        _eq(what + " out0", fin_out[0], T.finish(want, 3, R)[0])
    return plan


PATTERNS = {"1", "2", "21", "4", "41", "42", "421"}                  # which of the loops (four, two, one rows in flight) a lane runs


def test_colsum1v_every_tail_length():
    """k_tr_colsum1v at C in {4 .. 128}, R = 128 + n for every tail n = 1 .. 64 (three chunks, the last of n rows): all three row loops and
    their hand-overs per lane.  C = 4: 256 row lanes, those at or above n have nothing; C = 128: 8 lanes, the four-in-flight loop runs twice
    in the full chunks.  Finisher 2 (the step's), 0, 3 and 1 in turn."""
    pat = lambda t: "".join(k for k, n in zip("421", t) if n)
    lane0, last = set(), set()
    with _big() as (tr, h):
        rng = np.random.default_rng(11)
        for Cc in (4, 8, 16, 32, 64, 128):
            RL = T.colsum1v_lanes(Cc)
            assert T.colsum1v_loops(Cc, 64, 0) == {256: (0, 0, 1), 128: (0, 0, 1), 64: (0, 0, 1), 32: (0, 1, 0), 16: (1, 0, 0), 8: (2, 0, 0)}[RL]
            for n in range(1, 65):
                lane0.add(pat(T.colsum1v_loops(Cc, n, 0)))
                last.add(pat(T.colsum1v_loops(Cc, n, min(RL, n) - 1)))
                assert n >= RL or T.colsum1v_loops(Cc, n, n) == (0, 0, 0)           # a lane at or above the chunk's rows runs none
                for rep in range(2):
                    plan = _check_colsum(h, rng, 1, 128 + n, Cc, (2, 0, 3, 1)[(n + rep) % 4])
                    assert plan == (3, True, False, 1)
    assert lane0 == PATTERNS and last >= PATTERNS, (lane0, last)


GENERIC1_C = (1, 2, 12, 20, 100, 129, 200)                           # what tr_colsum sends to k_tr_colsum<1>: C % 4 != 0, 256 % (C / 4) != 0, C > 128


@pytest.mark.parametrize("wide", [False, True], ids=["to-128", "over-128"])
def test_colsum_generic_mode_1(wide):
    with (_dense() if wide else _big()) as (tr, h):
        rng = np.random.default_rng(12)
        for Cc in [c for c in GENERIC1_C if (c > 128) == wide]:
            for R in R_SET:
                for rep in range(2):
                    plan = _check_colsum(h, rng, 1, R, Cc, (2, 0)[rep])
                    assert plan == (-(-R // 64), False, False, -(-Cc // 64)) and (plan[3] > 1) == (Cc >= 65)


MODE02_C = (1, 7, 9, 32, 63, 64, 65, 82, 128, 200)                   # the policy bias at 7, 9, 82 columns, the value head's one, SimpleNet widths


@pytest.mark.parametrize("wide", [False, True], ids=["to-128", "over-128"])
def test_colsum_modes_0_and_2(wide):
    """k_tr_colsum<0> with the batch-statistics finisher (with and without a bias) and <2> with the bias-gradient finisher, as the step pairs them"""
    with (_dense() if wide else _big()) as (tr, h):
        rng = np.random.default_rng(13)
        for Cc in [c for c in MODE02_C if (c > 128) == wide]:
            for R in R_SET:
                for rep in range(2):
                    plan = _check_colsum(h, rng, 0, R, Cc, (1, 0)[rep], with_bias=bool(R % 2))
                    assert plan == (-(-R // 64), False, False, -(-Cc // 64))
                    _check_colsum(h, rng, 2, R, Cc, 3)


NCHUNKS = (1, 2, 63, 64, 65, 129, 672)


def _rows_of(nchunks):
    """64, 128 and 4096 rows are powers of two (exact batch statistics); 672 chunks = 43 008 rows, the shipped batch; else a ragged last chunk"""
    return 64 * nchunks if nchunks in (1, 2, 64, 672) else 64 * (nchunks - 1) + 17


@pytest.mark.parametrize("inside", [False, True], ids=["separate-launch", "finish-inside"])
def test_second_stage_every_chunk_count_and_finisher(inside, monkeypatch):
    """k_tr_colsum_final (64-stride loop, then a tree) and tr_finish (AZHIP_TRAIN_FINISH_INSIDE=1: the last workgroup by counter, nsub
    sub-sums per pair) over 1 .. 672 chunks with all four finishers, the two inputs of a (C, chunks) pair taking turns"""
    if inside:
        monkeypatch.setenv("AZHIP_TRAIN_FINISH_INSIDE", "1")
        # (mode, C): k_tr_colsum1v at nsub = 32, 4, 2, 1; the generic kernels at 100 columns (threads 200 .. 255 own no pair) and at
        # 65 .. 128 columns, two column blocks: the last workgroup may sit in either
        cases = [(1, 64), (1, 4), (1, 32), (1, 128), (1, 100), (0, 65), (0, 100), (2, 128)]
        assert [T.finish_nsub(c) for c in (4, 32, 64, 100, 128)] == [32, 4, 2, 1, 1]
    else:
        monkeypatch.delenv("AZHIP_TRAIN_FINISH_INSIDE", raising=False)
        cases = [(1, 64), (1, 100), (0, 128), (2, 7)]
    assert [T.final_plan(n) for n in NCHUNKS] == [(1, 1), (1, 2), (1, 63), (1, 64), (2, 64), (3, 64), (11, 64)]
    with _big() as (tr, h):
        rng = np.random.default_rng(14 + inside)
        for i, (mode, Cc) in enumerate(cases):
            for nchunks in NCHUNKS if i == 0 else NCHUNKS[:-1]:      # the 43 008 rows of the shipped batch once: on the step's own pairing, 64 columns in mode 1
                R = _rows_of(nchunks)
                two = [T.colsum_case(rng, mode, R, Cc) for _ in range(2)]
                wants = [T.colsum(mode, **c) for c in two]
                for k, fin_mode in enumerate((1, 2, 3, 0, 2, 1)):
                    plan = _check_colsum(h, rng, mode, R, Cc, fin_mode, inside, case=two[k % 2], want=wants[k % 2])
                    assert plan[0] == nchunks and plan[2] == inside and plan[1] == (mode == 1 and Cc != 100) and plan[3] == (1 if plan[1] else -(-Cc // 64))


# ---------------------------------------------------------------------------------------------- batch norm and dense epilogues
_BN = (ct.c_void_p, ct.c_int32, ct.c_int64, ct.c_int32, ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.c_int32, ct.c_int64,
       ct.c_void_p, ct.c_void_p)


def _bn(h, op, rows, Cc, g=None, first=None, second=None, consts=None, mf=None, flag=0, want_out2=False):
    out = np.full((rows, Cc), np.nan, dtype=f32)
    out2 = np.full((rows, Cc), np.nan, dtype=f32) if want_out2 else None
    consts = np.ascontiguousarray(consts) if consts is not None else None
    _fn("az_debug_trainer_bn", *_BN)(h, op, rows, Cc, _vp(g), _vp(first), _vp(second), _vp(consts), _vp(mf), flag, rows * Cc, _vp(out), _vp(out2))
    return out, out2


def _bn_rows(Cc):
    """a single-digit row count, one whose rows x C is just over 65 536, and one between; none a multiple of the 1024 elements of four workgroups"""
    rows = [7, 131, 65536 // Cc + 1]
    assert all((r * Cc) % 1024 for r in rows) and 65536 < rows[2] * Cc <= 65536 + Cc
    return rows


@pytest.mark.parametrize("Cc", [1, 2, 4, 6, 64, 100, 128])
def test_bn_apply_backward_and_dense_epilogues_are_exact(Cc):
    """k_tr_bn_apply (res present and null), k_tr_bn_bwd<4> (C % 4 == 0) and <1> in place with dy_out present and null, k_tr_bias_act with and
    without relu, k_tr_relu_bwd"""
    with _trainer(1, 4, F=128) as (tr, h):                           # bn_mf holds 128 columns
        rng = np.random.default_rng(20 + Cc)
        for rows in _bn_rows(Cc):
            c = T.bn_case(rng, rows, Cc)
            what = "rows %d C %d " % (rows, Cc)
            for res in (None, c["res"]):
                out, _ = _bn(h, 0, rows, Cc, g=c["g"], second=res, consts=np.stack([c["mean"], c["invstd"], c["gamma"], c["beta"]]))
                _eq(what + "bn_apply res %s" % (res is not None), out, T.bn_apply(c["g"], c["mean"], c["invstd"], c["gamma"], c["beta"], res))
            dg, dy = T.bn_bwd(c["da"], c["a"], c["g"], c["mean"], c["invstd"], c["gamma"], c["mf"].astype(np.float64))
            assert np.abs(dg).max() > 0 and (dy == 0).any() and (dy != 0).any()
            for want2 in (False, True):
                out, out2 = _bn(h, 1, rows, Cc, g=c["g"], first=c["da"], second=c["a"], consts=np.stack([c["mean"], c["invstd"], c["gamma"]]), mf=c["mf"], want_out2=want2)
                _eq(what + "bn_bwd dy_out %s" % want2, out, dg)
                if want2:
                    _eq(what + "bn_bwd dy", out2, dy)
            for relu in (0, 1):
                out, _ = _bn(h, 2, rows, Cc, g=c["g"], consts=c["bias"][None], flag=relu)
                _eq(what + "bias_act relu %d" % relu, out, T.bias_act(c["g"], c["bias"], relu))
            out, _ = _bn(h, 3, rows, Cc, first=c["da"], second=c["a"])
            _eq(what + "relu_bwd", out, T.relu_bwd(c["da"], c["a"]))


# ---------------------------------------------------------------------------------------------- im2col
@pytest.mark.parametrize("game,B", [(g, b) for g in (0, 1, 2, 3) for b in (2, 3)], ids=lambda v: str(v))
def test_im2col_is_exact(game, B):
    """the stem's gather on every geometry a trainer accepts (7x6, 3x3, 14x1, 9x9 with 4 planes): every plane value a unique code of
    (board, plane, y, x), so a read across a board or row edge is a wrong code where the reference has a zero"""
    W, H, Cc, _ = _DIMS[game]
    planes = T.plane_codes(B, Cc, H, W)
    want = T.im2col(planes)
    assert (want == 0).any() and planes.max() < 2 ** 24
    with _trainer(game, B) as (tr, h):
        f = _fn("az_debug_trainer_im2col", ct.c_void_p, ct.c_void_p, ct.c_int64, ct.c_void_p, ct.c_int64)
        for rep in range(2):
            p = planes if rep == 0 else (planes.max() + 1 - planes).astype(f32)
            col = np.full(want.shape, np.nan, dtype=f32)
            f(h, _vp(p), p.size, _vp(col), col.size)
            _eq("im2col %s B %d pass %d" % (NAMES[game], B, rep), col, want if rep == 0 else T.im2col(p))


# ---------------------------------------------------------------------------------------------- loss
_LOSS = (ct.c_void_p, ct.c_int32, ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.c_int64, ct.c_void_p, ct.c_void_p, ct.c_int64, ct.c_float, ct.c_float,
         ct.c_float, ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.c_void_p)


def _loss(h, c, force_wide, terms_in=None):
    """one call of az_debug_trainer_loss: ((dlogits, dt, terms[4][B]), wide kernel ran?, the five step sums of terms_in or None)"""
    B, A = c["logits"].shape
    dl, dt, terms = np.full((B, A), np.nan, dtype=f32), np.full(B, np.nan, dtype=f32), np.full((4, B), np.nan)
    wide = np.full(1, -1, dtype=np.int32)
    sums5 = np.full(5, np.nan) if terms_in is not None else None
    _fn("az_debug_trainer_loss", *_LOSS)(h, int(force_wide), _vp(c["logits"]), _vp(c["tpre"]), _vp(c["Am"]), _vp(c["P"]), B * A, _vp(c["V"]), _vp(c["W"]), B,
                                         c["cinv"], c["rho"], c["gscale"], _vp(dl), _vp(dt), _vp(terms), _vp(wide), _vp(terms_in), _vp(sums5))
    return (dl, dt, terms), bool(wide[0]), sums5


@functools.lru_cache(maxsize=None)
def _e():
    return T.loss_reference_error()


def _int_terms(rng, B):
    """integer-valued per-sample terms: their sums are exact in any order"""
    return rng.integers(-1000, 1001, size=(4, B)).astype(np.float64)


@pytest.mark.parametrize("game,B", T.LOSS_CASES, ids=["%s-%d" % (NAMES[g], b) for g, b in T.LOSS_CASES])
def test_loss_kernels_against_float64_and_each_other(game, B):
    """k_tr_loss (A <= 9) and k_tr_loss_wide (forced at the same A; by itself at 82 actions): device vs float64 within 4 e per figure, narrow
    == wide on identical inputs; then k_tr_step_sums on integer terms, =="""
    A = T.LOSS_GAMES[game]
    c = T.loss_case(game, B)
    want = T.loss64(*T._loss_args(c))
    bound = 4 * _e()
    with _trainer(game, B) as (tr, h):
        rng = np.random.default_rng(B)
        outs = {}
        for force in ((False, True) if A <= T.AZ_MAX_ACTIONS else (False,)):
            terms_in = _int_terms(rng, B)
            got, wide, sums5 = _loss(h, c, force, terms_in)
            plan = T.loss_plan(B, A, force)
            assert wide == plan[0] == (force or game == 3)
            dev = T.loss_deviation(got, want)
            print("loss %s B=%d %s (%d workgroups of %d): device vs float64 %s" % (NAMES[game], B, "wide" if wide else "narrow", plan[1], plan[2], dict(zip(T.LOSS_KINDS, ["%.3g" % v for v in dev]))))
            assert all(np.isfinite(z).all() for z in got) and (dev <= bound).all(), (dict(zip(T.LOSS_KINDS, dev)), dict(zip(T.LOSS_KINDS, bound)))
            _eq("step sums", sums5[:4], terms_in.sum(axis=1))
            outs[wide] = got
        if len(outs) == 2:
            for name, a, b in zip(("dlogits", "dt", "terms"), outs[False], outs[True]):
                assert np.array_equal(a, b), ("narrow != wide", name, np.argwhere(a != b)[:4].tolist())


def test_loss_without_legal_mass_stays_finite():
    """one row whose legal mass underflows to 0 (S ~ e^-80): finiteness only, both kernels, as the second call on a trainer"""
    c = T.loss_case(1, 257, degenerate=True)
    with _trainer(1, 257) as (tr, h):
        _loss(h, T.loss_case(1, 257), False)
        for force in (False, True):
            got, wide, _ = _loss(h, c, force)
            assert wide == force and all(np.isfinite(z).all() for z in got)


@pytest.mark.parametrize("B", [2, 1025])
def test_step_sums_are_exact(B):
    """k_tr_step_sums' 256-stride loop and tree at 2 and at 1025 samples (255, 256, 257 ride on the loss cases): integer terms, ==; the fifth
    sum is k_tr_sumsq over the trainable parameters (float64 products of fp32 values, 1e-12)"""
    import azhip
    hp = azhip.ResNetHP(num_blocks=1, num_filters=64, num_policy_head_filters=32, num_value_head_filters=32)
    blob = random_params(1, hp, seed=1)
    with _trainer(1, B) as (tr, h):
        rng = np.random.default_rng(B)
        for rep in range(2):
            terms_in = _int_terms(rng, B)
            _, _, sums5 = _loss(h, T.loss_case(1, B) if B <= 257 else _tiled_case(B), False, terms_in)
            _eq("step sums B %d" % B, sums5[:4], terms_in.sum(axis=1))
            ssq = float((blob.astype(np.float64)[_trainable(param_layout(1, hp))] ** 2).sum())
            assert abs(sums5[4] - ssq) <= 1e-12 * ssq


def _tiled_case(B):
    c = T.loss_case(1, 257)
    reps = -(-B // 257)
    return {k: (np.ascontiguousarray(np.concatenate([v] * reps)[:B]) if isinstance(v, np.ndarray) else v) for k, v in c.items()}


# ---------------------------------------------------------------------------------------------- sum of squares and the trainable mask
def _trainable(layout):
    return np.array([not (n.endswith(".mean") or n.endswith(".var")) for n, s in layout for _ in range(int(np.prod(s)))])


def _int_blob(layout, seed):
    """weights, biases, gamma, beta integers in [-2, 2]; running mean in {-3, 3}, running variance in {2, 3}: none of them zero"""
    rng = np.random.default_rng(seed)
    parts = []
    for name, shape in layout:
        n = int(np.prod(shape))
        parts.append(rng.choice([-3, 3], size=n) if name.endswith(".mean") else rng.integers(2, 4, size=n) if name.endswith(".var") else rng.integers(-2, 3, size=n))
    return np.concatenate(parts).astype(f32)


@pytest.mark.parametrize("net", ["resnet", "simplenet"])
def test_sum_of_squares_over_the_trainable_mask_is_exact(net):
    """k_tr_sumsq through az_trainer_gradients: an integer blob, l2 = 2^-10 -> Lreg == l2 sum(w^2) over the trainable entries exactly (the sum
    stays below 2^24); a mask that let a running statistic in would move it by an integer (every running statistic is at least 2 in size)"""
    import azhip
    from azhip.network import SimpleNetHP
    if net == "resnet":
        hp = azhip.ResNetHP(num_blocks=1, num_filters=64, num_policy_head_filters=32, num_value_head_filters=32)
        layout, kw = param_layout(1, hp), {}
    else:
        hp = SimpleNetHP(width=100, depth_common=2, use_batch_norm=True)
        layout, kw = simple_param_layout(1, hp), dict(simple=hp)
    blob, mask = _int_blob(layout, 7), _trainable(layout)
    sq = blob.astype(np.float64) ** 2
    want = float(sq[mask].sum())
    assert want < 2 ** 24 and sq[~mask].min() >= 4 and (~mask).sum() > 0
    l2 = 2.0 ** -10
    with _trainer(1, 16, blob=blob, l2=l2, **kw) as (tr, h):
        for rep in range(2):
            loss, parts, grad = tr.gradients(np.arange(16) + rep)
            assert float(parts[2]) == l2 * want, (float(parts[2]) / l2, want, float(sq.sum()))


# ---------------------------------------------------------------------------------------------- the seams check their arguments
def test_pass_seams_refuse_wrong_sizes():
    from azhip import _lib as L
    with _trainer(1, 4) as (tr, h):                                  # 64 filters: sums and means for 64 columns, partials for max(1, 5) x 2 x 64
        rng = np.random.default_rng(0)
        ok = T.colsum_case(rng, 1, 5, 8)
        _check_colsum(h, rng, 1, 5, 8, 2)
        x = np.ones((4, 8), dtype=f32)
        cs, bn = _fn("az_debug_trainer_colsum", *_COLSUM), _fn("az_debug_trainer_bn", *_BN)
        sums, fo, info = np.zeros((2, 200)), np.zeros((4, 200), dtype=f32), np.zeros(4, dtype=np.int32)
        wide = T.colsum_case(rng, 0, 2, 65)
        tall = T.colsum_case(rng, 0, 64 * 6, 64)
        calls = [
            lambda: _colsum(h, 0, wide),                                                            # 65 columns do not fit sums[2][64]
            lambda: _colsum(h, 0, tall),                                                            # 6 chunks x 2 x 64 do not fit the partials
            lambda: cs(h, 0, 4, 8, _vp(x), None, None, 31, None, 0, 0.0, 0, None, _vp(sums), None, _vp(info)),       # n != R C
            lambda: cs(h, 3, 4, 8, _vp(x), None, None, 32, None, 0, 0.0, 0, None, _vp(sums), None, _vp(info)),       # no such mode
            lambda: cs(h, 1, 4, 8, _vp(x), None, None, 32, None, 0, 0.0, 0, None, _vp(sums), None, _vp(info)),       # mode 1 without its arrays
            lambda: cs(h, 0, 4, 8, _vp(x), None, None, 32, None, 1, 0.5, 0, None, _vp(sums), _vp(fo), _vp(info)),    # finisher 1 without its inputs
            lambda: cs(h, 0, 4, 8, _vp(x), None, None, 32, None, 2, 0.0, 0, None, _vp(sums), None, _vp(info)),       # finisher 2 without its output
            lambda: bn(h, 0, 4, 8, _vp(x), None, None, _vp(x), None, 0, 31, _vp(x.copy()), None),                    # n != rows C
            lambda: bn(h, 4, 4, 8, _vp(x), None, None, _vp(x), None, 0, 32, _vp(x.copy()), None),                    # no such op
            lambda: bn(h, 1, 4, 8, _vp(x), _vp(x), _vp(x), _vp(x), None, 0, 32, _vp(x.copy()), None),                # the backward pass without mf
            lambda: _bn(h, 1, 2, 65, g=np.ones((2, 65), dtype=f32), first=np.ones((2, 65), dtype=f32), second=np.ones((2, 65), dtype=f32),
                        consts=np.ones((3, 65), dtype=f32), mf=np.ones((2, 65), dtype=f32)),                       # 65 columns do not fit bn_mf[2][64]
            lambda: _fn("az_debug_trainer_im2col", ct.c_void_p, ct.c_void_p, ct.c_int64, ct.c_void_p, ct.c_int64)(h, _vp(x), 4 * 27 - 1, _vp(np.zeros(4 * 9 * 27, dtype=f32)), 4 * 9 * 27),
            lambda: _fn("az_debug_trainer_im2col", ct.c_void_p, ct.c_void_p, ct.c_int64, ct.c_void_p, ct.c_int64)(h, _vp(np.zeros(4 * 27, dtype=f32)), 4 * 27, _vp(np.zeros(4 * 9 * 27, dtype=f32)), 4 * 9 * 27 + 1),
        ]
        c = T.loss_case(1, 4)
        short = dict(c, logits=c["logits"][:3], Am=c["Am"][:3], P=c["P"][:3])
        calls.append(lambda: _loss(h, short, False))                                                # B A floats short
        calls.append(lambda: _loss(h, dict(c, rho=0.0), False))
        for i, call in enumerate(calls):
            with pytest.raises(L.AzError):
                call()
                pytest.fail("call %d was accepted" % i)
        _check_colsum(h, rng, 1, 5, 8, 2, case=ok)                                                  # and the trainer still works
    from simplenet_ref import TTT_SHIPPED
    with _trainer(1, 4, simple=TTT_SHIPPED) as (tr, h):
        with pytest.raises(L.AzError):                                                              # a dense chain has no stem
            _fn("az_debug_trainer_im2col", ct.c_void_p, ct.c_void_p, ct.c_int64, ct.c_void_p, ct.c_int64)(h, _vp(np.zeros(4 * 27, dtype=f32)), 4 * 27, _vp(np.zeros(4 * 9 * 27, dtype=f32)), 4 * 9 * 27)
