"""The references of tests/train_pass_refs.py held themselves, without a GPU: batch-norm backward and the loss gradient against torch
autograd in float64, im2col against torch's unfold, the sensitivity of the column-sum cases (removing or doubling any single row changes
the reference's bits in both sums), the loop-coverage arithmetic of the k_tr_colsum1v sweep, and the figure `e` the device's loss is
bounded by (tests/test_train_passes_gpu.py)."""
import numpy as np
import pytest
import torch

import train_pass_refs as T

EPS32 = float(T.EPS32)


def test_bn_backward_equals_autograd():
    """dg, dgamma, dbeta and the skip share of a = relu(bn(g) + res) with batch statistics against torch autograd in float64, to 1e-12"""
    rng = np.random.default_rng(1)
    for rows, C, with_res in ((7, 1, False), (50, 6, True), (130, 64, True), (33, 100, False)):
        g, da, res = rng.normal(size=(rows, C)), rng.normal(size=(rows, C)), rng.normal(size=(rows, C))
        gamma, beta = rng.uniform(0.5, 2, size=C) * rng.choice([-1, 1], size=C), rng.normal(size=C)
        tg, tgam, tbeta, tres = (torch.tensor(z, dtype=torch.float64, requires_grad=True) for z in (g, gamma, beta, res))
        z = tgam * (tg - tg.mean(dim=0)) / torch.sqrt(tg.var(dim=0, unbiased=False) + 1e-5) + tbeta
        a = torch.relu(z + tres if with_res else z)
        a.backward(torch.tensor(da))
        dg, dgamma, dbeta, dy = T.bn_layer_bwd(da, g, gamma, beta, res if with_res else None)
        for name, got, want in (("dg", dg, tg.grad), ("dgamma", dgamma, tgam.grad), ("dbeta", dbeta, tbeta.grad)) + ((("dres", dy, tres.grad),) if with_res else ()):
            want = want.numpy()
            assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), (rows, C, name, np.abs(got - want).max())


def _torch_loss(c):
    """gscale sum_i w_i (Lp_i + Lv_i + cinv Linv_i) with the formula of TorchNet.losses (tests/test_train_gpu.py) per sample"""
    f = lambda k: torch.tensor(np.asarray(c[k], dtype=np.float64))
    lg, t = f("logits").requires_grad_(), f("tpre").requires_grad_()
    A, P, V, W = f("Am"), f("P"), f("V"), f("W")
    pm = torch.softmax(lg, dim=1) * A
    sp = pm.sum(dim=1, keepdim=True)
    Ph = pm / (sp + EPS32)
    kl = (P * torch.log(Ph + EPS32)).sum(dim=1) * W
    mse = ((torch.tanh(t) / c["rho"] - V / c["rho"]) ** 2) * W
    inv = (1 - sp).reshape(-1) * W
    (c["gscale"] * (-kl + mse + c["cinv"] * inv).sum()).backward()
    return lg.grad.numpy(), t.grad.numpy(), np.stack([W.numpy(), kl.detach().numpy(), mse.detach().numpy(), inv.detach().numpy()])


@pytest.mark.parametrize("game,B", [(0, 257), (1, 64), (2, 255), (3, 65)])
def test_loss_gradient_equals_autograd(game, B):
    """the analytic gradient of loss64 against autograd of the TorchNet.losses formula in float64, to 1e-12 of each row's largest entry"""
    c = T.loss_case(game, B)
    dl, dt, terms = T.loss64(*T._loss_args(c))
    rl, rt, rterms = _torch_loss(c)
    dev = T.loss_deviation((dl, dt, terms), (rl, rt, rterms))
    scale = np.abs(rl).max(axis=1, keepdims=True)
    assert (np.abs(dl - rl) <= 1e-12 * np.maximum(scale, np.abs(rl).max())).all(), dev
    assert np.abs(dt - rt).max() <= 1e-12 * max(1.0, np.abs(rt).max()), dev
    assert np.abs(terms - rterms).max() <= 1e-12 * max(1.0, np.abs(rterms).max()), dev
    assert np.abs(rl).max() > 0 and np.abs(rt).max() > 0


def test_loss_cases_hold_what_they_are_for():
    seen = set()
    for game, B in T.LOSS_CASES:
        c = T.loss_case(game, B)
        A = c["Am"].shape[1]
        assert A == T.LOSS_GAMES[game] and T.loss_plan(B, A)[0] == (game == 3)
        seen |= {"single"} if (c["Am"].sum(axis=1) == 1).any() else set()
        seen |= {"pzero"} if ((c["P"] == 0) & (c["Am"] > 0)).any() else set()
        seen |= {"w0"} if (c["W"] == 0).any() else set()
        seen |= {"v1"} if ((np.abs(c["V"]) == 1) & (np.abs(c["tpre"]) > 3)).any() else set()
        assert np.ptp(c["logits"]) > 12
    assert seen == {"single", "pzero", "w0", "v1"}
    assert {T.loss_plan(B, 7)[1] for B in T.LOSS_NARROW_B} == {1, 2} and {T.loss_plan(B, 82)[1] for B in T.LOSS_WIDE_B} == {1, 2, 3}


def test_float32_restatement_stays_close_to_float64():
    """e of the loss bound (the device gets 4 e): printed for the docstring of the GPU test, and sane.  Measured: dlogits 4.9e-5 (rows with
    one legal action: gq / den - gu_sum cancels), dt 5.9e-4 (1 - tanh^2 at |t| near 6), mse 3.7e-5; kl 0.077 and inv 0.49 are the rows
    whose value lies at the 1e-6 floor (q = 1: log(1 + eps); S = 1 within rounding), where one fp32 rounding of S is a tenth of the floor."""
    e = T.loss_reference_error()
    print("e =", dict(zip(T.LOSS_KINDS, ["%.3g" % v for v in e])))
    d = dict(zip(T.LOSS_KINDS, e))
    assert d["w"] == 0.0 and 0 < d["dlogits"] < 1e-3 and 0 < d["dt"] < 1e-2 and 0 < d["mse"] < 1e-3 and 0 < d["kl"] < 1 and 0 < d["inv"] < 1


def test_im2col_equals_unfold():
    for B, C, H, W in ((2, 3, 6, 7), (3, 4, 9, 9), (2, 5, 1, 14), (3, 3, 3, 3)):
        planes = T.plane_codes(B, C, H, W)
        col = T.im2col(planes)
        u = torch.nn.functional.unfold(torch.tensor(planes.astype(np.float64)), 3, padding=1)            # [B][C 9][H W], row = c 9 + tap
        want = u.reshape(B, C, 9, H * W).permute(0, 3, 2, 1).reshape(B * H * W, 9 * C).numpy()
        assert np.array_equal(col, want)
        assert len(np.unique(planes)) == planes.size and planes.min() > 0 and planes.max() < 2 ** 24


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_column_sum_cases_are_sensitive_to_every_row(mode):
    """removing or doubling any single row changes the reference's bits in at least one column of each sum the mode forms -- by brute force
    on small cases (the generator asserts the condition that implies it for every case of any size)"""
    rng = np.random.default_rng(mode)
    for R, C in ((2, 1), (63, 4), (65, 12), (129, 64), (70, 100)):
        case = T.colsum_case(rng, mode, R, C)
        rows = lambda k, idx: {key: (v[idx] if v.ndim == 2 else v) for key, v in case.items()}
        base = T.colsum(mode, **case)
        for r in range(R):
            keep = np.array([i for i in range(R) if i != r], dtype=np.int64)
            twice = np.concatenate([np.arange(R), [r]])
            for idx in (keep, twice):
                s = T.colsum(mode, **rows(None, idx))
                for w in range(1 if mode == 2 else 2):
                    assert (s[w] != base[w]).any(), (mode, R, C, r, w)


def test_finish_matches_its_definition():
    """the finisher against the textbook formulas in float64 (to fp32 rounding), and exactly at a power-of-two row count"""
    rng = np.random.default_rng(5)
    R, C = 64, 12
    case, fc = T.colsum_case(rng, 0, R, C), T.finish_case(rng, C)
    x = case["x"].astype(np.float64)
    mean, invstd, rm, rv = T.finish(T.colsum(0, **case), 1, R, **fc)
    assert np.array_equal(mean, x.mean(axis=0).astype(np.float32))
    assert np.allclose(invstd, 1 / np.sqrt(x.var(axis=0) + 1e-5), rtol=1e-6)
    m = fc["momentum"]
    assert np.array_equal(rm, ((1 - m) * fc["run_mean"] + m * (x.mean(axis=0) + fc["bias"])).astype(np.float32))
    assert np.allclose(rv, (1 - m) * fc["run_var"] + m * x.var(axis=0, ddof=1), rtol=1e-6)
    assert T.ulps32(np.float32([1.0]), np.nextafter(np.float32(1.0), np.float32(2.0)))[0] == 1


def test_colsum1v_sweep_reaches_every_loop_and_hand_over():
    """R = 128 + n, n = 1 .. 64, C in {4 .. 128}: which of the three row loops lane 0 and the last live lane of the LAST chunk run.  Over the
    sweep every pattern the arithmetic allows for a 64-row chunk occurs: one row alone, two in flight with and without a single row after,
    four in flight alone (twice at C = 128), followed by two, by one, by both."""
    pat = lambda t: "".join(k for k, n in zip("421", t) if n)
    lane0, last = set(), set()
    for C in (4, 8, 16, 32, 64, 128):
        RL = T.colsum1v_lanes(C)
        assert RL == {4: 256, 8: 128, 16: 64, 32: 32, 64: 16, 128: 8}[C]
        for n in range(1, 65):
            lane0.add(pat(T.colsum1v_loops(C, n, 0)))
            last.add(pat(T.colsum1v_loops(C, n, min(RL, n) - 1)))
            assert sum(k * v for k, v in zip((4, 2, 1), T.colsum1v_loops(C, n, 0))) == -(-n // RL)       # rows of lane 0
    assert T.colsum1v_loops(128, 64, 0) == (2, 0, 0) and T.colsum1v_loops(4, 64, 200) == (0, 0, 0)
    assert lane0 == {"1", "2", "21", "4", "41", "42", "421"}, lane0
    assert last >= {"1", "2", "21", "4", "41", "42", "421"}, last
