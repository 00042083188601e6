"""Plain numpy float64 references of the optimiser step's reductions and pointwise passes (csrc/train.hip), the generators of their
test cases and the launch arithmetic of the kernels restated.  No GPU, no library of the project: tests/test_train_passes_cpu.py holds
these references themselves (against torch autograd, and the sensitivity of the generated cases), tests/test_train_passes_gpu.py holds
the kernels against them.

Exactness by construction (the method of tests/exact_nets.py): inputs are small integers, means integers and halves, invstd / gamma /
momentum powers of two, running statistics small integers.  Every fp32 product of the kernels is then exact -- a contraction of
a * b + c into one fused operation cannot change a bit -- and the double partial sums are exact in any order, so the device is
compared with `==`.  Where a value is NOT exact by construction (a mean over a ragged row count) the reference applies the kernel's
own casts in the kernel's order, written down once in `finish`."""
import numpy as np

f32, f64 = np.float32, np.float64
TR_CHUNK = 64                                                        # rows of a first-stage workgroup (train.hip)
AZ_MAX_ACTIONS = 9                                                   # games with more actions take k_tr_loss_wide (include/azhip.h)
EPS32 = f32(1.1920929e-07)


# ------------------------------------------------------------------------------------------------ launch arithmetic, restated
def colsum_plan(mode, R, C, fin_inside=False):
    """tr_colsum: (chunks, vectorised MODE 1 form?, second stage inside the producer?, gridDim.y of the producer)"""
    vec = mode == 1 and C % 4 == 0 and C <= 128 and 256 % (C // 4) == 0
    return -(-R // TR_CHUNK), vec, bool(fin_inside and C <= 128), 1 if vec else -(-C // 64)


def colsum1v_lanes(C):
    """k_tr_colsum1v: row lanes of a workgroup, RL = 256 / (C / 4)"""
    return 256 // (C // 4)


def colsum1v_loops(C, rows, lane):
    """iterations of the three row loops of k_tr_colsum1v (four, two, one rows in flight) that row lane `lane` runs over a chunk of `rows` rows"""
    RL, r, n4, n2, n1 = colsum1v_lanes(C), lane, 0, 0, 0
    while r + 3 * RL < rows:
        n4, r = n4 + 1, r + 4 * RL
    while r + RL < rows:
        n2, r = n2 + 1, r + 2 * RL
    while r < rows:
        n1, r = n1 + 1, r + RL
    return n4, n2, n1


def finish_nsub(C, threads=256):
    """tr_finish: sub-sums per (sum, column) pair when 2 C pairs fit the workgroup, else 0 (a thread loops over pairs)"""
    return threads // (2 * C) if 2 * C <= threads else 0


def final_plan(nchunks):
    """k_tr_colsum_final: (iterations of thread 0's 64-stride loop, threads that hold a partial)"""
    return -(-nchunks // 64), min(nchunks, 64)


def loss_plan(B, A, force_wide=False):
    """tr_loss: (wide kernel?, workgroups, threads per workgroup)"""
    wide = force_wide or A > AZ_MAX_ACTIONS
    return (True, -(-B // 64), 64) if wide else (False, -(-B // 256), 256)


# ------------------------------------------------------------------------------------------------ column sums and finishers
def colsum(mode, x, out_act=None, g=None, mean=None, invstd=None):
    """sums[2][C] of k_tr_colsum<mode> / k_tr_colsum1v in float64, with the kernel's fp32 casts: mode 0 (x, x^2); mode 1 (dy, dy xhat),
    dy = x where out_act > 0 else 0, xhat = fp32(fp32(g - mean) * invstd); mode 2 (x, 0).  The products are taken in double."""
    x = np.asarray(x, dtype=f32)
    if mode == 0:
        v = x.astype(f64)
        return np.stack([v.sum(axis=0), (v * v).sum(axis=0)])
    if mode == 2:
        v = x.astype(f64)
        return np.stack([v.sum(axis=0), np.zeros(x.shape[1])])
    dy = np.where(np.asarray(out_act, dtype=f32) > 0, x, f32(0)).astype(f32)
    xh = ((np.asarray(g, dtype=f32) - np.asarray(mean, dtype=f32)).astype(f32) * np.asarray(invstd, dtype=f32)).astype(f32)
    return np.stack([dy.astype(f64).sum(axis=0), (dy.astype(f64) * xh.astype(f64)).sum(axis=0)])


def finish(sums, fin_mode, R, momentum=0.0, bias=None, run_mean=None, run_var=None):
    """what k_tr_colsum_final / tr_finish do with sums[2][C], operation by operation with the fp32 casts of the kernel:
    1: (mean, invstd, run_mean, run_var) -- Flux BatchNorm: biased variance, eps 1e-5, unbiased running variance;  2: (dbeta, dgamma, mf[2][C]);
    3: (out0,).  float32 arrays."""
    s0, s1 = np.asarray(sums[0], dtype=f64), np.asarray(sums[1], dtype=f64)
    if fin_mode == 1:
        mom = f32(momentum)
        m = s0 / f64(R)
        var = np.maximum(s1 / f64(R) - m * m, 0.0)
        mean = m.astype(f32)
        invstd = (1.0 / np.sqrt(var + 1e-5)).astype(f32)
        b = np.zeros_like(mean) if bias is None else np.asarray(bias, dtype=f32)
        one_m = f32(f32(1.0) - mom)
        rm = ((one_m * np.asarray(run_mean, dtype=f32)).astype(f32) + (mom * (mean + b).astype(f32)).astype(f32)).astype(f32)
        unb = (var * (f64(R) / f64(R - 1))).astype(f32)
        rv = ((one_m * np.asarray(run_var, dtype=f32)).astype(f32) + (mom * unb).astype(f32)).astype(f32)
        return mean, invstd, rm, rv
    if fin_mode == 2:
        return s0.astype(f32), s1.astype(f32), np.stack([(s0 / f64(R)).astype(f32), (s1 / f64(R)).astype(f32)])
    if fin_mode == 3:
        return (s0.astype(f32),)
    return ()


def ulps32(a, b):
    """distance of two float32 arrays in units of the last place (same sign assumed, finite)"""
    a, b = np.asarray(a, dtype=f32), np.asarray(b, dtype=f32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def _signed(rng, shape, hi=3):
    """integers of {-hi .. -1, 1 .. hi} as fp32: no entry is zero"""
    return (rng.integers(1, hi + 1, size=shape) * rng.choice([-1, 1], size=shape)).astype(f32)


def row_contributions(mode, case):
    """[2][R][C] float64: what each row adds to each of the two sums"""
    x = case["x"].astype(f64)
    if mode == 0:
        return np.stack([x, x * x])
    if mode == 2:
        return np.stack([x, np.zeros_like(x)])
    dy = np.where(case["out_act"] > 0, x, 0.0)
    xh = (case["g"].astype(f64) - case["mean"].astype(f64)) * case["invstd"].astype(f64)
    return np.stack([dy, dy * xh])


def colsum_case(rng, mode, R, C):
    """inputs of one column-sum case.  x from {-3 .. -1, 1 .. 3}; mode 1: a 0/1 activation, integer g, mean of integers and halves,
    invstd a power of two, and in every row at least one column that is unmasked with g != mean.  ASSERTED here, so that no case can hide
    what it is for: every row adds something non-zero to at least one column of each sum the mode forms (mode 2 forms one), and every
    sum stays far below 2^53 in units of its grid (1 or 1/4) -- so removing or doubling any single row changes the reference's bits."""
    case = {"x": _signed(rng, (R, C))}
    if mode == 1:
        case["out_act"] = rng.integers(0, 2, size=(R, C)).astype(f32) * f32(2.5)
        case["g"] = rng.integers(-3, 4, size=(R, C)).astype(f32)
        case["mean"] = (rng.integers(-2, 3, size=C) * 0.5).astype(f32)
        case["invstd"] = rng.choice([0.5, 1.0, 2.0], size=C).astype(f32)
        live = (case["out_act"] > 0) & (case["g"] != case["mean"])
        for r in np.flatnonzero(~live.any(axis=1)):                  # give such a row one live column
            c = int(rng.integers(0, C))
            case["out_act"][r, c] = f32(2.5)
            case["g"][r, c] = case["mean"][c] + f32(1.5)
    contrib = row_contributions(mode, case)
    for w in range(1 if mode == 2 else 2):
        assert (contrib[w] != 0).any(axis=1).all(), "a row adds nothing to sum %d" % w
    assert np.abs(contrib).sum(axis=1).max() * 4 < 2 ** 50
    assert np.array_equal(contrib * 4, np.round(contrib * 4))        # quarters at the finest: exact in any order
    return case


def finish_case(rng, C):
    """inputs of the batch-statistics finisher: momentum a power of two (1 - momentum a short dyadic), integer bias and running statistics"""
    return dict(momentum=float(rng.choice([0.25, 0.5, 0.125])), bias=rng.integers(-2, 3, size=C).astype(f32),
                run_mean=rng.integers(-3, 4, size=C).astype(f32), run_var=rng.integers(1, 5, size=C).astype(f32))


# ------------------------------------------------------------------------------------------------ batch norm, dense epilogues
def bn_apply(g, mean, invstd, gamma, beta, res=None):
    """a = relu(gamma ((g - mean) invstd) + beta (+ res)), float64"""
    v = f64(1) * gamma * ((np.asarray(g, dtype=f64) - mean) * invstd) + beta
    if res is not None:
        v = v + res
    return np.maximum(v, 0.0)


def bn_bwd(da, a, g, mean, invstd, gamma, mf):
    """k_tr_bn_bwd in float64: dy = da (a > 0); dg = gamma invstd (dy - mf[0] - xhat mf[1]); returns (dg, dy)"""
    dy = np.where(np.asarray(a) > 0, np.asarray(da, dtype=f64), 0.0)
    xh = (np.asarray(g, dtype=f64) - mean) * invstd
    return f64(1) * gamma * invstd * (dy - mf[0] - xh * mf[1]), dy


def bn_layer_bwd(da, g, gamma, beta, res=None, eps=1e-5):
    """the whole backward pass of a = relu(bn(g) (+ res)) with batch statistics, float64, as the step composes it: column sums of mode 1,
    finisher 2, k_tr_bn_bwd.  Returns (dg, dgamma, dbeta, dy): dy is also the gradient with respect to res."""
    g = np.asarray(g, dtype=f64)
    R = g.shape[0]
    mean = g.mean(axis=0)
    invstd = 1.0 / np.sqrt(g.var(axis=0) + eps)
    a = bn_apply(g, mean, invstd, gamma, beta, res)
    dy = np.where(a > 0, np.asarray(da, dtype=f64), 0.0)
    xh = (g - mean) * invstd
    s0, s1 = dy.sum(axis=0), (dy * xh).sum(axis=0)
    dg, _ = bn_bwd(da, a, g, mean, invstd, gamma, np.stack([s0 / R, s1 / R]))
    return dg, s1, s0, dy


def bias_act(x, bias, relu):
    v = np.asarray(x, dtype=f64) + bias
    return np.maximum(v, 0.0) if relu else v


def relu_bwd(dy, y):
    return np.where(np.asarray(y) > 0, np.asarray(dy, dtype=f64), 0.0)


def bn_case(rng, rows, C):
    """exact inputs of the pointwise passes: integer g / da / res in [-3, 3], an activation with zeros, negatives and positives, mean of
    integers and halves, invstd and gamma (signed) powers of two, integer beta and bias, mf of halves"""
    ints = lambda: rng.integers(-3, 4, size=(rows, C)).astype(f32)
    return dict(g=ints(), da=ints(), res=ints(), a=rng.integers(-1, 3, size=(rows, C)).astype(f32),
                mean=(rng.integers(-2, 3, size=C) * 0.5).astype(f32), invstd=rng.choice([0.5, 1.0, 2.0], size=C).astype(f32),
                gamma=(rng.choice([0.5, 1.0, 2.0], size=C) * rng.choice([-1, 1], size=C)).astype(f32), beta=rng.integers(-2, 3, size=C).astype(f32),
                mf=(rng.integers(-4, 5, size=(2, C)) * 0.5).astype(f32), bias=rng.integers(-2, 3, size=C).astype(f32))


# ------------------------------------------------------------------------------------------------ im2col
def plane_codes(B, C, H, W):
    """planes[B][C][H][W] whose value is a unique positive integer code of (board, plane, y, x): a read across a board or row edge is a wrong
    code where a zero belongs"""
    return (1 + np.arange(B * C * H * W)).reshape(B, C, H, W).astype(f32)


def im2col(planes):
    """col[B H W][9 C], column = tap C + c, tap = 3 (dy + 1) + (dx + 1): the 3x3 neighbourhood of each position, zero off the board.
    A direct triple loop over (row, tap, channel)."""
    B, C, H, W = planes.shape
    col = np.zeros((B * H * W, 9 * C), dtype=f64)
    for r in range(B * H * W):
        b, y, x = r // (H * W), (r % (H * W)) // W, r % W
        for tap in range(9):
            yy, xx = y + tap // 3 - 1, x + tap % 3 - 1
            if 0 <= yy < H and 0 <= xx < W:
                for c in range(C):
                    col[r, tap * C + c] = planes[b, c, yy, xx]
    return col


# ------------------------------------------------------------------------------------------------ loss
def loss64(logits, tpre, Am, P, V, W, cinv, rho, gscale):
    """`losses` (learning.jl:67-90) per sample in float64 with its analytic gradient:
      p = softmax(logits), u = p Am, S = sum u, q = u / (S + eps)
      kl_i = sum_a P_a log(q_a + eps) w, inv_i = (1 - S) w, mse_i = ((tanh t - V) / rho)^2 w
      dlogits, dt = gradient of gscale sum_i (-kl_i + mse_i + cinv inv_i)
    returns dlogits[B][A], dt[B], terms[4][B] = w, kl, mse, inv"""
    lg, Am, P = (np.asarray(z, dtype=f64) for z in (logits, Am, P))
    t, V, w = (np.asarray(z, dtype=f64) for z in (tpre, V, W))
    eps = f64(EPS32)
    e = np.exp(lg - lg.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True)
    u = p * Am
    S = u.sum(axis=1, keepdims=True)
    den = S + eps
    q = u / den
    kl = (P * np.log(q + eps)).sum(axis=1) * w
    gq = -P / (q + eps)                                              # d(-sum P log(q + eps)) / dq
    gu = gq / den - (gq * u).sum(axis=1, keepdims=True) / (den * den)   # ... / du: q_a = u_a / (sum u + eps)
    dp = Am * (gu - cinv) * w[:, None] * gscale                      # u = p Am; the invalid-mass penalty: d(1 - S)/du = -1
    dlogits = p * (dp - (p * dp).sum(axis=1, keepdims=True))         # softmax backward
    vh = np.tanh(t)
    d = vh / rho - V / rho
    dt = 2.0 * d / rho * (1.0 - vh * vh) * w * gscale
    return dlogits, dt, np.stack([w, kl, d * d * w, (1.0 - S[:, 0]) * w])


def loss32(logits, tpre, Am, P, V, W, cinv, rho, gscale, expf, logf, tanhf):
    """k_tr_loss restated operation by operation in Float32 (one rounding per operation, no contraction; sums over the actions in action
    order), with the oracle's expf / logf / tanhf (vectorised over an array: callables float32 array -> float32 array).  Vectorised
    over the samples, sequential over the actions as the kernel's loops are.  Same outputs as loss64; kl is accumulated in double."""
    lg, Am, P = (np.asarray(z, dtype=f32) for z in (logits, Am, P))
    t, V, w = (np.asarray(z, dtype=f32) for z in (tpre, V, W))
    cinv, rho, gscale, eps = f32(cinv), f32(rho), f32(gscale), EPS32
    B, A = lg.shape
    mx = lg.max(axis=1)
    p = np.stack([expf((lg[:, a] - mx).astype(f32)) for a in range(A)], axis=1)
    se = np.zeros(B, dtype=f32)
    for a in range(A):
        se = (se + p[:, a]).astype(f32)
    p = (p / se[:, None]).astype(f32)
    u = (p * Am).astype(f32)
    S = np.zeros(B, dtype=f32)
    for a in range(A):
        S = (S + u[:, a]).astype(f32)
    den = (S + eps).astype(f32)
    kl = np.zeros(B, dtype=f64)
    gu_sum = np.zeros(B, dtype=f32)
    gq = np.zeros((B, A), dtype=f32)
    for a in range(A):
        q = (u[:, a] / den).astype(f32)
        qe = (q + eps).astype(f32)
        kl += ((P[:, a] * logf(qe)).astype(f32) * w).astype(f32).astype(f64)
        gq[:, a] = ((-P[:, a]) / qe).astype(f32)
        gu_sum = (gu_sum + (gq[:, a] * u[:, a]).astype(f32)).astype(f32)
    gu_sum = (gu_sum / (den * den).astype(f32)).astype(f32)
    dp = np.zeros((B, A), dtype=f32)
    dot = np.zeros(B, dtype=f32)
    for a in range(A):
        inner = (((gq[:, a] / den).astype(f32) - gu_sum).astype(f32) - cinv).astype(f32)
        dp[:, a] = (((Am[:, a] * inner).astype(f32) * w).astype(f32) * gscale).astype(f32)
        dot = (dot + (p[:, a] * dp[:, a]).astype(f32)).astype(f32)
    dlogits = (p * (dp - dot[:, None]).astype(f32)).astype(f32)
    vh = tanhf(t)
    d = ((vh / rho).astype(f32) - (V / rho).astype(f32)).astype(f32)
    one_m = (f32(1) - (vh * vh).astype(f32)).astype(f32)
    dt = (((((f32(2) * d).astype(f32) / rho).astype(f32) * one_m).astype(f32) * w).astype(f32) * gscale).astype(f32)
    mse = ((d * d).astype(f32) * w).astype(f32)
    inv = ((f32(1) - S).astype(f32) * w).astype(f32)
    return dlogits, dt, np.stack([w.astype(f64), kl, mse.astype(f64), inv.astype(f64)])


def oracle_math():
    """(expf, logf, tanhf) of the CPU oracle (oracle/azref.c: the functions the device's az_expf / az_logf / az_tanhf are held bit-identical
    to), each vectorised over a float32 array"""
    import ctypes as C
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
    import azref as R
    out = []
    for name in ("azr_expf", "azr_logf", "azr_tanhf"):
        fn = getattr(R.lib(), name)
        fn.restype, fn.argtypes = C.c_float, [C.c_float]
        out.append(lambda a, fn=fn: np.array([fn(float(v)) for v in np.asarray(a, dtype=f32).ravel()], dtype=f32).reshape(np.shape(a)))
    return tuple(out)


LOSS_GAMES = {0: 7, 1: 9, 2: 6, 3: 82}                               # game id -> actions
LOSS_NARROW_B = (2, 255, 256, 257)                                   # k_tr_loss: 256 threads per workgroup
LOSS_WIDE_B = (2, 63, 64, 65, 130)                                   # k_tr_loss_wide: 64 threads per workgroup
LOSS_CASES = [(g, b) for g in (0, 1, 2) for b in LOSS_NARROW_B] + [(3, b) for b in LOSS_WIDE_B]
LOSS_CONSTS = dict(cinv=1.0, rho=2.0)                                # nonvalidity_penalty, rewards_renormalization
MIN_LEGAL_MASS = 1e-3


def loss_case(game, B, degenerate=False):
    """inputs of one loss case, the same for every caller (seeded by game and batch): logits spread over +-8, 0/1 masks with at least one
    legal action, targets on the legal actions; rows with a single legal action (i % 5 == 1), target zeros (i % 7 == 2), w = 0 (i % 4 == 3),
    V = +-1 with |tpre| up to 6 (i % 3 == 0).  The legal mass S stays >= 1e-3 (asserted) -- unless `degenerate`: then row 0 has S ~ 0."""
    A = LOSS_GAMES[game]
    rng = np.random.default_rng(1000 * game + B + (500000 if degenerate else 0))
    lg = rng.uniform(-8, 8, size=(B, A))
    Am = (rng.random((B, A)) < 0.7).astype(f64)
    P = rng.random((B, A))
    t = rng.uniform(-2, 2, size=B)
    V = rng.uniform(-1, 1, size=B)
    w = rng.uniform(0.2, 3.0, size=B)
    for i in range(B):
        if i % 5 == 1:
            Am[i] = 0
        if not Am[i].any():
            Am[i, rng.integers(0, A)] = 1
        if i % 7 == 2:
            P[i, rng.random(A) < 0.5] = 0
        if i % 4 == 3:
            w[i] = 0
        if i % 3 == 0:
            V[i] = rng.choice([-1.0, 1.0])
            t[i] = rng.uniform(3, 6) * rng.choice([-1.0, 1.0])
        P[i] *= Am[i]
        if P[i].sum() == 0:
            P[i, np.flatnonzero(Am[i])[0]] = 1
        P[i] /= P[i].sum()
        e = np.exp(lg[i] - lg[i].max())
        if (e * Am[i]).sum() / e.sum() < 4 * MIN_LEGAL_MASS:          # lift the best legal action to the top of the row
            lg[i, np.flatnonzero(Am[i])[0]] = lg[i].max()
    if degenerate:
        lg[0], Am[0], P[0] = 40.0, 0.0, 0.0
        lg[0, 0], Am[0, 0], P[0, 0], w[0] = -40.0, 1.0, 1.0, 1.0
    out = dict(logits=lg.astype(f32), tpre=t.astype(f32), Am=Am.astype(f32), P=P.astype(f32), V=V.astype(f32), W=w.astype(f32),
               gscale=float(f32(1.0) / (f32(B) * f32(1.3))), **LOSS_CONSTS)
    e = np.exp(out["logits"].astype(f64) - out["logits"].astype(f64).max(axis=1, keepdims=True))
    S = (e * Am).sum(axis=1) / e.sum(axis=1)
    assert degenerate or S.min() >= MIN_LEGAL_MASS, S.min()
    assert not degenerate or S[0] < 1e-30
    return out


LOSS_KINDS = ("dlogits", "dt", "w", "kl", "mse", "inv")


def loss_deviation(got, want):
    """the six figures the loss is held by: dlogits relative to each row's largest reference entry, dt and the four terms relative to the
    value with a floor of 1e-6.  got / want = (dlogits, dt, terms[4][B])"""
    dl, dt, tm = (np.asarray(z, dtype=f64) for z in got)
    rl, rt, rm = (np.asarray(z, dtype=f64) for z in want)
    rel = lambda a, b: float((np.abs(a - b) / np.maximum(np.abs(b), 1e-6)).max())
    rowmax = np.maximum(np.abs(rl).max(axis=1, keepdims=True), 1e-300)
    return np.array([float((np.abs(dl - rl) / rowmax).max()), rel(dt, rt)] + [rel(tm[k], rm[k]) for k in range(4)])


def loss_reference_error():
    """e: the largest deviation of the Float32 restatement from the float64 reference over LOSS_CASES, per figure of LOSS_KINDS.  The device
    gets 4 e: contraction changes how single operations round, not how many there are."""
    fns = oracle_math()
    e = np.zeros(6)
    for game, B in LOSS_CASES:
        c = loss_case(game, B)
        e = np.maximum(e, loss_deviation(loss32(*_loss_args(c), *fns), loss64(*_loss_args(c))))
    return e


def _loss_args(c):
    return c["logits"], c["tpre"], c["Am"], c["P"], c["V"], c["W"], c["cinv"], c["rho"], c["gscale"]
