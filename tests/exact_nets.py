"""Test helpers for the bfloat16 tower (csrc/resnet16b.h): its float64 emulation, and networks whose bf16 arithmetic is EXACT.

The emulation (torch_forward_bf16) restates the kernel's scheme: the F -> F convolution weights and every activation the tower
stores are rounded to bf16, everything else is wide.  With random dense weights a 10-block chain drifts up to 1.5e-2 from it
(rounding-boundary flips, the MFMA's internal summation order), which hides a wrong tap or a mis-packed fragment.

exact_net() therefore builds networks in which nothing rounds: ternary convolution weights, batch norm folded to scale 1 and an
integer shift, integer input planes.  Every stored activation is then a small integer (<= 255: exact in bf16), every partial
sum an integer far below 2^24, so summation order and rounding mode cannot matter and a correct kernel's tower output EQUALS
the emulation's.  Only the fp32 heads round, and those are held to 1e-5 elsewhere (TOL of tests/test_net.py).  The shifts are
calibrated on the batch the builder draws, so the construction is data-dependent by design: a test sends that batch (or a
prefix of it -- boards are evaluated independently, so every condition on single activations carries over to a prefix).

Layers are numbered 0 = stem, 2 b + 1 / 2 b + 2 = first / second convolution of block b; acts[k] is what layer k stores."""
import functools

import numpy as np
import torch

import azref as R
from azhip.network import ResNetHP, random_params, split_params
from test_net import batch_of, random_positions


def bf16(x):
    """round to nearest even: the kernel's v_cvt_pk_bf16_f32"""
    return x.to(torch.bfloat16).to(torch.float64)


def _on_f32_bits(x, f):
    return f(x.to(torch.float32).view(torch.int32)).view(torch.float32).to(torch.float64)


def bf16_trunc(x):
    """WRONG on purpose (rounding-leg mutation): drop the low 16 bits of the fp32 value"""
    return _on_f32_bits(x, lambda i: i & -65536)


def bf16_half_away(x):
    """WRONG on purpose (rounding-leg mutation): round half away from zero"""
    return _on_f32_bits(x, lambda i: (i + 0x8000) & -65536)


def _layer_names(hp):
    out = [("stem.conv", "stem.bn")]
    for b in range(hp.num_blocks):
        out += [("block%d.conv1" % b, "block%d.bn1" % b), ("block%d.conv2" % b, "block%d.bn2" % b)]
    return out


def _torch_w(W):
    """Flux W[i, j, ci, co] of a true convolution -> conv2d's (co, ci, ky, kx)"""
    return W.flip(0, 1).permute(3, 2, 1, 0).contiguous()


def _flux_w(w):
    """inverse of _torch_w"""
    return w.flip(2, 3).permute(3, 2, 1, 0).contiguous()


def _fold(p, conv, bnp):
    """scale and shift as bn_fold of az_net_set_params computes them (fp32)"""
    g, be, mu, var = (p[bnp + "." + k].to(torch.float32) for k in ("gamma", "beta", "mean", "var"))
    scale = g / torch.sqrt(var + torch.tensor(1e-5, dtype=torch.float32))
    shift = (p[conv + ".b"].to(torch.float32) - mu) * scale + be
    s = (1, -1, 1, 1)
    return scale.to(torch.float64).view(s), shift.to(torch.float64).view(s)


def _drop_tap(z, xin, w, ky, kx, y, x):
    """the convolution output at cell (y, x) without tap (ky, kx): what a tap skipped for that cell's border class leaves"""
    sy, sx = y + ky - 1, x + kx - 1
    assert 0 <= sy < xin.shape[2] and 0 <= sx < xin.shape[3], "the dropped tap must be on the board"
    z = z.clone()
    z[:, :, y, x] -= xin[:, :, sy, sx] @ w[:, :, ky, kx].T
    return z


def tower_bf16(p, hp, X, rnd=bf16, skip_unrounded=False, mutate=None, base=None):
    """The tower of the bf16 scheme in float64.  Returns (acts, raw): per layer the stored (rounded) activation and the value
    before rounding.  `mutate` injects ONE error, to measure what a comparison with this emulation can see:
      ("tap", layer, ky, kx, y, x)   layer drops tap (ky, kx) at board cell (y, x), all boards and channels
      ("skip", block)                 the skip connection of `block` adds the block input shifted by one board cell
      ("chan", layer, co, ci, kx)     the weight (co, ci, middle row, kx) of `layer` sits at the neighbouring input channel ci ^ 1
    `base` = the acts of the unmutated run: layers before the mutated one are taken from it instead of recomputed."""
    names = _layer_names(hp)
    kind = mutate[0] if mutate else None
    mlayer = None if not mutate else 2 * mutate[1] + 2 if kind == "skip" else mutate[1]
    first = mlayer if (base is not None and mlayer is not None) else 0
    acts, raw = ([None] * len(names), [None] * len(names))
    if first > 0:
        acts[:first] = base[:first]
    unrounded_in = None
    for k in range(first, len(names)):
        conv, bnp = names[k]
        xin = torch.as_tensor(X, dtype=torch.float64) if k == 0 else acts[k - 1]
        w = _torch_w(p[conv + ".W"])
        if k > 0:
            w = bf16(w)                                              # the stem stays fp32, its output is stored in bf16
        if kind == "chan" and k == mlayer:
            co, ci, kx = mutate[2:]                                 # middle kernel row: on the board in every geometry
            w = w.clone()
            w[co, ci ^ 1, 1, kx], w[co, ci, 1, kx] = w[co, ci, 1, kx] + w[co, ci ^ 1, 1, kx], 0.0
        z = torch.nn.functional.conv2d(xin, w, None, padding=1)
        if kind == "tap" and k == mlayer:
            z = _drop_tap(z, xin, w, *mutate[2:])
        scale, shift = _fold(p, conv, bnp)
        y = z * scale + shift
        if k > 0 and k % 2 == 0:                                     # second convolution of a block: + the block input AS STORED
            skip = unrounded_in if (skip_unrounded and unrounded_in is not None) else acts[k - 2]
            if kind == "skip" and k == mlayer:
                skip = torch.roll(skip.flatten(2), 1, dims=2).view_as(skip)
            y = y + skip
        raw[k] = torch.relu(y)
        acts[k] = rnd(raw[k])
        if k % 2 == 0:
            unrounded_in = raw[k]
    return acts, raw


def heads_bf16(p, x, A):
    """1x1 head convolutions on bf16 weights, features in fp32, dense heads wide; masked and renormalised policy"""
    N = x.shape[0]

    def feat(h):
        z = torch.nn.functional.conv2d(x, bf16(_torch_w(p[h + ".conv.W"])), None, padding=0)
        scale, shift = _fold(p, h + ".conv", h + ".bn")
        return torch.relu(z * scale + shift).to(torch.float32).to(torch.float64).reshape(N, -1)

    logits = feat("phead") @ p["phead.dense.W"].T + p["phead.dense.b"]
    pol = torch.softmax(logits, dim=1)
    v1 = torch.relu(feat("vhead") @ p["vhead.dense1.W"].T + p["vhead.dense1.b"])
    val = torch.tanh(v1 @ p["vhead.dense2.W"].T + p["vhead.dense2.b"]).reshape(N)
    pm = pol * torch.as_tensor(A, dtype=torch.float64)
    sp = pm.sum(dim=1, keepdim=True)
    return (pm / (sp + float(np.finfo(np.float32).eps))).numpy(), val.numpy()


def params64(game, hp, blob):
    return {k: torch.tensor(np.ascontiguousarray(v), dtype=torch.float64) for k, v in split_params(game, hp, blob).items()}


def tower_stats(acts, raw, rnd=bf16):
    """per stored activation tensor: (elements that rounding changed, largest magnitude, share of non-zero elements)"""
    return [(int((rnd(r) != r).sum()), float(r.abs().max()), float((a != 0).double().mean())) for a, r in zip(acts, raw)]


def torch_forward_bf16(game, hp, blob, X, A, stats=None, **kw):
    """P, V of the bf16 scheme (any board geometry: the shapes come from X and the parameter layout).  `stats`: a list that
    receives tower_stats(); keywords as tower_bf16."""
    p = params64(game, hp, blob)
    acts, raw = tower_bf16(p, hp, X, **kw)
    if stats is not None:
        stats.extend(tower_stats(acts, raw))
    return heads_bf16(p, acts[-1], A)


# ------------------------------------------------------------------------------------------------ exact networks
BN_VAR_ONE = np.float32(1) - np.float32(1e-5)      # var + 1e-5f == 1.0f in fp32: bn_fold gives scale exactly 1


def distinct_positions(game, n, seed):
    """n random positions with pairwise different input planes (Mancala shows the initial board whenever black is to move)"""
    envs, seen, k = [], set(), 0
    while len(envs) < n:
        for g in random_positions(game, 2 * n, seed + 1000 * k):
            t = g.vectorize().tobytes()
            if t not in seen and len(envs) < n:
                seen.add(t)
                envs.append(g)
        k += 1
    return envs


def _ternary(rng, F, cin, nnz, rows=None, taps=range(9)):
    """(F, cin, 3, 3) with +-1 entries.  nnz = None: every entry.  Otherwise the output channels `rows` (default: all) get nnz
    entries each at a random tap of `taps`, wired so that every input channel is read equally often (a channel that nobody reads
    would hide whatever went wrong in it)"""
    if nnz is None:
        return torch.tensor(rng.integers(0, 2, size=(F, cin, 3, 3)) * 2.0 - 1.0)
    rows = np.arange(F) if rows is None else rows
    w = np.zeros((F, cin, 9))
    for j in range(nnz):
        ci = np.concatenate([rng.permutation(cin) for _ in range(len(rows) // cin + 1)])[:len(rows)]
        w[rows, ci, np.asarray(taps)[(rng.integers(0, len(taps), size=len(rows)) + j) % len(taps)]] = rng.integers(0, 2, size=len(rows)) * 2.0 - 1.0
    return torch.tensor(w.reshape(F, cin, 3, 3))


def _positions(game, n, seed):
    """(X, A, keys): real positions for the device games (so that az_net_evaluate_keys can be compared too), random planes
    for Go 9x9 (keys = None: it has no device twin)"""
    if game == R.GO9:
        from test_go9_net_gpu import random_go_batch
        return random_go_batch(n, seed) + (None,)
    envs = distinct_positions(game, n, seed)
    return batch_of(game, envs) + (np.array([g.key() for g in envs], dtype=np.uint64),)


def _set_layer(pv, conv, bnp, w, beta):
    """convolution bias 0, batch norm = identity + beta: scale exactly 1, shift exactly beta after bn_fold"""
    pv[conv + ".W"][...] = _flux_w(w).numpy()
    pv[conv + ".b"][...] = 0.0
    pv[bnp + ".gamma"][...] = 1.0
    pv[bnp + ".beta"][...] = beta.numpy()
    pv[bnp + ".mean"][...] = 0.0
    pv[bnp + ".var"][...] = BN_VAR_ONE


def _finish_heads(game, hp, blob, pv, x, A):
    """1x1 head convolution weights rounded to bf16 (the blob is what the kernel uses); both head batch norms get the largest
    gamma = 2^-e at which neither head saturates on tower output x; the rest stays as random_params drew it"""
    for h in ("phead", "vhead"):
        pv[h + ".conv.W"][...] = bf16(torch.tensor(np.ascontiguousarray(pv[h + ".conv.W"]), dtype=torch.float64)).numpy()
    for e in range(24):
        pv["phead.bn.gamma"][...] = 2.0 ** -e
        pv["vhead.bn.gamma"][...] = 2.0 ** -e
        P, V = heads_bf16(params64(game, hp, blob), x, A)
        if np.median(P.max(1)) < 0.4 and np.abs(V).max() < 0.8:
            return
    raise AssertionError("heads saturate at every gamma tried")


def exact_net(game, hp, n=64, seed=0, nnz=2, nnz1=4, cancel=0.5, q=0.5, dense=None, q_dense_in=0.7):
    """(blob, X, A, keys) of an exact network for `game`, calibrated on the n boards it returns.

    Tower: ternary weights, nnz per output channel (nnz1 in a block's first convolution, on the channels that do not pass
    through) at random taps, every input channel read equally often (see _ternary: with purely random wiring a seventh of the
    channels has no reader, and an error that lands there cannot show); batch norm gamma 1, mean 0, var BN_VAR_ONE,
    convolution bias 0, beta = minus an integer threshold near the q-quantile of the channel's pre-activation over this batch
    (found layer by layer in float64), so that a share of about 1 - q of the units is active at every depth.
    For a share `cancel` of a block's channels the first convolution passes the block input through (centre tap of the own
    channel, beta 0: the input is >= 0) and the second carries -1 there: the skip connection that the kernel adds must cancel
    exactly and the channel starts afresh.  On the other channels the skip accumulates; with all of them accumulating the
    values grow by a factor per block and leave bf16's 8 bits before depth 10.
    `dense` = k: layer k (1 .. 2 * blocks) is fully dense ternary -- a non-zero in EVERY (input channel, tap, output channel)
    entry of its weight fragments, which the sparse layers sample only thinly.  The layer before it (unless that is the stem,
    whose 0 / 1 / 2 outputs are small anyway) is calibrated at q_dense_in so that the dense sums stay small; no channel of
    the dense layer's block passes through.
    Heads: see _finish_heads."""
    rng = np.random.Generator(np.random.Philox(seed))
    blob = random_params(game, hp, seed=4000 + seed)
    pv = split_params(game, hp, blob)                               # views into blob
    X, A, keys = _positions(game, n, 100 + seed)
    F, names = hp.num_filters, _layer_names(hp)
    x = torch.tensor(X, dtype=torch.float64)
    block_in, through = None, None
    taps = range(9) if X.shape[2] > 1 else range(3, 6)              # a board of one row: only the middle kernel row is ever on it
    for k, (conv, bnp) in enumerate(names):
        if k % 2 == 1:
            dense_block = dense in (k, k + 1)
            through = np.sort(rng.choice(F, size=0 if dense_block else int(round(cancel * F)), replace=False))
            w = _ternary(rng, F, F, None if k == dense else nnz1, np.setdiff1d(np.arange(F), through), taps)
            w[through, through, 1, 1] = 1.0
        else:
            w = _ternary(rng, F, x.shape[1], None if k == dense else nnz, None, taps)
            if k > 0:
                w[through, through, 1, 1] = -1.0
        z = torch.nn.functional.conv2d(x, w, None, padding=1)
        if k > 0 and k % 2 == 0:
            z = z + block_in
        qk = q_dense_in if (dense is not None and k == dense - 1 and k > 0) else q
        zc = z.transpose(0, 1).flatten(1)
        v = torch.quantile(zc, qk, dim=1, interpolation="lower")    # z is integer: of the thresholds v - 1 and v, the one whose
        near = [((zc > (v - d).view(-1, 1)).double().mean(1) - (1 - qk)).abs() for d in (1, 0)]   # active share is nearer 1 - q
        beta = -torch.where(near[0] <= near[1], v - 1, v)
        if k % 2 == 1:
            beta[through] = 0.0
        x = torch.relu(z + beta.view(1, -1, 1, 1))
        if k % 2 == 0:
            block_in = x
        _set_layer(pv, conv, bnp, w, beta)
    _finish_heads(game, hp, blob, pv, x, A)
    return blob, X, A, keys


def make_hp(nblocks, F):
    return ResNetHP(num_blocks=nblocks, num_filters=F, num_policy_head_filters=32, num_value_head_filters=32)


_SHALLOW = dict(nnz=3, nnz1=6)                     # up to 5 blocks the values stay small with denser wiring
# name -> (game, blocks, filters, exact_net keywords).  Every network is built on 64 boards; the GPU tests send prefixes.
CONFIGS = {"c4-10x128-s0": (R.C4, 10, 128, dict(seed=0)), "c4-10x128-s1": (R.C4, 10, 128, dict(seed=1)),
           "c4-5x64-s0": (R.C4, 5, 64, dict(seed=0, **_SHALLOW)), "c4-5x64-s1": (R.C4, 5, 64, dict(seed=1, **_SHALLOW)),
           "ttt-3x64": (R.TTT, 3, 64, dict(seed=0, **_SHALLOW)), "ttt-3x128": (R.TTT, 3, 128, dict(seed=0, **_SHALLOW)),
           "mancala-3x64": (R.MANCALA, 3, 64, dict(seed=0, **_SHALLOW)), "mancala-3x128": (R.MANCALA, 3, 128, dict(seed=0, **_SHALLOW)),
           "go9-10x128-s0": (R.GO9, 10, 128, dict(seed=0)), "go9-10x128-s1": (R.GO9, 10, 128, dict(seed=1))}
for _F in (64, 128):
    for _d in range(1, 7):
        CONFIGS["c4-3x%d-dense%d" % (_F, _d)] = (R.C4, 3, _F, dict(seed=0, dense=_d, nnz1=2))
NBOARDS = 64


@functools.lru_cache(maxsize=None)
def build(name):
    """(game, hp, blob, X, A, keys) of CONFIGS[name]"""
    game, nblocks, F, kw = CONFIGS[name]
    hp = make_hp(nblocks, F)
    return (game, hp) + exact_net(game, hp, NBOARDS, **kw)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(P, V, acts, stats) of the emulation on CONFIGS[name]'s 64 boards"""
    game, hp, blob, X, A, _ = build(name)
    p = params64(game, hp, blob)
    acts, raw = tower_bf16(p, hp, X)
    return heads_bf16(p, acts[-1], A) + (acts, tower_stats(acts, raw))


# ------------------------------------------------------------------------------------------------ the rounding leg
# Exact networks cannot see HOW the kernel rounds.  This one can: one block, Connect-Four.  The stem (fp32 weights, never
# rounded) multiplies a 0 / 1 plane by a value bf16 cannot hold, so its output must be rounded when it is stored:
#   257, 259, 1 + 2^-8   ties: nearest-even 256, 260, 1;  truncation 256, 258, 1;  half away from zero 258, 260, 1 + 2^-7
#   257.5                 no tie: nearest 258, truncation 256
#   -300                  ReLU gives 0 whatever the rounding
# conv1 is the identity; conv2 has -1 (even channels) or +1 (odd channels) on the centre tap of its own channel.  With -1 the
# block output is skip - stored: 0 if the skip adds what was stored, 1 (= 257 - 256) if it adds the unrounded value; with +1 it
# is twice the stored value, which shows the rounding mode itself.
ROUNDING_VALUES = (257.0, 259.0, 257.5, 1.0 + 2.0 ** -8, -300.0, 3.0)


@functools.lru_cache(maxsize=None)
def rounding_net(F=64, n=16, seed=7):
    """(game, hp, blob, X, A, keys)"""
    game, hp = R.C4, make_hp(1, F)
    blob = random_params(game, hp, seed=4100 + seed)
    pv = split_params(game, hp, blob)
    X, A, keys = _positions(game, n, 200 + seed)
    C = X.shape[1]
    ch = np.arange(F)
    stem, ident, sign = torch.zeros(F, C, 3, 3, dtype=torch.float64), torch.zeros(F, F, 3, 3, dtype=torch.float64), torch.zeros(F, F, 3, 3, dtype=torch.float64)
    stem[ch, ch % C, 1, 1] = torch.tensor([ROUNDING_VALUES[(c // C) % len(ROUNDING_VALUES)] for c in ch], dtype=torch.float64)
    ident[ch, ch, 1, 1] = 1.0
    sign[ch, ch, 1, 1] = torch.tensor(np.where(ch % 2 == 0, -1.0, 1.0))
    zero = torch.zeros(F, dtype=torch.float64)
    for (conv, bnp), w in zip(_layer_names(hp), (stem, ident, sign)):
        _set_layer(pv, conv, bnp, w, zero)
    acts, _ = tower_bf16(params64(game, hp, blob), hp, X)
    _finish_heads(game, hp, blob, pv, acts[-1], A)
    return game, hp, blob, X, A, keys
