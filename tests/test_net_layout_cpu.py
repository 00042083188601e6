"""The parameter blob's layout and every weight order of csrc/net_layout.h, without a GPU and without the library.
tests/net_layout_driver.cpp (host compiler, net_layout.h only) prints the layout table and dumps every index map (dst[j] = blob[map[j]],
-1 = zero padding).  The expectations below were written from the lane rules as the kernels' comments and the packers that header
replaced state them, and from azhip.network.param_layout for the offsets -- not from net_layout.h:
  * the table is param_layout's running sums, name by name; the total is num_parameters and the oracle's net_num_params;
  * every map equals a numpy restatement of its order; every layer's map hits each weight of the layer once, the padding counts are
    the expected ones, the head maps stay inside the two head convolutions, `trainable` is 0 on running mean / variance only;
  * mutation leg: three wrong rules applied to the restatement are seen by at least one of the shapes."""
import os
import subprocess

import numpy as np
import pytest

import azref as R
from azhip import _lib as L
from azhip.network import ResNetHP, num_parameters, param_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# game -> (C, P, A, APAD): csrc/games.h
GEOM = {L.GAME_TICTACTOE: (3, 9, 9, 16), L.GAME_CONNECT_FOUR: (3, 42, 7, 8), L.GAME_MANCALA: (5, 14, 6, 8), L.GAME_GO9_PLANES: (4, 81, 82, 88)}
HEADS = [(32, 32), (4, 8), (2, 1)]           # k_heads16 and k_heads_mfma / k_heads_mfma only / neither
SHAPES = [(g, nb, F, h) for g in GEOM for nb in (0, 1, 2) for F in (64, 128) for h in HEADS]
IDS = ["g%d-nb%d-F%d-h%dx%d" % (g, nb, F, h[0], h[1]) for g, nb, F, h in SHAPES]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("net_layout")
    exe = str(d / "net_layout_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "net_layout_driver.cpp"), "-o", exe])

    def run(shape):
        """(layout table, maps by name, the trainer's working offsets, flags) of one shape"""
        g, nb, F, (npf, nvf) = shape
        out = str(d / "maps.bin")
        text = subprocess.run([exe] + [str(x) for x in GEOM[g] + (nb, F, npf, nvf, 1)] + [out], capture_output=True, text=True, check=True).stdout
        raw, at = np.fromfile(out, dtype=np.int32), 0
        table, maps, wk, flags = [], {}, {}, {}
        for kind, name, *val in (ln.split() for ln in text.splitlines()):
            if kind == "at":
                table.append((name, int(val[0])))
            elif kind == "map":
                maps[name] = raw[at:at + int(val[0])]
                at += int(val[0])
            elif kind == "wk":
                wk[name] = [int(v) for v in val]
            else:
                flags[kind] = int(name)
        assert at == raw.size
        return table, maps, wk, flags
    return run


@pytest.fixture(scope="module", params=SHAPES, ids=IDS)
def dumped(request, driver):
    """one driver run per shape, shared by the tests below"""
    return (request.param,) + driver(request.param)


# ------------------------------------------------------------------------------------------------------------- the restatement
def offsets(game, hp):
    at, n = {}, 0
    for name, shape in param_layout(game, hp):
        at[name] = n
        n += int(np.prod(shape))
    at["total"] = n
    return at


def flux(ksz, cin, tap, ci, co, mut=()):
    """Flux W[i + k (j + k (ci + Cin co))]; tap t = (dy+1)*3 + (dx+1) reads W[i = 1 - dx, j = 1 - dy] (true convolution)"""
    if ksz == 1:
        return ci + cin * co
    wi, wj = 1 - (tap % 3 - 1), 1 - (tap // 3 - 1)
    if "swap_wi_wj" in mut:
        wi, wj = wj, wi
    return wi + 3 * (wj + 3 * (ci + cin * co))


def grid(*dims):
    return np.meshgrid(*[np.arange(d) for d in dims], indexing="ij", sparse=True)


def frag32(ntap, cin, coutpad, src):
    """k_tower, 32x32x2: [tap][CoutPad/32][Cin/8][64][4], ci = (l >> 5) Cin/2 + 4 jq + q, co = 32 n + (l & 31)"""
    t, n, jq, l, q = grid(ntap, coutpad // 32, cin // 8, 64, 4)
    return np.broadcast_to(src(t, (l >> 5) * (cin // 2) + 4 * jq + q, 32 * n + (l & 31)), (ntap, coutpad // 32, cin // 8, 64, 4)).ravel()


def frag16(ntap, F, src):
    """k_tower16, 16x16x4: [tap][F/16][F/16][64][4], ci = (g & 1) F/2 + 2 (4 sq + q) + (g >> 1), g = l >> 4, co = 16 ct + (l & 15)"""
    t, ct, sq, l, q = grid(ntap, F // 16, F // 16, 64, 4)
    g = l >> 4
    return np.broadcast_to(src(t, (g & 1) * (F // 2) + 2 * (4 * sq + q) + (g >> 1), 16 * ct + (l & 15)), (ntap, F // 16, F // 16, 64, 4)).ravel()


def frag16b(ntap, F, src):
    """k_tower16b, bf16 16x16x32: [tap][F/16][F/32][64][8], ci = 32 ks + 8 (l >> 4) + el, co = 16 ct + (l & 15)"""
    t, ct, ks, l, el = grid(ntap, F // 16, F // 32, 64, 8)
    return np.broadcast_to(src(t, 32 * ks + 8 * (l >> 4) + el, 16 * ct + (l & 15)), (ntap, F // 16, F // 32, 64, 8)).ravel()


def stem32(C, F, src):
    """[F/32][K2][64]: k = t C + ci padded to 2 K2; lane l supplies k = (l >> 5) K2 + j for MFMA j, column 32 nt + (l & 31)"""
    K2 = (9 * C + 1) // 2
    nt, j, l = grid(F // 32, K2, 64)
    k = (l >> 5) * K2 + j + 0 * nt
    return np.where(k < 9 * C, src(k // C, k % C, 32 * nt + (l & 31)), -1).ravel()


def stem16(C, F, src):
    """[F/16][NS][64]: position p = 4 s + (l >> 4) of the interleaved halves, k = (p & 1) K2 + (p >> 1), column 16 ct + (l & 15)"""
    K2 = (9 * C + 1) // 2
    NS = (2 * K2 + 3) // 4
    ct, s, l = grid(F // 16, NS, 64)
    p = 4 * s + (l >> 4) + 0 * ct
    k = (p & 1) * K2 + (p >> 1)
    return np.where((k < 9 * C) & (p < 2 * K2), src(k // C, k % C, 16 * ct + (l & 15)), -1).ravel()


def gemm(ntap, cin, cout, src):
    t, ci, co = grid(ntap, cin, cout)
    return np.broadcast_to(src(t, ci, co), (ntap, cin, cout)).ravel()


def dense(at, nout, P, nf, width):
    """Flux Dense W[out + nout (p + P f)] -> k-major [k = p nf + f][width]"""
    p, f, o = grid(P, nf, width)
    return np.where(o < nout, at + o + nout * (p + P * f), -1).ravel()


def vector(at, n, width):
    return np.where(np.arange(width) < n, at + np.arange(width), -1)


def heads32(P, A, L_, F, npf, nvf, val, pol):
    """k_heads_mfma: value tiles then policy tiles of 32 columns; per MFMA pair i and lane: (W[4i+h][o], W[4i+2+h][o]), h = l >> 5"""
    out = []
    for mat, width, nf, ncol in ((val, F, nvf, F), (pol, L_, npf, A)):
        for tile in range((ncol + 31) // 32):
            i, l, e = grid(P * nf // 4, 64, 2)
            k, o = 4 * i + 2 * e + (l >> 5), tile * 32 + (l & 31) + 0 * i + 0 * e
            out.append(np.where(o < ncol, mat[k * width + np.minimum(o, width - 1)], -1).ravel())
    return np.concatenate(out)


def heads16(P, A, L_, F, val, pol):
    """k_heads16: tiles of 16 columns, per 16-k block j and lane a float4, element s = W[16 j + 4 s + (l >> 4)][16 tile + (l & 15)]"""
    out = []
    for mat, width, ncol in ((val, F, F), (pol, L_, A)):
        for tile in range((ncol + 15) // 16):
            j, l, s = grid(2 * P, 64, 4)
            k, o = 16 * j + 4 * s + (l >> 4), tile * 16 + (l & 15) + 0 * j + 0 * s
            out.append(np.where(o < ncol, mat[k * width + np.minimum(o, width - 1)], -1).ravel())
    return np.concatenate(out)


def restate(shape, mut=()):
    """every array of the driver, from the rules above"""
    g, nb, F, (npf, nvf) = shape
    C, P, A, L_ = GEOM[g]
    hp = ResNetHP(num_blocks=nb, num_filters=F, num_policy_head_filters=npf, num_value_head_filters=nvf)
    at = offsets(g, hp)
    if "npf_for_nvf" in mut:                                            # the value head's pieces laid out as if it had npf filters
        wrong = offsets(g, ResNetHP(num_blocks=nb, num_filters=F, num_policy_head_filters=npf, num_value_head_filters=npf))
        at = {k: (wrong[k] if k.startswith("vhead") else v) for k, v in at.items()}
    tower = ["block%d.conv%d.W" % (b, k) for b in range(nb) for k in (1, 2)]

    def conv(name, ksz, cin):
        return lambda t, ci, co: at[name] + flux(ksz, cin, t, ci, co, mut)

    def conv_dg(name):                                                  # the data gradient: in and out swapped, taps mirrored
        return lambda t, ci, co: at[name] + flux(3, F, t if "no_tap_mirror" in mut else 8 - t, co, ci, mut)

    def head(t, ci, co):                                                # policy filters, value filters, zero channels up to F
        return np.where(co < npf, at["phead.conv.W"] + ci + F * co, np.where(co < npf + nvf, at["vhead.conv.W"] + ci + F * (co - npf), -1))

    def head_vec(pname, vname):
        co = np.arange(F)
        return np.where(co < npf, at[pname] + co, np.where(co < npf + nvf, at[vname] + co - npf, -1))

    def cat(parts, pad):
        return np.concatenate([np.asarray(p, dtype=np.int64) for p in parts] + [np.full(pad, -1)])

    m = {}
    m["stem_w"] = stem32(C, F, conv("stem.conv.W", 3, C))
    m["s16_w"] = stem16(C, F, conv("stem.conv.W", 3, C))
    m["conv_w"] = cat([frag32(9, F, F, conv(n, 3, F)) for n in tower], 4)
    m["c16_w"] = cat([frag16(9, F, conv(n, 3, F)) for n in tower], 4)
    m["c16b_w"] = cat([frag16b(9, F, conv(n, 3, F)) for n in tower], 8)
    m["head_w"], m["h16_w"], m["h16b_w"] = frag32(1, F, F, head), frag16(1, F, head), frag16b(1, F, head)
    m["head_b"] = head_vec("phead.conv.b", "vhead.conv.b")
    m["head_bn"] = np.concatenate([head_vec("phead.bn." + k, "vhead.bn." + k) for k in ("gamma", "beta", "mean", "var")])
    m["pol_w"], m["pol_b"] = dense(at["phead.dense.W"], A, P, npf, L_), vector(at["phead.dense.b"], A, L_)
    m["val_w"], m["val_b"] = dense(at["vhead.dense1.W"], F, P, nvf, F), vector(at["vhead.dense1.b"], F, F)
    m["val2_w"] = vector(at["vhead.dense2.W"], F, F)
    m["hd_w"] = heads32(P, A, L_, F, npf, nvf, m["val_w"], m["pol_w"]) if npf % 4 == 0 and nvf % 4 == 0 else np.full(4, -1)
    m["hd16_w"] = heads16(P, A, L_, F, m["val_w"], m["pol_w"]) if (npf, nvf) == (32, 32) else np.full(4, -1)
    # the trainer: per convolution the GEMM matrix [taps cin][cout], for the tower's layers then the forward and the data-gradient
    # fragments; the dense matrices k-major, as wide as they have outputs; scat = the GEMM matrices and the dense layers
    parts, primary = [gemm(9, C, F, conv("stem.conv.W", 3, C))], [True]
    for n in tower:
        parts += [gemm(9, F, F, conv(n, 3, F)), frag16(9, F, conv(n, 3, F)), frag16(9, F, conv_dg(n))]
        primary += [True, False, False]
    parts += [gemm(1, F, npf, conv("phead.conv.W", 1, F)), gemm(1, F, nvf, conv("vhead.conv.W", 1, F)),
              dense(at["phead.dense.W"], A, P, npf, A), dense(at["vhead.dense1.W"], F, P, nvf, F), vector(at["vhead.dense2.W"], F, F)]
    primary += [True] * 5
    m["train_map"] = cat(parts, 0)
    starts = np.cumsum([0] + [len(p) for p in parts])
    m["train_scat"] = cat([np.arange(starts[i], starts[i + 1]) for i in range(len(parts)) if primary[i]], 0)
    m["trainable"] = np.ones(at["total"], dtype=np.int64)
    for name, shp in param_layout(g, hp):
        if name.endswith(".mean") or name.endswith(".var"):
            m["trainable"][at[name]:at[name] + shp[0]] = 0
    return at, m, starts


# ----------------------------------------------------------------------------------------------------------------------- tests
def test_layout_table_is_param_layout(dumped):
    (g, nb, F, (npf, nvf)), table = dumped[:2]
    hp = ResNetHP(num_blocks=nb, num_filters=F, num_policy_head_filters=npf, num_value_head_filters=nvf)
    want = offsets(g, hp)
    assert table == [(name, want[name]) for name, _ in param_layout(g, hp)] + [("total", want["total"])]
    assert want["total"] == num_parameters(g, hp) == R.net_num_params(g, nb, F, npf, nvf)


def test_every_map_is_its_lane_rule(dumped):
    shape, _, maps, wk, flags = dumped
    g, nb, F, (npf, nvf) = shape
    at, want, starts = restate(shape)
    assert set(maps) == set(want)
    for name in want:
        assert np.array_equal(maps[name], want[name]), name
    assert (flags["hd_ok"], flags["hd16_ok"]) == (int(npf % 4 == 0 and nvf % 4 == 0), int((npf, nvf) == (32, 32)))
    # the trainer's working offsets are where the restatement's pieces start
    got = [wk["conv0"][0]] + [o for l in range(1, 2 * nb + 1) for o in wk["conv%d" % l]] + [wk["conv%d" % (2 * nb + 1)][0], wk["conv%d" % (2 * nb + 2)][0]] + wk["dense"]
    assert got == list(starts[:-1])
    assert wk["conv0"][1:] == [0, 0] and wk["conv%d" % (2 * nb + 1)][1:] == [0, 0] and wk["conv%d" % (2 * nb + 2)][1:] == [0, 0]


def test_map_structure(dumped):
    (g, nb, F, (npf, nvf)), _, maps, wk, _ = dumped
    C, P, A, L_ = GEOM[g]
    hp = ResNetHP(num_blocks=nb, num_filters=F, num_policy_head_filters=npf, num_value_head_filters=nvf)
    at = offsets(g, hp)

    def once(m, name, n):                                               # hits every weight of the piece exactly once, nothing else but padding
        hit = m[m >= 0]
        assert np.array_equal(np.sort(hit), np.arange(at[name], at[name] + n)), name
        return m.size - hit.size

    nw = 9 * F * F
    for l in range(2 * nb):
        name = "block%d.conv%d.W" % (l // 2, l % 2 + 1)
        for arr in ("conv_w", "c16_w", "c16b_w"):
            assert once(maps[arr][l * nw:(l + 1) * nw], name, nw) == 0
        wm, ffwd, fdg = wk["conv%d" % (l + 1)]
        for o in (wm, ffwd, fdg):
            assert once(maps["train_map"][o:o + nw], name, nw) == 0
    assert [maps[a].size - 2 * nb * nw for a in ("conv_w", "c16_w", "c16b_w")] == [4, 4, 8]
    assert all((maps[a][2 * nb * nw:] == -1).all() for a in ("conv_w", "c16_w", "c16b_w"))
    K2 = (9 * C + 1) // 2
    assert once(maps["stem_w"], "stem.conv.W", 9 * C * F) == (F // 32) * K2 * 64 - 9 * C * F
    assert once(maps["s16_w"], "stem.conv.W", 9 * C * F) == (F // 16) * ((2 * K2 + 3) // 4) * 64 - 9 * C * F
    assert once(maps["train_map"][:9 * C * F], "stem.conv.W", 9 * C * F) == 0
    pw, vw = at["phead.conv.W"], at["vhead.conv.W"]
    for arr in ("head_w", "h16_w", "h16b_w"):                           # both head convolutions once, nothing outside them, F - npf - nvf zero channels
        m = maps[arr]
        hit = np.sort(m[m >= 0])
        assert np.array_equal(hit, np.concatenate([np.arange(pw, pw + F * npf), np.arange(vw, vw + F * nvf)])), arr
        assert m.size == F * F and m.size - hit.size == F * (F - npf - nvf)
    assert (maps["head_b"] < 0).sum() == F - npf - nvf and (maps["head_bn"] < 0).sum() == 4 * (F - npf - nvf)
    assert once(maps["pol_w"], "phead.dense.W", A * P * npf) == P * npf * (L_ - A)
    assert once(maps["val_w"], "vhead.dense1.W", F * P * nvf) == 0
    assert once(maps["pol_b"], "phead.dense.b", A) == L_ - A and once(maps["val_b"], "vhead.dense1.b", F) == 0 and once(maps["val2_w"], "vhead.dense2.W", F) == 0
    if npf % 4 == 0 and nvf % 4 == 0:
        m = maps["hd_w"]
        nv = F * P * nvf
        assert once(m[:nv], "vhead.dense1.W", nv) == 0
        assert once(m[nv:], "phead.dense.W", A * P * npf) == ((A + 31) // 32 * 32 - A) * P * npf
    else:
        assert np.array_equal(maps["hd_w"], np.full(4, -1))
    if (npf, nvf) == (32, 32):
        m = maps["hd16_w"]
        nv = F * P * nvf
        assert once(m[:nv], "vhead.dense1.W", nv) == 0
        assert once(m[nv:], "phead.dense.W", A * P * npf) == ((A + 15) // 16 * 16 - A) * P * npf
    else:
        assert np.array_equal(maps["hd16_w"], np.full(4, -1))
    # the scattered entries carry every weight's gradient once; the mask spares running mean and variance only
    weights = np.concatenate([np.arange(at[n], at[n] + int(np.prod(s))) for n, s in param_layout(g, hp) if n.endswith(".W")])
    assert np.array_equal(np.sort(maps["train_map"][maps["train_scat"]]), weights)
    frozen = np.concatenate([np.arange(at[n], at[n] + s[0]) for n, s in param_layout(g, hp) if n.endswith(".mean") or n.endswith(".var")])
    assert np.array_equal(np.flatnonzero(maps["trainable"] == 0), frozen) and set(np.unique(maps["trainable"])) == {0, 1}


def old_regularisation_walk(C, P, A, nb, F, npf, nvf):
    """The blob indices az_learning_status's regularisation sum visited while csrc/memory.hip still walked the blob by hand, restated from
    that walk: `take` n values, `skip` n values -- per convolution its weight, bias, gamma and beta taken, running mean and variance
    skipped; the dense layers taken whole.  Returns (the indices in the order visited, where the walk ended)."""
    at, seen = 0, []

    def take(n):
        nonlocal at
        seen.append(np.arange(at, at + n))
        at += n

    def skip(n):
        nonlocal at
        at += n

    take(9 * C * F); take(F); take(2 * F); skip(2 * F)
    for _ in range(2 * nb):
        take(9 * F * F); take(F); take(2 * F); skip(2 * F)
    take(F * npf); take(npf); take(2 * npf); skip(2 * npf); take(A * P * npf); take(A)
    take(F * nvf); take(nvf); take(2 * nvf); skip(2 * nvf); take(F * P * nvf); take(F); take(F); take(1)
    return np.concatenate(seen), at


@pytest.mark.parametrize("game,nb,F", [(L.GAME_TICTACTOE, 1, 64), (L.GAME_CONNECT_FOUR, 5, 64), (L.GAME_MANCALA, 5, 128), (L.GAME_GO9_PLANES, 10, 128)],
                         ids=["ttt-1x64", "c4-5x64", "mancala-5x128", "go9-10x128"])
def test_trainable_mask_marks_what_the_regularisation_walk_visited(driver, game, nb, F):
    """reg_sum_trainable sums blob[i]^2 over trainable_mask in ascending i; the hand walk it replaced visited exactly those i, ascending"""
    C_, P, A, _ = GEOM[game]
    table, maps, _, _ = driver((game, nb, F, (32, 32)))
    visited, end = old_regularisation_walk(C_, P, A, nb, F, 32, 32)
    assert end == dict(table)["total"] == maps["trainable"].size
    assert np.all(np.diff(visited) > 0)                                 # one accumulator in ascending blob order, then as now
    assert np.array_equal(np.flatnonzero(maps["trainable"]), visited)


@pytest.mark.parametrize("mut,arrays", [("swap_wi_wj", ("conv_w", "c16_w", "c16b_w", "stem_w", "s16_w", "train_map")),
                                        ("no_tap_mirror", ("train_map",)),
                                        ("npf_for_nvf", ("head_b", "head_bn", "val_w", "val_b", "val2_w", "train_map", "trainable"))])
def test_the_shapes_can_see_a_wrong_rule(driver, mut, arrays):
    """the restatement with one rule broken disagrees with the driver on at least one shape (and on the arrays that rule touches)"""
    seen = set()
    for shape in [s for s in SHAPES if s[1] == 1 and s[2] == 64]:       # one block, 64 filters: every game and head form
        maps = driver(shape)[1]
        _, wrong, _ = restate(shape, mut=(mut,))
        seen |= {name for name in wrong if not np.array_equal(maps[name], wrong[name])}
    assert seen >= set(arrays), (mut, seen)
