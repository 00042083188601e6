"""The SimpleNet parameter blob and every weight order of csrc/net_layout.h (SimpleLayout, SimpleMaps, SimpleTrainMaps), without a GPU and
without the library.  tests/simplenet_layout_driver.cpp (host compiler, net_layout.h only) prints the layout table and dumps every
index map (dst[j] = blob[map[j]], -1 = zero padding).  The expectations are written from simplenet.jl:37-64 (the order of the Flux arrays),
from azhip.network.simple_param_layout for the offsets and from the lane rule in simplenet.h's comment -- not from net_layout.h:
  * the table is simple_param_layout's running sums, layer by layer; the shipped Tic-tac-toe network is 336 410 values, 332 810 trainable;
  * every fragment map equals a numpy restatement of its order, hits each weight of its layer exactly once and pads with the expected
    number of zeros; no weight of the blob is in two layers' maps; vectors are padded to 16;
  * the trainer's matrices are k-major, each dense matrix once, `scat` lists all their entries; `trainable` is 0 on running mean /
    variance only;
  * mutation leg: two wrong lane rules applied to the restatement are seen."""
import os
import subprocess

import numpy as np
import pytest

from azhip import _lib as L
from azhip.network import SimpleNetHP, simple_param_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOM = {L.GAME_TICTACTOE: (27, 9), L.GAME_CONNECT_FOUR: (126, 7), L.GAME_MANCALA: (70, 6)}     # game -> (indim, A): csrc/games.h
WIDTHS = (1, 4, 15, 16, 17, 100, 200, 256)
DEPTHS = ((0, 0, 0), (6, 1, 1), (2, 0, 3))
SHAPES = [(g, w, d, bn) for g in GEOM for w in WIDTHS for d in DEPTHS for bn in (0, 1)]
IDS = ["g%d-w%d-d%d%d%d-bn%d" % ((g, w) + d + (bn,)) for g, w, d, bn in SHAPES]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("simplenet_layout")
    exe = str(d / "simplenet_layout_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "simplenet_layout_driver.cpp"), "-o", exe])

    def run(shape):
        g, w, dep, bn = shape
        out = str(d / "maps.bin")
        text = subprocess.run([exe] + [str(x) for x in GEOM[g] + (w,) + dep + (bn,)] + [out], capture_output=True, text=True, check=True).stdout
        raw, at = np.fromfile(out, dtype=np.int32), 0
        table, maps, wk, total, heads = [], {}, [], None, None
        for kind, name, *val in (ln.split() for ln in text.splitlines()):
            if kind == "at" and name == "total":
                total = int(val[0])
            elif kind == "at":
                table.append([int(v) for v in val])
            elif kind == "map":
                maps[name] = raw[at:at + int(val[0])]
                at += int(val[0])
            elif kind == "wk":
                wk.append(int(val[0]))
            elif kind == "heads":
                heads = (int(name), int(val[0]), int(val[1]))
        assert at == raw.size
        return table, maps, wk, total, heads
    return run


def hp_of(shape):
    g, w, dep, bn = shape
    return SimpleNetHP(width=w, depth_common=dep[0], depth_phead=dep[1], depth_vhead=dep[2], use_batch_norm=bool(bn))


def layers_of(shape):
    """[(in, out, W offset, b offset, bn offset or None, last)] from the Python layout's running sums"""
    g = shape[0]
    out, at, cur = [], 0, None
    for name, shp in simple_param_layout(g, hp_of(shape)):
        n = int(np.prod(shp))
        if name.endswith(".W"):
            cur = dict(out=shp[0], inn=shp[1], w=at, b=None, bn=None, last=".out." in name)
            out.append(cur)
        elif name.endswith(".b"):
            cur["b"] = at
        elif name.endswith(".gamma"):
            cur["bn"] = at
        at += n
    return out, at


def frag16(inn, outn, w, mut=()):
    """[OP/16][KP/16][64][4]: k = 16 j + 4 q + (l >> 4), column 16 ct + (l & 15); Flux W(o, i) at w + o + out i"""
    KP, OP = -(-inn // 16) * 16, -(-outn // 16) * 16
    ct, j, l, q = np.meshgrid(np.arange(OP // 16), np.arange(KP // 16), np.arange(64), np.arange(4), indexing="ij")
    k = 16 * j + 4 * q + (l >> 4)
    if "k_contiguous" in mut:
        k = 16 * j + 4 * (l >> 4) + q
    o = 16 * ct + (l & 15)
    idx = w + o + outn * k
    if "row_major" in mut:
        idx = w + k + inn * o
    return np.where((k < inn) & (o < outn), idx, -1).ravel().astype(np.int32)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_layout_and_maps(shape, driver):
    table, maps, wk, total, heads = driver(shape)
    want, n = layers_of(shape)
    assert total == n and len(table) == len(want)
    dc, dp, dv = shape[2]
    assert heads == (1 + dc, 1 + dc, 1 + dc + dp + 1)
    seen = np.zeros(n, dtype=np.int32)
    work = 0
    for l, (row, d) in enumerate(zip(table, want)):
        w, b, bn, inn, outn, hasbn, last = row
        assert (w, b, inn, outn, bool(last)) == (d["w"], d["b"], d["inn"], d["out"], d["last"])
        assert bool(hasbn) == (d["bn"] is not None) and (not hasbn or bn == d["bn"])
        m = maps["l%d.w" % l]
        assert np.array_equal(m, frag16(inn, outn, w))
        real = m[m >= 0]
        assert np.array_equal(np.sort(real), np.arange(w, w + inn * outn))           # each weight of the layer exactly once
        OP, KP = -(-outn // 16) * 16, -(-inn // 16) * 16
        assert m.size == OP * KP and m.size % 256 == 0
        seen[real] += 1
        vec = lambda at: np.where(np.arange(OP) < outn, at + np.arange(OP), -1)
        assert np.array_equal(maps["l%d.b" % l], vec(b))
        for k in range(4):
            mk = maps["l%d.bn%d" % (l, k)]
            assert np.array_equal(mk, vec(bn + k * outn)) if hasbn else mk.size == 0
        # the trainer: k-major [in][out]
        assert wk[l] == work
        i, o = np.meshgrid(np.arange(inn), np.arange(outn), indexing="ij")
        assert np.array_equal(maps["train_map"][work:work + inn * outn], (w + o + outn * i).ravel())
        work += inn * outn
    assert maps["train_map"].size == work and np.array_equal(maps["train_scat"], np.arange(work))
    nw = sum(d["inn"] * d["out"] for d in want)
    assert seen.sum() == nw and seen.max() == 1                                       # every dense matrix in the blob exactly once
    tr = np.ones(n, dtype=np.int32)
    for d in want:
        if d["bn"] is not None:
            tr[d["bn"] + 2 * d["out"]:d["bn"] + 4 * d["out"]] = 0
    assert np.array_equal(maps["trainable"], tr)
    if not shape[3]:
        assert tr.all() and n == nw + sum(d["out"] for d in want)                    # without batch norm the four vectors are absent


def test_shipped_tictactoe_sizes(driver):
    """games/tictactoe/params.jl: width 200, depth_common 6, batch norm, head depths 1"""
    table, maps, wk, total, heads = driver((L.GAME_TICTACTOE, 200, (6, 1, 1), 1))
    assert total == 336410 and int(maps["trainable"].sum()) == 332810


def test_wrong_lane_rules_are_seen(driver):
    shape = (L.GAME_TICTACTOE, 17, (2, 0, 3), 1)
    table, maps, wk, total, heads = driver(shape)
    for mut in ("k_contiguous", "row_major"):
        assert any(not np.array_equal(maps["l%d.w" % l], frag16(r[3], r[4], r[0], mut=(mut,))) for l, r in enumerate(table)), mut


def test_python_mirror_of_the_network(tmp_path):
    """azhip.network.SimpleNet without a device: sizes, initial parameters, split_params, save / load"""
    import azhip
    from azhip.network import SimpleNet, load_params, save_params
    gspec = azhip.TicTacToeSpec()
    hp = SimpleNetHP(width=200, depth_common=6, use_batch_norm=True, batch_norm_momentum=1.0)
    nn = SimpleNet(gspec, hp, seed=5)
    assert nn.params().size == 336410 and nn.num_parameters() == 332810
    p = nn.split_params()
    assert [k for k, _ in nn.param_layout()][:6] == ["common0.dense.W", "common0.dense.b", "common0.bn.gamma", "common0.bn.beta", "common0.bn.mean", "common0.bn.var"]
    assert p["common0.dense.W"].shape == (200, 27) and p["phead.out.W"].shape == (9, 200) and p["vhead.out.W"].shape == (1, 200)
    assert all(not v.any() for k, v in p.items() if k.endswith(".b"))                # Flux's zero biases
    w = p["common3.dense.W"]
    assert np.abs(w).max() <= np.sqrt(6.0 / 400) and w.std() > 0.05                   # Glorot uniform
    assert np.abs(p["common2.bn.var"] - 1).max() <= 0.1 and np.abs(p["common2.bn.mean"]).max() <= 0.1
    assert nn.engine_options() == dict(simplenet=hp) and azhip.MCTS.oracle_kind(nn) == L.ORACLE_SIMPLENET
    path = str(tmp_path / "net.bin")
    save_params(path, nn)
    back = load_params(path, gspec)
    assert isinstance(back, SimpleNet) and np.array_equal(back.params(), nn.params())
    assert (back.hyper.width, back.hyper.depth_common, back.hyper.depth_phead, back.hyper.depth_vhead, back.hyper.use_batch_norm) == (200, 6, 1, 1, True)
    with pytest.raises(ValueError):
        SimpleNet(gspec, hp, params=np.zeros(10, dtype=np.float32))
    plain = SimpleNet(gspec, SimpleNetHP(width=100, depth_common=4), seed=1)           # grid-world's shape: no batch-norm vectors at all
    assert plain.params().size == plain.num_parameters() == 27 * 100 + 100 + 6 * (100 * 100 + 100) + 9 * 100 + 9 + 100 + 1
