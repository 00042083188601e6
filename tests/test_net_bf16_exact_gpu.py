"""k_tower16b (csrc/resnet16b.h) against its float64 emulation on networks whose bf16 arithmetic is exact (tests/exact_nets.py).

Nothing rounds in such a tower, so a correct kernel's tower output equals the emulation's and only the fp32 heads are left:
the bound is TOL = 1e-5 of tests/test_net.py, where tests/test_net_bf16_gpu.py needs 1.5e-2 at depth 10.  A tap skipped in one
border class of one layer, a wrong neighbour-table entry, a skip connection that adds the wrong row or a mis-packed weight
fragment moves the output by 1e-3 and more (tests/test_exact_nets.py measures that on the CPU).  Every case forces each tile
count the engine can launch, asserts the kernel form it ran, and holds the forms to each other bit for bit (choose_tower's
invariant); the device games also go through the fused encode path.  A rounding leg covers what exact networks cannot see.

Every case prints its largest gap to the emulation; the fp32 CPU oracle, whose heads round like the device's, is within
3e-7 (P) and 1.2e-6 (V) of the emulation on these networks (tests/test_exact_nets.py)."""
import numpy as np
import pytest

import azref as R
import exact_nets as E
from test_net import TOL

pytestmark = pytest.mark.gpu

GAME_NAME = {R.C4: "ConnectFour", R.TTT: "TicTacToe", R.MANCALA: "Mancala", R.GO9: "Go9Planes"}
NTS = {R.C4: 3, R.TTT: 3, R.MANCALA: 3, R.GO9: 6}              # row tiles of the latency form: whole boards in at least 48 rows
SIZES = (1, 9, 43, 64)                                          # one board; one / several workgroups with a partial last one; the whole batch


def run_forms(game, hp, blob, X, A, keys, Pe, Ve, monkeypatch, towers, sizes, label):
    """one engine per forced form, every batch size on it; returns the largest gaps to the emulation"""
    import azhip
    F, out, gap = hp.num_filters, {}, [0.0, 0.0]
    small = dict(num_workers=1, batch_size=1, num_iters_per_turn=2) if keys is None else dict(num_workers=8, batch_size=8, num_iters_per_turn=8)
    for tower in towers:
        if tower:
            monkeypatch.setenv("AZHIP_TOWER", tower)
        else:
            monkeypatch.delenv("AZHIP_TOWER", raising=False)
        with azhip.Engine(game=game, oracle=azhip.ORACLE_RESNET, num_blocks=hp.num_blocks, num_filters=F, num_policy_head_filters=32,
                          num_value_head_filters=32, net_bf16=1, **small) as e:
            e.net_set_params(blob)
            for n in sizes:
                P, V, _ = e.net_forward(X[:n], A[:n])
                kernel = e.net_last_kernel()
                want = "k_tower16b<%s,%d,NT=" % (GAME_NAME[game], F)
                assert kernel.startswith(want) and (not tower or kernel == want + "%d>" % {"16": 11, "3": NTS[game], "22": 22}[tower]), (tower, kernel)
                if keys is not None:
                    Pk, Vk = e.net_evaluate_keys(keys[:n])
                    assert np.array_equal(P, Pk) and np.array_equal(V, Vk), (tower, n)      # planes path == fused encode path
                dP, dV = np.abs(P - Pe[:n]).max(), np.abs(V - Ve[:n]).max()
                gap = [max(gap[0], dP), max(gap[1], dV)]
                assert dP < TOL and dV < TOL, (label, kernel, n, dP, dV, np.argwhere(np.abs(P - Pe[:n]) >= TOL)[:8].tolist(), np.nonzero(np.abs(V - Ve[:n]) >= TOL)[0][:8].tolist())
                assert np.all(P[A[:n] == 0] == 0) and np.allclose(P.sum(1), 1, atol=1e-5)
                out[tower, n] = (P, V)
    for n in sizes:                                                 # every bf16 form computes the same bits
        for tower in towers[1:]:
            assert np.array_equal(out[tower, n][0], out[towers[0], n][0]) and np.array_equal(out[tower, n][1], out[towers[0], n][1]), (tower, n)
    print("exact bf16 %s: forms %s sizes %s: vs emulation dP %.2e dV %.2e" % (label, list(towers), list(sizes), gap[0], gap[1]))
    return gap


def forms(F):
    return ("16", "3", "22", "") if F == 128 else ("16", "3", "")   # 22 row tiles exist at 128 filters only


@pytest.mark.parametrize("name", [n for n in sorted(E.CONFIGS) if "dense" not in n])
def test_exact_network_within_fp32_head_tolerance(name, monkeypatch):
    game, hp, blob, X, A, keys = E.build(name)
    Pe, Ve = E.reference(name)[:2]
    run_forms(game, hp, blob, X, A, keys, Pe, Ve, monkeypatch, forms(hp.num_filters), SIZES, name)


@pytest.mark.parametrize("name", [n for n in sorted(E.CONFIGS) if "dense" in n])
def test_one_dense_layer_fills_every_weight_fragment_entry(name, monkeypatch):
    """one layer has a non-zero in every (input channel, tap, output channel) entry: the c16b_w packing of az_net_set_params"""
    game, hp, blob, X, A, keys = E.build(name)
    Pe, Ve = E.reference(name)[:2]
    run_forms(game, hp, blob, X, A, keys, Pe, Ve, monkeypatch, forms(hp.num_filters)[:-1], (43, 64), name)


@pytest.mark.parametrize("F", [64, 128])
def test_rounding_leg(F, monkeypatch):
    """The stem's outputs 257, 259, 257.5 and 1 + 2^-8 must be stored as 256, 260, 258 and 1 (round to nearest even) and the
    skip connection must add the STORED value; truncation, half-away-from-zero or an unrounded skip move the emulation by
    7e-4 and more (tests/test_exact_nets.py)."""
    game, hp, blob, X, A, keys = E.rounding_net(F)
    Pe, Ve = E.torch_forward_bf16(game, hp, blob, X, A)
    run_forms(game, hp, blob, X, A, keys, Pe, Ve, monkeypatch, ("16", "3") if F == 64 else ("22", "3"), (len(X),), "rounding leg %d filters" % F)
