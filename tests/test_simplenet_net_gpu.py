"""The SimpleNet engine's network (csrc/simplenet.h k_simplenet) through az_net_*:
  * P, V, Pinv of az_net_forward within 1e-5 of the float64 restatement (tests/simplenet_ref.py) for random networks;
  * batch independence, bit for bit: the same 40 boards at N = 1, 15, 16, 17, 31, 33, 257, in shuffled positions;
  * the same bits through every path: az_net_forward on encoded rows, az_net_evaluate_keys on the keys, and the priors
    az_mcts_node_stats reports after an explore of those roots;
  * exact networks (tests/simplenet_exact.py) at widths 15, 17 and 200, after the CPU has shown that every misplaced weight is visible;
  * refusals."""
import ctypes as C

import numpy as np
import pytest

import azhip
import azref as R
from azhip import _lib as L
from azhip.engine import default_cfg
from azhip.network import SimpleNetHP, simple_random_params
from simplenet_exact import exact_params, moved_weights
from simplenet_ref import GRID_WORLD_LIKE, TOL, TTT_SHIPPED, batch_of, forward64, keys_of, random_positions

pytestmark = pytest.mark.gpu

NETS = [(R.TTT, TTT_SHIPPED), (R.TTT, GRID_WORLD_LIKE),
        (R.C4, SimpleNetHP(width=100, depth_common=3, depth_phead=2, depth_vhead=0, use_batch_norm=True)),
        (R.MANCALA, SimpleNetHP(width=24, depth_common=2, depth_phead=0, depth_vhead=2, use_batch_norm=False)),
        (R.TTT, SimpleNetHP(width=1, depth_common=0, depth_phead=0, depth_vhead=0, use_batch_norm=True)),
        (R.C4, SimpleNetHP(width=256, depth_common=1, use_batch_norm=True))]
IDS = ["ttt-shipped", "ttt-gridworld", "c4-w100", "mancala-w24", "ttt-w1", "c4-w256"]


def engine(game, hp, **kw):
    kw.setdefault("num_workers", 64)
    kw.setdefault("batch_size", 64)
    kw.setdefault("num_iters_per_turn", 8)
    return azhip.Engine(game=game, simplenet=hp, **kw)


def biased(game, hp, seed):
    """random parameters with the biases moved off zero, so that a dropped or misplaced bias shows"""
    blob = simple_random_params(game, hp, seed)
    rng = np.random.default_rng(seed)
    off = 0
    from azhip.network import simple_param_layout
    for name, shape in simple_param_layout(game, hp):
        n = int(np.prod(shape))
        if name.endswith(".b"):
            blob[off:off + n] = rng.uniform(-0.2, 0.2, n)
        off += n
    return blob


@pytest.mark.parametrize("game,hp", NETS, ids=IDS)
def test_forward_within_tolerance_of_float64(game, hp):
    envs = random_positions(game, 70, seed=5)
    X, A = batch_of(game, envs)
    blob = biased(game, hp, seed=11)
    with engine(game, hp) as e:
        assert e.net_num_params() == blob.size
        e.net_set_params(blob)
        assert np.array_equal(e.net_get_params(), blob)
        P, V, Pinv = e.net_forward(X, A)
        assert e.net_last_kernel().startswith("k_simplenet<")
    Pr, Vr, Ir = forward64(game, hp, blob, X, A)
    dP, dV, dI = np.abs(P - Pr).max(), np.abs(V - Vr).max(), np.abs(Pinv - Ir).max()
    print("max |dP| %.3g |dV| %.3g |dPinv| %.3g" % (dP, dV, dI))
    assert dP <= TOL and dV <= TOL and dI <= TOL
    assert np.all(P[A == 0] == 0) and np.allclose(P.sum(axis=1), 1.0, atol=1e-5)


@pytest.mark.parametrize("width", [15, 17, 200])
def test_exact_networks(width):
    """tests/simplenet_exact.py: inputs 0 / 1, weights in {-1, 0, 1} with at most two non-zeros per row, batch-norm scales powers of two,
    every pre-activation a small integer in fp32; every depth above 1.  First, on the CPU: moving ANY single weight to the neighbouring
    index changes an output by more than 100 x the tolerance.  Then the device is held to the tolerance."""
    hp = SimpleNetHP(width=width, depth_common=2, depth_phead=2, depth_vhead=2, use_batch_norm=True)
    envs = random_positions(R.TTT, 64, seed=31)
    X, A = batch_of(R.TTT, envs)
    blob, mats = exact_params(R.TTT, hp, seed=1, Xcal=X)
    Pr, Vr, Ir = forward64(R.TTT, hp, blob, X, A)
    assert np.abs(Vr).max() < 0.999 and (Pr * (1 - Pr)).max() > 0.05          # neither tanh nor softmax saturated
    worst, moved = np.inf, 0
    for idx, m in moved_weights(blob, mats):
        P, V, I = forward64(R.TTT, hp, m, X, A)
        worst = min(worst, max(np.abs(P - Pr).max(), np.abs(V - Vr).max(), np.abs(I - Ir).max()))
        moved += 1
    print("width %d: %d weights moved, the least visible one changes an output by %.3g" % (width, moved, worst))
    assert moved == int(sum(np.count_nonzero(blob[o:o + n]) for o, n in mats)) and worst > 100 * TOL
    with engine(R.TTT, hp) as e:
        e.net_set_params(blob)
        P, V, Pinv = e.net_forward(X, A)
        Pk, Vk = e.net_evaluate_keys(keys_of(envs))
    dP, dV, dI = np.abs(P - Pr).max(), np.abs(V - Vr).max(), np.abs(Pinv - Ir).max()
    print("max |dP| %.3g |dV| %.3g |dPinv| %.3g" % (dP, dV, dI))
    assert dP <= TOL and dV <= TOL and dI <= TOL
    assert np.array_equal(P, Pk) and np.array_equal(V, Vk)


def test_shipped_network_size():
    with engine(R.TTT, TTT_SHIPPED) as e:
        assert e.net_num_params() == 336410


@pytest.mark.parametrize("game,hp", [NETS[0], NETS[2]], ids=[IDS[0], IDS[2]])
def test_batch_independence_bit_for_bit(game, hp):
    envs = random_positions(game, 40, seed=9)
    X, A = batch_of(game, envs)
    filler = batch_of(game, random_positions(game, 257, seed=10))
    rng = np.random.default_rng(3)
    with engine(game, hp) as e:
        e.net_set_params(biased(game, hp, seed=12))
        P0, V0, I0 = e.net_forward(X, A)
        for N in (1, 15, 16, 17, 31, 33, 257):
            # the 40 boards, a few at a time, at random positions of a batch of N otherwise filled with other boards
            for first in range(0, 40, N):
                mine = np.arange(first, min(first + N, 40))
                pos = rng.permutation(N)[:mine.size]
                Xb, Ab = filler[0][:N].copy(), filler[1][:N].copy()
                Xb[pos], Ab[pos] = X[mine], A[mine]
                P, V, Pinv = e.net_forward(Xb, Ab)
                assert np.array_equal(P[pos], P0[mine]) and np.array_equal(V[pos], V0[mine]) and np.array_equal(Pinv[pos], I0[mine]), N


@pytest.mark.parametrize("game,hp", [NETS[0], NETS[2], NETS[3]], ids=[IDS[0], IDS[2], IDS[3]])
def test_same_bits_through_every_path(game, hp):
    envs = random_positions(game, 40, seed=21)
    X, A = batch_of(game, envs)
    keys = keys_of(envs)
    with engine(game, hp, dirichlet_noise_eps=0.0, prior_temperature=1.0, reset_every=1) as e:
        e.net_set_params(biased(game, hp, seed=13))
        Xe, Ae = e.encode(keys)
        assert np.array_equal(Xe, X) and np.array_equal(Ae, A)
        P, V, _ = e.net_forward(X, A)
        Pk, Vk = e.net_evaluate_keys(keys)
        assert np.array_equal(P, Pk) and np.array_equal(V, Vk)
        e.mcts_explore(keys, 8)
        for s in range(len(envs)):
            N, W, Pn, Vn, mask = e.mcts_node_stats(s, keys[s])
            av = A[s] > 0
            assert np.array_equal(Pn[av], P[s][av]), s
            assert N.sum() == 7


def test_refusals():
    lib = L.lib()
    h = C.c_void_p()

    def hp_rec(**kw):
        rec = L.SimpleNetHPRec()
        L.check(lib.az_simplenet_hp_init(C.byref(rec)))
        for k, v in kw.items():
            setattr(rec, k, v)
        return rec

    rec = hp_rec()
    assert (rec.struct_size, rec.width, rec.depth_common, rec.depth_phead, rec.depth_vhead, rec.use_batch_norm) == (24, 200, 6, 1, 1, 1)
    cfg = default_cfg(game=R.TTT, num_workers=8, batch_size=8, num_iters_per_turn=4)
    for bad, frag in ((dict(width=0), b"width"), (dict(width=257), b"width"), (dict(depth_common=-1), b"depth"), (dict(depth_phead=17), b"depth"),
                      (dict(depth_vhead=-2), b"depth"), (dict(struct_size=20), b"az_simplenet_hp_init"), (dict(use_batch_norm=2), b"use_batch_norm")):
        r = hp_rec(**bad)
        assert lib.az_engine_create_simplenet(C.byref(cfg), C.byref(r), C.byref(h)) == L.AZ_ERR_BAD_ARG and frag in lib.az_last_error() and not h.value, bad
    go = default_cfg(game=L.GAME_GO9_PLANES, num_workers=8, batch_size=8, num_iters_per_turn=4)
    assert lib.az_engine_create_simplenet(C.byref(go), C.byref(rec), C.byref(h)) == L.AZ_ERR_BAD_ARG and not h.value
    bf = default_cfg(game=R.TTT, num_workers=8, batch_size=8, num_iters_per_turn=4, net_bf16=1)
    assert lib.az_engine_create_simplenet(C.byref(bf), C.byref(rec), C.byref(h)) == L.AZ_ERR_BAD_ARG and b"net_bf16" in lib.az_last_error() and not h.value
    plain = default_cfg(game=R.TTT, oracle=L.ORACLE_SIMPLENET, num_workers=8, batch_size=8, num_iters_per_turn=4)
    assert lib.az_engine_create(C.byref(plain), C.byref(h)) == L.AZ_ERR_BAD_ARG and b"az_engine_create_simplenet" in lib.az_last_error() and not h.value
    hp = SimpleNetHP(width=17, depth_common=1)
    with engine(R.TTT, hp, num_workers=8, batch_size=8) as e:
        n = e.net_num_params()
        for m in (n - 1, n + 1):
            with pytest.raises(azhip.AzError) as ei:
                e.net_set_params(np.zeros(m, dtype=np.float32))
            assert ei.value.status == L.AZ_ERR_BAD_ARG
        key = e.init_key()
        with pytest.raises(azhip.AzError) as ei:
            e.mcts_explore([key], 4)                                 # a search before az_net_set_params
        assert ei.value.status == L.AZ_ERR_STATE
        with pytest.raises(azhip.AzError) as ei:
            e.net_forward(*batch_of(R.TTT, [R.Game(R.TTT)]))
        assert ei.value.status == L.AZ_ERR_STATE
