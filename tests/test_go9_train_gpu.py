"""The 9x9x4 geometry (AZ_GAME_GO9_PLANES, 82 actions) learns: the optimiser step and the loss evaluation end to end on a data set
made from tensors, against the references the three device-twin games are held to (tests/test_train_gpu.py, tests/test_memory_gpu.py):
fp64 torch autograd in train mode with the device's ReLU masks, torch.optim.Adam trajectories, the oracle's Float32 learning status."""
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import azref as R
from azhip.network import param_layout
from test_train_gpu import TorchNet, _device_relu_masks, _rel_err_by_array

pytestmark = pytest.mark.gpu
GO = 3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def go_samples(n, seed):
    """random 0/1 planes, masks with at least one legal action (the pass action sometimes the only one), P a random distribution on
    the legal actions, V in [-1, 1], random positive W"""
    rng = np.random.default_rng(seed)
    X = rng.integers(0, 2, size=(n, 4, 9, 9)).astype(np.float32)
    A = (rng.random((n, 82)) < rng.uniform(0.2, 0.9, size=(n, 1))).astype(np.float32)
    A[:, 81] = 1.0
    A[::7, :81] = 0.0                                               # every seventh sample: pass only
    only_point = rng.integers(0, 81, size=n)
    for i in range(3, n, 11):                                       # and some without pass: one point
        A[i] = 0.0
        A[i, only_point[i]] = 1.0
    P = (rng.random((n, 82)) ** 3 * A).astype(np.float64)
    P = (P / P.sum(axis=1, keepdims=True)).astype(np.float32)
    P[A == 0] = 0.0
    V = rng.uniform(-1, 1, n).astype(np.float32)
    W = rng.uniform(0.25, 3.0, n).astype(np.float32)
    assert (A.sum(axis=1) >= 1).all() and (A[::7].sum(axis=1) == 1).all()
    return W, X, A, P, V


@pytest.mark.parametrize("nblocks,F,B", [(1, 64, 6), (1, 64, 16), (2, 128, 6), (2, 128, 16)])
def test_go9_gradients_match_torch_autograd(nblocks, F, B):
    """az_trainer_gradients vs TorchNet (fp64 autograd, train mode) differentiated with the DEVICE's ReLU masks: tol 1e-3 of each
    array's largest entry, l2_tol 3e-4; the loss parts within rtol 5e-5, atol 5e-6 (the bounds of tests/test_train_gpu.py)"""
    import azhip
    gspec = azhip.Go9PlanesSpec()
    data = go_samples(B + 5, 10 * B + F)
    hp = azhip.ResNetHP(num_blocks=nblocks, num_filters=F, num_policy_head_filters=32, num_value_head_filters=32)
    nn = azhip.ResNet(gspec, hp, seed=8)
    lp = azhip.LearningParams(samples_weighing_policy=0, l2_regularization=1e-4, loss_computation_batch_size=64, batch_size=B,
                              rewards_renormalization=2.0, nonvalidity_penalty=1.0, use_position_averaging=False)
    with azhip.TensorDataset(gspec, *data) as td, azhip.Trainer(gspec, nn, td, lp) as tr:
        assert tr.batch_size() == B
        idx = np.random.default_rng(5).choice(len(td), size=B, replace=False)
        loss, parts, grad = tr.gradients(idx)
        batch = [x[idx] for x in data]
        ref = TorchNet(GO, hp, nn.params())
        with torch.no_grad():
            L, (Lp, Lv, Lreg, Linv, scale) = ref.losses(batch, float(tr.Wmean), float(tr.Hp), 1e-4, 1.0, 2.0)
        print("go9 %dx%d B=%d: loss %.6f vs %.6f, parts %s" % (nblocks, F, B, loss, L.item(), parts))
        assert abs(loss - L.item()) < 2e-5 * max(1.0, abs(L.item()))
        assert np.allclose(parts, [Lp.item(), Lv.item(), Lreg.item(), Linv.item(), scale.item()], rtol=5e-5, atol=5e-6), (parts, Lp.item(), Lv.item(), Linv.item())
        masks, flips = _device_relu_masks(tr, hp, ref)
        ref2 = TorchNet(GO, hp, nn.params(), masks=masks)
        L2, (_, _, Lreg2, _, scale2) = ref2.losses(batch, float(tr.Wmean), float(tr.Hp), 1e-4, 1.0, 2.0)
        (L2 - scale2 * Lreg2).backward()                             # the device gradient excludes the L2 term (added in the update)
        assert abs(L2.item() - L.item()) < 1e-12 * max(1.0, abs(L.item()))
        worst = _rel_err_by_array(GO, hp, grad.astype(np.float64), ref2.blob(grads=True), tol=1e-3, l2_tol=3e-4)
        print("  largest relative gradient error %.2e, %d ReLU units differ" % (worst, flips))
        assert np.array_equal(tr.trained_params(), nn.params())       # the probe moves neither parameters nor running statistics


def test_go9_adam_steps_follow_torch():
    """three Adam steps vs torch.optim.Adam on the fp64 restatement (same batches through the shuffling contract), as
    tests/test_train_gpu.py::test_adam_steps_follow_torch: losses within rtol 2e-4, atol 2e-5, and the parameters moved"""
    import azhip
    from test_arena_oracle import _u64
    gspec, B, n = azhip.Go9PlanesSpec(), 16, 50
    data = go_samples(n, 77)
    hp = azhip.ResNetHP(num_blocks=1, num_filters=64, num_policy_head_filters=32, num_value_head_filters=32)
    nn = azhip.ResNet(gspec, hp, seed=2)
    lp = azhip.LearningParams(samples_weighing_policy=0, l2_regularization=1e-3, loss_computation_batch_size=64, batch_size=B,
                              optimiser=azhip.Adam(lr=1e-3), use_position_averaging=False)
    with azhip.TensorDataset(gspec, *data) as td, azhip.Trainer(gspec, nn, td, lp) as tr:
        ls = tr.batch_updates(3, seed=11)
        got = tr.trained_params()
        Wmean, Hp = float(tr.Wmean), float(tr.Hp)
    perm = list(range(n))
    for k, i in enumerate(range(n - 1, 0, -1)):
        j = min(int(_u64(11, 0, 0, 5, k) * (i + 1)), i)
        perm[i], perm[j] = perm[j], perm[i]
    ref = TorchNet(GO, hp, nn.params())
    train = [t for t in ref.p.values() if t.requires_grad]
    opt = torch.optim.Adam(train, lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
    run = {k: v.detach().clone() for k, v in ref.p.items() if k.endswith(".mean") or k.endswith(".var")}
    losses = []
    for s in range(3):
        idx = perm[s * B:(s + 1) * B]
        opt.zero_grad()
        L, _ = ref.losses([x[idx] for x in data], Wmean, Hp, 1e-3, 1.0, 1.0)
        L.backward()
        opt.step()
        losses.append(L.item())
        mom = hp.batch_norm_momentum
        for pre, (mu, var, m) in ref.batch_stats.items():
            run[pre + ".mean"] = (1 - mom) * run[pre + ".mean"] + mom * mu
            run[pre + ".var"] = (1 - mom) * run[pre + ".var"] + mom * var * (m / (m - 1))
    for k, v in run.items():
        ref.p[k] = v
    want = ref.blob()
    # The loss of step s is taken on the parameters after s updates, so the second and third loss hold the trajectory.  No bound on
    # the largest single parameter difference: Adam's update is lr m / (sqrt(v) + eps), of size lr whatever the gradient's size, so
    # an entry whose gradient lies within fp32 rounding of zero may step the other way (up to 2 lr per step) without any error in the
    # step.  The figure is printed (measured: 3.9e-4 on block0.conv1.W after three steps of lr 1e-3, median difference 1.5e-8).
    diff, off, where = np.abs(got - want), 0, None
    for name, shape in param_layout(GO, hp):
        k = int(np.prod(shape))
        if where is None or diff[off:off + k].max() > where[1]:
            where = (name, diff[off:off + k].max())
        off += k
    print("go9 adam: device %s torch %s, parameter difference max %.2e (%s) median %.2e" % (ls, losses, diff.max(), where[0], np.median(diff)))
    assert np.allclose(ls, losses, rtol=2e-4, atol=2e-5), (ls, losses)
    assert np.abs(got - nn.params()).max() > 5e-4                    # it did move (3 steps of lr 1e-3)


def _oracle_learning_status(hp, blob, data, l2, cinv, renorm, batch):
    """learning_status (learning.jl:158-181) restated in Float32 around the oracle's network: R.learning_status keeps its policies in
    arrays of 9 actions and does not take this geometry, so Network.forward_normalized comes from R.net_forward_normalized(R.GO9, ...)
    and the loss formula of oracle/azref.c (azr_learning_status) is restated here operation by operation: Float32 terms with the
    oracle's logf, Float64 sums, per-batch Float32 losses, batches averaged by their weight"""
    import ctypes as C
    W, X, A, P, V = [np.ascontiguousarray(x, dtype=np.float32) for x in data]
    n, nA = len(W), A.shape[1]
    f32 = np.float32
    logf = R.lib().azr_logf
    logf.restype, logf.argtypes = C.c_float, [C.c_float]
    lg = lambda a: np.array([logf(float(v)) for v in a], dtype=np.float32)
    eps = f32(1.1920929e-07)
    Ph, Vh, Pinv = R.net_forward_normalized(R.GO9, (hp.num_blocks, hp.num_filters, hp.num_policy_head_filters, hp.num_value_head_filters), blob, X, A)
    sw = float(W.astype(np.float64).sum())
    shp = sum(float(((P[i] * lg(P[i] + eps)) * W[i]).astype(np.float64).sum()) for i in range(n))
    Wmean, Hp = f32(sw / n), f32(-shp / sw)
    reg, off = 0.0, 0
    for name, shape in param_layout(GO, hp):
        k = int(np.prod(shape))
        if not (name.endswith(".mean") or name.endswith(".var")):
            reg += float((blob[off:off + k].astype(np.float64) ** 2).sum())
        off += k
    Lreg = f32(0) if l2 == 0 else f32(float(f32(l2)) * reg)
    acc = np.zeros(7)
    for b0 in range(0, n, min(batch, n)):
        idx = range(b0, min(n, b0 + min(batch, n)))
        bw = kl = hn = mse = inv = 0.0
        for i in idx:
            w = W[i]
            l = lg(Ph[i] + eps)
            bw += float(w)
            kl += float(((P[i] * l) * w).astype(np.float64).sum())
            hn += float(((Ph[i] * l) * w).astype(np.float64).sum())
            d = f32(Vh[i] / f32(renorm)) - f32(V[i] / f32(renorm))
            mse += float(f32(f32(d * d) * w))
            inv += float(f32(Pinv[i] * w))
        Lp = f32(f32(-kl / bw) - Hp)
        Lv = f32(mse / bw)
        Linv = f32(0) if cinv == 0 else f32(f32(cinv) * f32(inv / bw))
        L = f32(f32(f32(bw / len(idx)) / Wmean) * f32(f32(f32(Lp + Lv) + Lreg) + Linv))
        Hn = f32(-hn / bw)
        acc += np.array([float(L), float(Lp), float(Lv), float(Lreg), float(Linv), float(Hn), 1.0]) * bw
    out = (acc[:6] / acc[6]).astype(np.float32)
    return np.array([out[0], out[1], out[2], out[3], out[4], Hp, out[5]])


@pytest.mark.parametrize("F,n,batch", [(64, 40, 16), (128, 23, 1024)])
def test_go9_learning_status_matches_oracle(F, n, batch):
    """learning_status on Go tensors (test mode: the towers az_net_forward runs for this geometry) vs the oracle's Float32
    restatement (its network + the loss formula, see _oracle_learning_status), rtol 2e-6, atol 1e-7; a partial last loss batch at (40, 16)"""
    import azhip
    gspec = azhip.Go9PlanesSpec()
    data = go_samples(n, 5 + F)
    hp = azhip.ResNetHP(num_blocks=2, num_filters=F, num_policy_head_filters=32, num_value_head_filters=32)
    nn = azhip.ResNet(gspec, hp, seed=21)
    lp = azhip.LearningParams(samples_weighing_policy=0, l2_regularization=1e-4, loss_computation_batch_size=batch,
                              rewards_renormalization=1.0, nonvalidity_penalty=1.0, use_position_averaging=False)
    with azhip.TensorDataset(gspec, *data) as td, azhip.Trainer(gspec, nn, td, lp) as tr:
        st = tr.learning_status()
        rep = tr.samples_report()
    want = _oracle_learning_status(hp, nn.params(), data, 1e-4, 1.0, 1.0, batch)
    got = np.array([st.loss.L, st.loss.Lp, st.loss.Lv, st.loss.Lreg, st.loss.Linv, st.Hp, st.Hpnet])
    print("go9 learning status F=%d: device %s oracle %s" % (F, got, want))
    assert np.allclose(got, want, rtol=2e-6, atol=1e-7), (got, want)
    assert rep.num_samples == rep.num_boards == n and rep.Wtot == pytest.approx(float(data[0].astype(np.float64).sum()), rel=1e-12)


def test_go9_learns_one_batch():
    """20 Adam steps at lr 2e-3 on ONE fixed batch of 32 Go samples, 1x64: the last loss is below the first -- the step moves against
    the gradient (not a rate)"""
    import azhip
    gspec = azhip.Go9PlanesSpec()
    data = go_samples(32, 9)
    hp = azhip.ResNetHP(num_blocks=1, num_filters=64, num_policy_head_filters=32, num_value_head_filters=32)
    lp = azhip.LearningParams(samples_weighing_policy=0, l2_regularization=1e-4, loss_computation_batch_size=64, batch_size=32,
                              optimiser=azhip.Adam(lr=2e-3), use_position_averaging=False)
    with azhip.TensorDataset(gspec, *data) as td, azhip.Trainer(gspec, azhip.ResNet(gspec, hp, seed=3), td, lp) as tr:
        assert tr.batch_size() == 32 == len(td)                      # every epoch is this one batch
        ls = tr.batch_updates(20)
    print("go9 one batch, 20 Adam steps:", ls)
    assert np.isfinite(ls).all() and ls[-1] < ls[0], ls


def test_host_stepped_go9_trains_on_its_own_games():
    """examples/host_stepped_go9 --train-steps 3: the finished games' positions go through az_dataset_create_from_tensors and three Adam
    steps; exit 0 and three finite losses"""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples")], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(ROOT, "examples", "host_stepped_go9"), "--workers", "32", "--sims", "24", "--seconds", "1.5", "--threads", "2",
                        "--blocks", "1", "--filters", "64", "--train-steps", "3"], capture_output=True, text=True, timeout=120, cwd="/tmp")
    assert r.returncode == 0, r.stderr
    lines = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 2 and lines[0]["games_finished"] >= 1
    t = lines[1]
    print(t)
    assert t["train_steps"] == 3 and t["samples"] >= 2 and len(t["losses"]) == 3 and np.isfinite(t["losses"]).all()
