"""The optimiser step and the loss evaluation of a SimpleNet engine (az_trainer_* on the dense chain of csrc/train.hip, az_learning_status)
against float64 restatements: NetLib.SimpleNet in TRAIN mode (simplenet.jl:37-64: BatchNorm with batch statistics), `losses`
(learning.jl:67-90), torch autograd gradients in Flux parameter order, Adam and CyclicNesterov trajectories, running statistics.
Tolerances and the ReLU-mask handling are tests/test_train_gpu.py's: gradients relative to the largest entry of each parameter array,
the reference differentiated with the DEVICE's ReLU masks (az_debug_trainer_activation) at 1e-3 and with its own at 1e-2.

Tolerance of the loss figures of az_learning_status.  The device's P, V, Pinv are within TOL = 1e-5 of the float64 network (the network
contract, tests/test_simplenet_net_gpu.py).  Propagated through the loss terms of the float64 reference itself:
  Lp, Hpnet   |d log(p + eps)| <= TOL / (p + eps) per entry, weighted by P (Lp) or |log p + 1| (Hpnet)
  Lv          |d (v - z)^2| <= 2 |v - z| TOL + TOL^2
  Linv        <= cinv TOL
plus 2e-6 relative for the Float32 arithmetic of the sums (the bound tests/test_memory_gpu.py uses against a Float32 oracle)."""
import ctypes as C

import numpy as np
import pytest
import torch

import azhip
from azhip import _lib as L
from azhip.network import SimpleNet, SimpleNetHP, simple_param_layout
from simplenet_ref import EPS32, TOL, TTT_SHIPPED, forward64, split
from test_train_gpu import _MaskedRelu

pytestmark = pytest.mark.gpu
SPECS = {0: "ConnectFourSpec", 1: "TicTacToeSpec", 2: "MancalaSpec"}


def memory_of(gspec, game, ngames=24, workers=8, nsims=24, seed=9):
    with azhip.Engine(game=game, oracle=azhip.ORACLE_HASH, num_workers=workers, batch_size=workers, num_iters_per_turn=nsims,
                      dirichlet_noise_eps=0.25, cpuct=1.0, reset_every=1, temperature=([0], [1.0]), seed=seed) as e:
        games, moves, ng, nm, _ = e.selfplay_run(ngames)
    mem = azhip.MemoryBuffer(gspec, 100000)
    mem.push_records(games, moves, ng, nm, 1.0)
    return mem


# ------------------------------------------------------------------------------------------------------------------ loss evaluation
def status64(game, hp, blob, trainable, data, l2, cinv, batch):
    """(figures, bounds): L, Lp, Lv, Lreg, Linv, Hp, Hpnet in float64 and what TOL on the network outputs can move each by"""
    W, X, A, P, V = [np.asarray(t, dtype=np.float64) for t in data]
    Wmean = W.mean()
    Hp = -(P * np.log(P + EPS32) * W[:, None]).sum() / W.sum()
    Lreg = l2 * float((np.asarray(blob, dtype=np.float64)[trainable] ** 2).sum())
    fig, bnd, ws = [], [], []
    for b0 in range(0, len(W), batch):
        s = slice(b0, min(b0 + batch, len(W)))
        Ph, Vh, Pinv = forward64(game, hp, blob, X[s], A[s])
        w, sw = W[s], W[s].sum()
        Lp = -(P[s] * np.log(Ph + EPS32) * w[:, None]).sum() / sw - Hp
        Lv = ((Vh - V[s]) ** 2 * w).sum() / sw
        Linv = cinv * (Pinv * w).sum() / sw
        Hn = -(Ph * np.log(Ph + EPS32) * w[:, None]).sum() / sw
        scale = w.mean() / Wmean
        bLp = TOL * (P[s] / (Ph + EPS32) * w[:, None]).sum() / sw
        bLv = ((2 * np.abs(Vh - V[s]) * TOL + TOL ** 2) * w).sum() / sw
        bHn = TOL * (np.abs(np.log(Ph + EPS32) + 1.0) * (A[s] > 0) * w[:, None]).sum() / sw
        fig.append([scale * (Lp + Lv + Lreg + Linv), Lp, Lv, Lreg, Linv, Hp, Hn])
        bnd.append([scale * (bLp + bLv + cinv * TOL), bLp, bLv, 0.0, cinv * TOL, 0.0, bHn])
        ws.append(sw)
    ws = np.array(ws) / np.sum(ws)
    return ws @ np.array(fig), ws @ np.array(bnd)


@pytest.mark.parametrize("game,hp,policy,batch", [
    (1, TTT_SHIPPED, 2, 1 << 20),
    (1, SimpleNetHP(width=100, depth_common=4, use_batch_norm=False), 0, 37),
    (0, SimpleNetHP(width=100, depth_common=2, depth_phead=2, use_batch_norm=True), 1, 64),
], ids=["ttt-shipped-log-weight", "ttt-no-bn-batch37", "c4-w100"])
def test_learning_status_matches_float64(game, hp, policy, batch):
    gspec = getattr(azhip, SPECS[game])()
    nn = SimpleNet(gspec, hp, seed=21)
    mem = memory_of(gspec, game)
    lp = azhip.LearningParams(samples_weighing_policy=policy, l2_regularization=1e-4, loss_computation_batch_size=batch,
                              rewards_renormalization=1.0, nonvalidity_penalty=1.0)
    with azhip.Trainer(gspec, nn, mem, lp, use_symmetries=True) as tr:
        st = tr.learning_status()
        data = tr.data.tensors()
    trainable = np.array([not (n.endswith(".mean") or n.endswith(".var")) for n, s in nn.param_layout() for _ in range(int(np.prod(s)))])
    assert trainable.sum() == nn.num_parameters()
    want, bound = status64(game, hp, nn.params(), trainable, data, 1e-4, 1.0, min(batch, len(data[0])))
    got = np.array([st.loss.L, st.loss.Lp, st.loss.Lv, st.loss.Lreg, st.loss.Linv, st.Hp, st.Hpnet])
    print("device ", got, "\nfloat64", want, "\nbound  ", bound)
    assert np.all(np.abs(got - want) <= bound + 2e-6 * np.abs(want) + 1e-7), (got, want, bound)
    assert st.loss.Lreg > 0 and len(data[0]) > 100
    mem.close()


# ------------------------------------------------------------------------------------------------------------------ the optimiser step
class TorchDense:
    """float64 restatement of the Flux SimpleNet in TRAIN mode + `losses`, parameters in Julia shapes.  masks (optional): layer name ->
    0/1 tensor; that layer's ReLU then differentiates with the given mask instead of (z > 0)."""

    def __init__(self, game, hp, blob, masks=None):
        self.game, self.hp = game, hp
        self.masks, self.own_masks, self.batch_stats = masks or {}, {}, {}
        self.names = [n for n, _ in simple_param_layout(game, hp)]
        self.p = {k: torch.tensor(np.ascontiguousarray(v), dtype=torch.float64, requires_grad=not (k.endswith(".mean") or k.endswith(".var")))
                  for k, v in split(game, hp, blob).items()}
        self.hidden = (["common%d" % l for l in range(hp.depth_common + 1)] + ["phead%d" % l for l in range(hp.depth_phead)]
                       + ["vhead%d" % l for l in range(hp.depth_vhead)])

    def blob(self, grads=False):
        out = []
        for n in self.names:
            t = self.p[n]
            a = (t.grad if grads else t.detach()) if (not grads or t.requires_grad) else None
            a = np.zeros(tuple(t.shape)) if a is None else a.numpy()
            out.append(np.asarray(a).reshape(-1, order="F"))
        return np.concatenate(out)

    def D(self, x, pre):
        z = x @ self.p[pre + ".dense.W"].T + self.p[pre + ".dense.b"]
        if self.hp.use_batch_norm:
            mu, var = z.mean(dim=0), z.var(dim=0, unbiased=False)
            self.batch_stats[pre + ".bn"] = (mu.detach(), var.detach(), z.shape[0])
            z = self.p[pre + ".bn.gamma"] * (z - mu) / torch.sqrt(var + 1e-5) + self.p[pre + ".bn.beta"]
        self.own_masks[pre] = (z.detach() > 0).to(torch.float64)
        return _MaskedRelu.apply(z, self.masks[pre]) if pre in self.masks else torch.relu(z)

    def forward(self, X):
        hp = self.hp
        x = X.reshape(X.shape[0], -1)
        for l in range(hp.depth_common + 1):
            x = self.D(x, "common%d" % l)
        y, v = x, x
        for l in range(hp.depth_phead):
            y = self.D(y, "phead%d" % l)
        for l in range(hp.depth_vhead):
            v = self.D(v, "vhead%d" % l)
        logits = y @ self.p["phead.out.W"].T + self.p["phead.out.b"]
        val = torch.tanh(v @ self.p["vhead.out.W"].T + self.p["vhead.out.b"]).reshape(-1)
        return torch.softmax(logits, dim=1), val

    def losses(self, batch, Wmean, Hp, l2, cinv, rho):
        W, X, A, P, V = [torch.tensor(np.asarray(x), dtype=torch.float64) for x in batch]
        pol, val = self.forward(X)
        pm = pol * A
        sp = pm.sum(dim=1, keepdim=True)
        Ph = pm / (sp + EPS32)
        Lp = -(P * torch.log(Ph + EPS32) * W[:, None]).sum() / W.sum() - Hp
        Lv = (((val / rho - V / rho) ** 2) * W).sum() / W.sum()
        Lreg = l2 * sum((t ** 2).sum() for t in self.p.values() if t.requires_grad)
        Linv = cinv * ((1 - sp).reshape(-1) * W).sum() / W.sum()
        scale = W.mean() / Wmean
        return scale * (Lp + Lv + Lreg + Linv), (Lp, Lv, Lreg, Linv, scale)


def device_relu_masks(tr, ref):
    """the ReLU masks (a > 0) of the device's last forward pass: layer `which` of the dense chain in blob order, [batch][out]"""
    f = L.lib().az_debug_trainer_activation
    f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64]
    hp, out = ref.hp, {}
    which = {**{"common%d" % l: l for l in range(hp.depth_common + 1)},
             **{"phead%d" % l: hp.depth_common + 1 + l for l in range(hp.depth_phead)},
             **{"vhead%d" % l: hp.depth_common + 1 + hp.depth_phead + 1 + l for l in range(hp.depth_vhead)}}
    for name in ref.hidden:
        own = ref.own_masks[name]
        a = np.zeros(own.numel(), dtype=np.float32)
        L.check(f(tr._trainer(), which[name], a.ctypes.data_as(C.c_void_p), a.size))
        m = torch.tensor(a.reshape(tuple(own.shape)) > 0).to(torch.float64)
        d = int((m != own).sum())
        assert d <= max(8, own.numel() // 20000), (name, d, own.numel())   # the same network: only units within rounding of zero differ
        out[name] = m
    return out


def rel_err_by_array(game, hp, got, want, tol, l2_tol):
    """every array: max |got - want| <= tol * max |want| + 2e-6 and ||got - want||_2 <= l2_tol ||want||_2 + 1e-7 (tests/test_train_gpu.py)"""
    off = 0
    for name, shape in simple_param_layout(game, hp):
        n = int(np.prod(shape))
        g, w = got[off:off + n], want[off:off + n]
        off += n
        if name.endswith(".mean") or name.endswith(".var"):
            assert not g.any()
            continue
        denom = max(np.abs(w).max(), 1e-7)
        assert np.abs(g - w).max() <= tol * denom + 2e-6, (name, np.abs(g - w).max(), denom)
        assert np.linalg.norm(g - w) <= l2_tol * np.linalg.norm(w) + 1e-7, (name, np.linalg.norm(g - w), np.linalg.norm(w))


GRAD_CASES = [(1, w, bn, B) for w in (24, 200) for bn in (True, False) for B in (5, 32, 70)] + [(0, 100, True, 32)]


@pytest.fixture(scope="module")
def memories():
    made = {}

    def get(game):
        if game not in made:
            gspec = getattr(azhip, SPECS[game])()
            made[game] = (gspec, memory_of(gspec, game, ngames=16, nsims=16, seed=3))
        return made[game]
    yield get
    for _, mem in made.values():
        mem.close()


@pytest.mark.parametrize("game,width,bn,B", GRAD_CASES, ids=["g%d-w%d-bn%d-B%d" % (g, w, bn, B) for g, w, bn, B in GRAD_CASES])
def test_gradients_match_torch_autograd(game, width, bn, B, memories):
    """batch 70 crosses the 64-row chunk of k_tr_colsum"""
    gspec, mem = memories(game)
    hp = SimpleNetHP(width=width, depth_common=2, use_batch_norm=bn)
    nn = SimpleNet(gspec, hp, seed=8)
    blob = nn.params().copy()
    off = 0
    rng = np.random.default_rng(4)
    for name, shape in nn.param_layout():                            # biases off zero: a bias gradient in the wrong slot then shows in the loss too
        n = int(np.prod(shape))
        if name.endswith(".b"):
            blob[off:off + n] = rng.uniform(-0.2, 0.2, n)
        off += n
    nn = SimpleNet(gspec, hp, params=blob)
    lp = azhip.LearningParams(samples_weighing_policy=1, l2_regularization=1e-4, loss_computation_batch_size=64, batch_size=B,
                              rewards_renormalization=2.0, nonvalidity_penalty=1.0)
    with azhip.Trainer(gspec, nn, mem, lp, use_symmetries=True) as tr:
        data = tr.data.tensors()
        n = len(data[0])
        assert n >= B and tr.batch_size() == B
        idx = np.random.default_rng(5).choice(n, size=B, replace=False)
        loss, parts, grad = tr.gradients(idx)
        batch = [x[idx] for x in data]
        ref = TorchDense(game, hp, blob)
        Lr, (Lp, Lv, Lreg, Linv, scale) = ref.losses(batch, float(tr.Wmean), float(tr.Hp), 1e-4, 1.0, 2.0)
        (Lr - scale * Lreg).backward()                               # the device gradient excludes the L2 term (added in the update)
        want = ref.blob(grads=True)
        print("loss device %.8g float64 %.8g" % (loss, Lr.item()))
        assert abs(loss - Lr.item()) < 2e-5 * max(1.0, abs(Lr.item()))
        assert np.allclose(parts, [Lp.item(), Lv.item(), Lreg.item(), Linv.item(), scale.item()], rtol=5e-5, atol=5e-6), (parts, Lp.item(), Lv.item())
        ref2 = TorchDense(game, hp, blob, masks=device_relu_masks(tr, ref))
        L2, (_, _, Lreg2, _, scale2) = ref2.losses(batch, float(tr.Wmean), float(tr.Hp), 1e-4, 1.0, 2.0)
        (L2 - scale2 * Lreg2).backward()
        assert abs(L2.item() - Lr.item()) < 1e-12 * max(1.0, abs(Lr.item()))
        rel_err_by_array(game, hp, grad.astype(np.float64), ref2.blob(grads=True), tol=1e-3, l2_tol=3e-4)
        rel_err_by_array(game, hp, grad.astype(np.float64), want, tol=1e-2, l2_tol=1e-3)
        assert np.array_equal(tr.trained_params(), blob)             # the probe moves neither parameters nor running statistics
        if bn:                                                       # with batch norm the Dense biases before it have gradient 0 exactly
            p = split(game, hp, grad)
            assert all(not v.any() for k, v in p.items() if k.endswith(".dense.b"))


def shuffled(n, seed):
    """the contract's shuffle: Fisher-Yates from the last index, draw k -> floor(u * (i + 1)), purpose 5, game word = epoch"""
    from test_arena_oracle import _u64
    perm = list(range(n))
    for k, i in enumerate(range(n - 1, 0, -1)):
        j = min(int(_u64(seed, 0, 0, 5, k) * (i + 1)), i)
        perm[i], perm[j] = perm[j], perm[i]
    return perm


def running_update(ref, run, mom):
    for pre, (mu, var, m) in ref.batch_stats.items():
        run[pre + ".mean"] = (1 - mom) * run[pre + ".mean"] + mom * mu
        run[pre + ".var"] = (1 - mom) * run[pre + ".var"] + mom * var * (m / (m - 1))


@pytest.mark.parametrize("mom", [1.0, 0.1])
def test_running_statistics_after_one_step(mom, memories):
    """momentum 1.0 is the shipped Tic-tac-toe setting: the running statistics ARE the last batch's (unbiased variance)"""
    gspec, mem = memories(1)
    hp = SimpleNetHP(width=24, depth_common=2, use_batch_norm=True, batch_norm_momentum=mom)
    nn = SimpleNet(gspec, hp, seed=12)
    B = 32
    lp = azhip.LearningParams(samples_weighing_policy=1, l2_regularization=1e-4, loss_computation_batch_size=64, batch_size=B, optimiser=azhip.Adam(lr=1e-3))
    with azhip.Trainer(gspec, nn, mem, lp, use_symmetries=True) as tr:
        data = tr.data.tensors()
        tr.batch_updates(1, seed=7)
        got = split(1, hp, tr.trained_params())
        idx = shuffled(len(data[0]), 7)[:B]
        ref = TorchDense(1, hp, nn.params())
        ref.losses([x[idx] for x in data], float(tr.Wmean), float(tr.Hp), 1e-4, 1.0, 1.0)
        run = {k: v.detach().clone() for k, v in ref.p.items() if k.endswith(".mean") or k.endswith(".var")}
        running_update(ref, run, mom)
        assert len(run) == 2 * 5
        for k, v in run.items():
            assert np.abs(got[k] - v.numpy()).max() < 2e-4, (k, np.abs(got[k] - v.numpy()).max())
            if mom == 1.0:
                assert np.abs(got[k] - split(1, hp, nn.params())[k]).max() > 1e-2   # nothing of the initial statistics is left


@pytest.mark.parametrize("bn", [True, False])
def test_adam_steps_follow_torch(bn, memories):
    """three Adam steps against torch.optim.Adam on the float64 restatement, same batches; tolerances of tests/test_train_gpu.py"""
    game, B = 1, 32
    gspec, mem = memories(game)
    hp = SimpleNetHP(width=200 if bn else 24, depth_common=2, use_batch_norm=bn, batch_norm_momentum=0.6)
    nn = SimpleNet(gspec, hp, seed=2)
    lp = azhip.LearningParams(samples_weighing_policy=1, l2_regularization=1e-3, loss_computation_batch_size=64, batch_size=B, optimiser=azhip.Adam(lr=1e-3))
    with azhip.Trainer(gspec, nn, mem, lp, use_symmetries=True) as tr:
        data = tr.data.tensors()
        ls = tr.batch_updates(3, seed=11)
        got = tr.trained_params()
        perm = shuffled(len(data[0]), 11)
        ref = TorchDense(game, hp, nn.params())
        train = [t for t in ref.p.values() if t.requires_grad]
        opt = torch.optim.Adam(train, lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
        run = {k: v.detach().clone() for k, v in ref.p.items() if k.endswith(".mean") or k.endswith(".var")}
        losses = []
        for s in range(3):
            opt.zero_grad()
            Lr, _ = ref.losses([x[perm[s * B:(s + 1) * B]] for x in data], float(tr.Wmean), float(tr.Hp), 1e-3, 1.0, 1.0)
            Lr.backward()
            opt.step()
            losses.append(Lr.item())
            running_update(ref, run, 0.6)
        for k, v in run.items():
            ref.p[k] = v
        want = ref.blob()
        print("losses device", ls, "float64", losses, "max |dparam| %.3g" % np.abs(got - want).max())
        assert np.allclose(ls, losses, rtol=2e-4, atol=2e-5), (ls, losses)
        assert np.abs(got - want).max() < 2e-4, np.abs(got - want).max()
        assert np.abs(got - nn.params()).max() > 5e-4               # it did move


def test_cyclic_nesterov_steps_follow_the_reference_rule(memories):
    """three CyclicNesterov steps (flux.jl:78-94: Optimisers.Nesterov, lr / momentum from CyclicSchedule, adjust! after update!)"""
    game, B, n = 1, 32, 3
    gspec, mem = memories(game)
    hp = SimpleNetHP(width=200, depth_common=2, use_batch_norm=True, batch_norm_momentum=1.0)
    nn = SimpleNet(gspec, hp, seed=3)
    opt = azhip.CyclicNesterov(lr_base=1e-3, lr_high=1e-2, lr_low=1e-3, momentum_low=0.8, momentum_high=0.9)   # games/tictactoe/params.jl
    lp = azhip.LearningParams(samples_weighing_policy=2, l2_regularization=1e-4, loss_computation_batch_size=64, batch_size=B, optimiser=opt)

    def pl(xs, ys, i):
        pt = max([k for k in range(4) if xs[k] <= i], default=-1)
        if pt < 0:
            return ys[0]
        if pt == 3 or xs[pt + 1] == xs[pt]:
            return ys[pt]
        return ys[pt] + (ys[pt + 1] - ys[pt]) / (xs[pt + 1] - xs[pt]) * (i - xs[pt])
    xs = [1, int(0.45 * n), int(0.9 * n), n]
    with azhip.Trainer(gspec, nn, mem, lp, use_symmetries=True) as tr:
        data = tr.data.tensors()
        ls = tr.batch_updates(n, seed=2)
        got = tr.trained_params()
        perm = shuffled(len(data[0]), 2)
        ref = TorchDense(game, hp, nn.params())
        train = [t for t in ref.p.values() if t.requires_grad]
        vel = [torch.zeros_like(t) for t in train]
        for s in range(n):
            lr = 1e-3 if s == 0 else pl(xs, [1e-3, 1e-2, 1e-3, 1e-3], s)
            rho = 0.9 if s == 0 else pl(xs, [0.9, 0.8, 0.9, 0.9], s)
            for t in train:
                t.grad = None
            Lr, _ = ref.losses([x[perm[s * B:(s + 1) * B]] for x in data], float(tr.Wmean), float(tr.Hp), 1e-4, 1.0, 1.0)
            Lr.backward()
            assert abs(float(Lr.detach()) - ls[s]) < 3e-4 * max(1.0, abs(float(Lr.detach()))), (s, float(Lr.detach()), ls[s])
            with torch.no_grad():
                for t, v in zip(train, vel):
                    newdx = -rho * rho * v + (1 + rho) * lr * t.grad              # Optimisers.apply!(::Nesterov)
                    v.mul_(rho).sub_(lr * t.grad)
                    t.sub_(newdx)
        want = ref.blob()
        mask = np.array([not (nm.endswith(".mean") or nm.endswith(".var")) for nm, s in nn.param_layout() for _ in range(int(np.prod(s)))])
        print("max |dparam| %.3g" % np.abs(got[mask] - want[mask]).max())
        assert np.abs(got[mask] - want[mask]).max() < 3e-4, np.abs(got[mask] - want[mask]).max()


def test_training_lowers_the_loss_on_its_data():
    """fixed seed: 200 Tic-tac-toe games at 64 simulations, device memory with symmetries, 200 Adam steps at batch 128 with batch norm at
    momentum 0.1: L on the data set after training is below L before (no margin asserted)"""
    gspec = azhip.TicTacToeSpec()
    hp = SimpleNetHP(width=200, depth_common=6, use_batch_norm=True, batch_norm_momentum=0.1)
    nn = SimpleNet(gspec, hp, seed=1)
    with azhip.Engine(game=1, simplenet=hp, num_workers=100, batch_size=100, num_iters_per_turn=64, cpuct=1.0, dirichlet_noise_eps=0.2,
                      dirichlet_noise_alpha=1.0, temperature=((0,), (1.0,)), reset_every=4, seed=1, lock_step=1) as e:
        e.net_set_params(nn.params())
        games, moves, ng, nm, _ = e.selfplay_run(200)
    mem = azhip.MemoryBuffer(gspec, 100000)
    mem.push_records(games, moves, ng, nm, 1.0)
    lp = azhip.LearningParams(samples_weighing_policy=2, l2_regularization=1e-4, loss_computation_batch_size=2048, batch_size=128,
                              nonvalidity_penalty=1.0, optimiser=azhip.Adam(lr=1e-3))
    with azhip.Trainer(gspec, nn, mem, lp, use_symmetries=True) as tr:
        before = tr.learning_status().loss.L
        ls = tr.batch_updates(200, seed=1)
        tr.install_trained()
        after = tr.learning_status().loss.L
    print("L before %.6f after %.6f (first / last step losses %.4f / %.4f)" % (before, after, ls[0], ls[-1]))
    assert np.isfinite(ls).all() and after < before
    mem.close()


def test_tictactoe_experiment_example_runs_end_to_end():
    """examples/tictactoe_experiment.py at tiny sizes: self-play -> memory -> CyclicNesterov updates -> status -> arena -> both duels"""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("tictactoe_experiment", os.path.join(os.path.dirname(__file__), "..", "examples", "tictactoe_experiment.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.main(iters=2, games=64, sims=16, bench_games=8, max_batches=30, quiet=True)
    assert len(out) == 2
    for r in out:
        lr = r["learning"]
        assert len(lr.losses) == 30 and np.isfinite(lr.losses).all() and np.isfinite(lr.checkpoints[-1].status_after.loss.L)
        assert len(lr.checkpoints[-1].evaluation.rewards) == 100 and len(r["benchmark"]) == 2
        assert all(len(ev.rewards) == 8 and np.all(np.abs(ev.rewards) <= 1) for ev in r["benchmark"])
        assert len(r["memory"].per_game_stage) == 4
    assert out[1]["self_play"].memory_size > out[0]["self_play"].memory_size
