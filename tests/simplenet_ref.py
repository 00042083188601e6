"""What the SimpleNet GPU tests share: a float64 NumPy restatement of NetLib.SimpleNet in test mode (simplenet.jl:37-64) followed by
Network.forward_normalized (network.jl:264-271), written from the Flux model over azhip.network.simple_param_layout's names -- not from
csrc/ -- and a few non-terminal positions per game."""
import numpy as np

import azref as R
from azhip.network import SimpleNetHP, simple_param_layout

TOL = 1e-5          # the project's network contract: fp32 outputs within 1e-5 of a float64 restatement
EPS32 = float(np.finfo(np.float32).eps)
TTT_SHIPPED = SimpleNetHP(width=200, depth_common=6, use_batch_norm=True, batch_norm_momentum=1.0)   # games/tictactoe/params.jl
GRID_WORLD_LIKE = SimpleNetHP(width=100, depth_common=4, use_batch_norm=False)                        # games/grid-world/params.jl


def split(game, hp, blob):
    out, off = {}, 0
    for name, shape in simple_param_layout(game, hp):
        n = int(np.prod(shape))
        out[name] = np.asarray(blob[off:off + n], dtype=np.float64).reshape(shape, order="F")
        off += n
    assert off == len(blob)
    return out


def forward64(game, hp, blob, X, A):
    """P (masked, normalised), V, Pinv in float64"""
    p = split(game, hp, blob)
    x = np.asarray(X, dtype=np.float64).reshape(len(X), -1)          # flatten of W x H x C = its memory order

    def D(x, pre):
        z = x @ p[pre + ".dense.W"].T + p[pre + ".dense.b"]
        if hp.use_batch_norm:
            z = p[pre + ".bn.gamma"] * (z - p[pre + ".bn.mean"]) / np.sqrt(p[pre + ".bn.var"] + 1e-5) + p[pre + ".bn.beta"]
        return np.maximum(z, 0.0)

    x = D(x, "common0")
    for l in range(hp.depth_common):
        x = D(x, "common%d" % (l + 1))
    y = x
    for l in range(hp.depth_phead):
        y = D(y, "phead%d" % l)
    logits = y @ p["phead.out.W"].T + p["phead.out.b"]
    e = np.exp(logits - logits.max(axis=1, keepdims=True))
    pol = e / e.sum(axis=1, keepdims=True)
    v = x
    for l in range(hp.depth_vhead):
        v = D(v, "vhead%d" % l)
    val = np.tanh(v @ p["vhead.out.W"].T + p["vhead.out.b"]).reshape(-1)
    pm = pol * np.asarray(A, dtype=np.float64)
    sp = pm.sum(axis=1, keepdims=True)
    return pm / (sp + EPS32), val, (1.0 - sp).reshape(-1)


def random_positions(game, n, seed):
    """n distinct-ish non-terminal positions reached by random play"""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        g = R.Game(game)
        for _ in range(int(rng.integers(0, 30))):
            if g.terminated():
                break
            g.play(int(rng.choice(g.available_actions())))
        if not g.terminated():
            out.append(g)
    return out


def batch_of(game, envs):
    w, h, c = R.DIMS[game]
    X = np.stack([g.vectorize().reshape(c, h, w) for g in envs])
    A = np.stack([g.actions_mask().astype(np.float32) for g in envs])
    return X, A


def keys_of(envs):
    return np.array([g.key() for g in envs], dtype=np.uint64)
