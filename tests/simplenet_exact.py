"""Exact SimpleNets for tests/test_simplenet_net_gpu.py: networks whose every pre-activation is a small integer (a dyadic rational after
the heads' last hidden layers), so that fp32 computes it without rounding in ANY order of summation and the device may differ from
float64 only in its softmax and tanh -- while a weight that sits one index off changes an output by far more than the tolerance.

  inputs       the games' 0 / 1 planes
  weights      in {-1, 0, 1}, at most two non-zeros per row of the k-major matrix (= per column of Flux's W(o, i)): input unit k of a layer
               feeds the output units s1(k) and s2(k) of two pseudo-random permutations (one of them when the layer narrows)
  batch norm   gamma a power of two (1 in the hidden layers, 2^-g in each head's last hidden layer, g chosen so that the logits / the
               value's pre-activation span about [-2, 2] on the calibration boards), var such that sqrtf(var + 1e-5f) is exactly 1, beta 0,
               bias 0, the running mean an integer: the folded scale is gamma exactly and the shift an integer multiple of it
  calibration  on a fixed set of boards every hidden unit's running mean is (the least value it sums) - 1: the unit passes at least 1 on
               every board, the network is affine in the planes there and no weight's effect is cut off by a ReLU; the biases of the two
               final layers centre their outputs (multiples of the last gamma)
  signatures   the gain of a unit is the integer vector of its path sums to the nine logits and the value; a weight moved from output
               unit o to o + 1 changes the outputs by (its input) x (gain[o + 1] - gain[o]), so the second permutation of each layer is
               redrawn per unit until neighbouring units of the layer below have different gains
exact_params returns (blob, [(offset, size) of every dense matrix]); moved_weights lists, for every non-zero weight, the blob with that
weight moved to the neighbouring index of its matrix."""
import numpy as np

from azhip.network import simple_param_layout


def unit_var():
    """v with float32(v + float32(1e-5)) == 1 exactly"""
    e = np.float32(1e-5)
    v = np.float32(1.0) - e
    for _ in range(8):
        s = np.float32(v + e)
        if s == np.float32(1.0):
            return v
        v = np.nextafter(v, np.float32(2.0) if s < 1 else np.float32(0.0), dtype=np.float32)
    raise AssertionError("no such variance")


def _matrix(rng, o, i, gain_out):
    """W (o, i): column k has +-1 at s1(k) and s2(k); gain_out (o, J): the gains of this layer's OUTPUT units.  The gains of the input
    units, W.T @ gain_out, differ between neighbours k, k + 1."""
    W = np.zeros((o, i))
    s1 = np.concatenate([rng.permutation(o) for _ in range(-(-i // o))])[:i]
    gin = np.zeros((i, gain_out.shape[1]))
    for k in range(i):
        for _ in range(200):
            col = np.zeros(o)
            col[s1[k]] = rng.choice((-1.0, 1.0))
            if o > 1:
                t = rng.integers(o - 1)
                col[t + (t >= s1[k])] = rng.choice((-1.0, 1.0))
            g = col @ gain_out
            if g.any() and (k == 0 or not np.array_equal(g, gin[k - 1])):
                break
        else:
            raise AssertionError("no column with a gain of its own")
        W[:, k], gin[k] = col, g
    return W, gin


def exact_params(game, hp, seed, Xcal):
    """Xcal: the calibration boards (N, C, H, W)"""
    assert hp.use_batch_norm and hp.depth_phead >= 1 and hp.depth_vhead >= 1
    rng = np.random.default_rng(seed)
    lay = simple_param_layout(game, hp)
    shapes = {n: s for n, s in lay}
    A, h = shapes["phead.out.W"][0], hp.width
    J = A + 1                                                         # gains: to the A logits, then to the value
    # ---- matrices, from the outputs back to the planes, so that every layer knows the gains of the units it feeds
    Wm = {}
    Wm["phead.out"], gp = _matrix(rng, A, h, np.eye(A, J))
    Wm["vhead.out"], gv = _matrix(rng, 1, h, np.eye(1, J, k=A))
    for l in reversed(range(hp.depth_phead)):
        Wm["phead%d" % l], gp = _matrix(rng, h, h, gp)
    for l in reversed(range(hp.depth_vhead)):
        Wm["vhead%d" % l], gv = _matrix(rng, h, h, gv)
    g = gp + gv                                                       # the trunk's last units feed both heads
    for l in reversed(range(hp.depth_common + 1)):
        Wm["common%d" % l], g = _matrix(rng, h, shapes["common%d.dense.W" % l][1], g)
    # ---- forward over the calibration boards: running means, the heads' last gammas, the final biases
    x = np.asarray(Xcal, dtype=np.float64).reshape(len(Xcal), -1)
    val = {}

    def hidden(x, pre, gamma):
        z = x @ Wm[pre].T
        mu = z.min(axis=0) - 1.0
        val[pre] = (gamma, mu)
        return gamma * (z - mu)

    def head(x, name, depth):
        for l in range(depth - 1):
            x = hidden(x, "%s%d" % (name, l), 1.0)
        pre = "%s%d" % (name, depth - 1)
        z = x @ Wm[pre].T
        raw = (z - (z.min(axis=0) - 1.0)) @ Wm[name + ".out"].T
        spread = max(np.abs(raw - np.median(raw, axis=0)).max(), 1.0)
        gamma = 2.0 ** -int(np.ceil(np.log2(spread / 2.0))) if spread > 2.0 else 1.0
        out = hidden(x, pre, gamma) @ Wm[name + ".out"].T
        val[name + ".out"] = -gamma * np.round(np.median(out, axis=0) / gamma)
    for l in range(hp.depth_common + 1):
        x = hidden(x, "common%d" % l, 1.0)
    head(x, "phead", hp.depth_phead)
    head(x, "vhead", hp.depth_vhead)
    # ---- the blob
    parts, mats, off = [], [], 0
    for name, shape in lay:
        n = int(np.prod(shape))
        pre = name[:-2] if name.endswith((".W", ".b")) else name.rsplit(".", 2)[0]
        pre = pre[:-6] if pre.endswith(".dense") else pre
        if name.endswith(".W"):
            parts.append(Wm[pre].ravel(order="F"))
            mats.append((off, n))
        elif name.endswith(".b"):
            parts.append(val[pre] if ".out." in name else np.zeros(n))
        elif name.endswith(".gamma"):
            parts.append(np.full(n, val[pre][0]))
        elif name.endswith(".beta"):
            parts.append(np.zeros(n))
        elif name.endswith(".mean"):
            parts.append(val[pre][1])
        else:
            parts.append(np.full(n, unit_var(), dtype=np.float64))
        off += n
    blob = np.concatenate(parts)
    assert np.array_equal(blob.astype(np.float32).astype(np.float64), blob)
    return blob.astype(np.float32), mats


def moved_weights(blob, mats):
    """for every non-zero weight: (index, blob with it moved to the next index of its matrix -- the previous one at the matrix's end)"""
    for off, n in mats:
        for idx in np.nonzero(blob[off:off + n])[0] + off:
            nb = idx + 1 if idx + 1 < off + n else idx - 1
            if nb < off:
                continue                                              # a 1 x 1 matrix has no neighbour
            m = blob.copy()
            m[nb], m[idx] = blob[idx], 0.0
            yield int(idx), m
