"""Time the device replay-memory path at scale: push_trace! of a self-play phase, the Trainer's data set
(symmetries + merge_by_state + convert_samples) and learning_status (5x64 ResNet, test mode).

--planes: the replay memory of a host-stepped game instead (azhip.PlaneMemoryBuffer, 9x9x4 Go geometry, about 30 % repeated
positions): az_dataset_create_from_plane_memory (merged, LOG_WEIGHT) against what a host without it does for the same samples -- a
numpy merge_by_state + convert_samples, then az_dataset_create_from_tensors with its upload -- in the same run; --out writes both as JSON.

--planes --symmetries: the same samples with the 7 dihedral symmetries declared (azhip.plane_symmetries, set_symmetries): the merged
LOG_WEIGHT build over the 8 x samples virtual rows, against what a host without declared symmetries does for the same data set -- gather
the images with numpy, push all 8 x samples into a memory of 8 x the capacity (upload included), run the build without symmetries."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "alphazero.jl_amd"))
import azhip  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--games", type=int, default=16384)
ap.add_argument("--filters", type=int, default=64)
ap.add_argument("--planes", action="store_true")
ap.add_argument("--symmetries", action="store_true")
ap.add_argument("--samples", type=int, default=1 << 20)
ap.add_argument("--out", default=None)
a = ap.parse_args()


def host_merge_convert(X, A, P, z, nv):
    """what a host does today: merge_by_state over the (X, A) rows and convert_samples (LOG_WEIGHT), vectorised numpy.  Rows are
    grouped by a 64-bit multiply-add hash and the grouping is verified word by word; sums run in buffer order (np.add.at)."""
    import numpy as np
    n = len(z)
    rows = np.concatenate([X.reshape(n, -1), A], axis=1).view(np.uint32)
    mult = np.random.default_rng(0).integers(1, 1 << 63, rows.shape[1], dtype=np.uint64) | np.uint64(1)
    h = np.concatenate([(rows[k:k + 65536].astype(np.uint64) * mult).sum(axis=1, dtype=np.uint64) for k in range(0, n, 65536)])
    _, first, inv = np.unique(h, return_index=True, return_inverse=True)
    assert np.array_equal(rows, rows[first][inv]), "hash collision"
    order = np.argsort(first, kind="stable")                                  # groups in order of first occurrence
    rank = np.empty_like(order)
    rank[order] = np.arange(len(order))
    g = rank[inv]
    cnt = np.bincount(g, minlength=len(order)).astype(np.float64)
    pi = np.zeros((len(order), P.shape[1]))
    zs = np.zeros(len(order))
    ns = np.zeros(len(order), dtype=np.int64)
    np.add.at(pi, g, P)
    np.add.at(zs, g, z)
    np.add.at(ns, g, nv)
    f = first[order]
    W = (np.log2(ns.astype(np.float64)) + 1.0).astype(np.float32)
    return W, X[f], A[f], (pi / cnt[:, None]).astype(np.float32), (zs / cnt).astype(np.float32)


def plane_samples(n):
    import numpy as np
    rng = np.random.default_rng(1)
    X = rng.integers(0, 2, size=(n, 4, 9, 9), dtype=np.uint8).astype(np.float32)
    A = (rng.random((n, 82), dtype=np.float32) < 0.6).astype(np.float32)
    A[:, 81] = 1.0
    dup = rng.permutation(n)[:int(0.3 * n)]                                   # these samples repeat an earlier (or later) position
    src = rng.integers(0, n, len(dup))
    X[dup], A[dup] = X[src], A[src]
    P = rng.random((n, 82)) * A
    P /= P.sum(axis=1, keepdims=True)
    z, t, nv = rng.uniform(-1, 1, n), rng.integers(1, 80, n).astype(np.float64), np.ones(n, dtype=np.int64)
    return X, A, P, z, t, nv


def write_result(res):
    import json
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


def timed_builds(mem, repeats, **kw):
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        d = mem.dataset(use_position_averaging=True, weighing_policy=azhip.LOG_WEIGHT, **kw)
        ms.append(round(1e3 * (time.perf_counter() - t0), 2))
        info = (len(d), d.sum_n, d.Wtot, d.Hp)
        d.close()
    return ms, info


def memory_bytes(gspec, capacity):
    """HBM of a plane memory's ring: per sample the (X, A) row in Float32, pi / z / t in Float64 and n"""
    w, h, c = gspec.state_dim()
    nA = gspec.num_actions()
    return capacity * (4 * (w * h * c + nA) + 8 * (nA + 2) + 8)


def symmetries_bench():
    import numpy as np
    gspec = azhip.Go9PlanesSpec()
    n = a.samples
    X, A, P, z, t, nv = plane_samples(n)
    xperm, aperm = azhip.plane_symmetries(gspec)
    nsym = len(xperm)
    # declared: n samples, the images are read through the tables
    mem = azhip.PlaneMemoryBuffer(gspec, n)
    mem.set_symmetries(xperm, aperm)
    t0 = time.perf_counter()
    mem.push_samples(X, A, P, z, t, nv)
    push_ms = 1e3 * (time.perf_counter() - t0)
    plain_ms, _ = timed_builds(mem, 4)
    sym_ms, info = timed_builds(mem, 5, use_symmetries=True)
    mem.close()
    # pushed: the host gathers the images (chunks of samples, so the host never holds all 8 n rows) and pushes them in the order
    # n + i * nsym + k into a memory of (1 + nsym) n samples
    big = azhip.PlaneMemoryBuffer(gspec, n * (1 + nsym))
    t0 = time.perf_counter()
    big.push_samples(X, A, P, z, t, nv)
    big_push_ms, gather_ms = 1e3 * (time.perf_counter() - t0), 0.0
    chunk = 1 << 16
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        t0 = time.perf_counter()
        m = hi - lo
        Xi = X[lo:hi].reshape(m, -1)[:, xperm].reshape(m * nsym, 4, 9, 9)
        Ai, Pi = A[lo:hi][:, aperm].reshape(m * nsym, -1), P[lo:hi][:, aperm].reshape(m * nsym, -1)
        zi, ti, ni = np.repeat(z[lo:hi], nsym), np.repeat(t[lo:hi], nsym), np.repeat(nv[lo:hi], nsym)
        t1 = time.perf_counter()
        big.push_samples(Xi, Ai, Pi, zi, ti, ni)
        t2 = time.perf_counter()
        gather_ms += 1e3 * (t1 - t0)
        big_push_ms += 1e3 * (t2 - t1)
    big_ms, big_info = timed_builds(big, 5)
    big.close()
    assert info == big_info, (info, big_info)                                   # the same rows in the same order: the same sums exactly
    write_result({"samples": n, "symmetries": nsym, "virtual_rows": n * (1 + nsym), "merged_rows": info[0], "sum_n": info[1],
                  "geometry": "9x9x4, 82 actions", "weighing_policy": "LOG_WEIGHT",
                  "declared_push_samples_ms_incl_upload": round(push_ms, 1), "declared_memory_bytes": memory_bytes(gspec, n),
                  "declared_build_ms": sym_ms, "declared_build_ms_best_after_first": min(sym_ms[1:]),
                  "same_memory_build_without_symmetries_ms": plain_ms,
                  "pushed_host_numpy_gather_ms": round(gather_ms, 1), "pushed_push_samples_ms_incl_upload": round(big_push_ms, 1),
                  "pushed_memory_bytes": memory_bytes(gspec, n * (1 + nsym)),
                  "pushed_build_ms": big_ms, "pushed_build_ms_best_after_first": min(big_ms[1:]),
                  "pushed_build_ms_spread_after_first": round(max(big_ms[1:]) - min(big_ms[1:]), 2)})


def planes_bench():
    import numpy as np
    gspec = azhip.Go9PlanesSpec()
    n = a.samples
    X, A, P, z, t, nv = plane_samples(n)
    mem = azhip.PlaneMemoryBuffer(gspec, n)
    t0 = time.perf_counter()
    mem.push_samples(X, A, P, z, t, nv)
    push_ms = 1e3 * (time.perf_counter() - t0)
    dev_ms = []
    for _ in range(4):
        t0 = time.perf_counter()
        d = mem.dataset(use_position_averaging=True, weighing_policy=azhip.LOG_WEIGHT)
        dev_ms.append(1e3 * (time.perf_counter() - t0))
        rows, info = len(d), (d.sum_n, d.Wtot, d.Hp)
        d.close()
    host = []
    for _ in range(2):
        t0 = time.perf_counter()
        tensors = host_merge_convert(X, A, P, z, nv)
        t1 = time.perf_counter()
        td = azhip.TensorDataset(gspec, *tensors)
        t2 = time.perf_counter()
        host.append((1e3 * (t1 - t0), 1e3 * (t2 - t1)))
        assert len(td) == rows and td.sum_n == rows and abs(td.Wtot - info[1]) <= 1e-6 * info[1], (len(td), rows, td.Wtot, info)
        td.close()
    res = {"samples": n, "merged_rows": rows, "geometry": "9x9x4, 82 actions", "weighing_policy": "LOG_WEIGHT",
           "device_dataset_build_ms": [round(x, 2) for x in dev_ms], "device_dataset_build_ms_best_after_first": round(min(dev_ms[1:]), 2),
           "push_samples_ms_incl_upload": round(push_ms, 1),
           "host_numpy_merge_convert_ms": [round(h[0], 1) for h in host], "host_create_from_tensors_ms_incl_upload": [round(h[1], 1) for h in host],
           "host_path_ms_best": round(min(h[0] + h[1] for h in host), 1)}
    write_result(res)


if a.symmetries and not a.planes:
    ap.error("--symmetries is a mode of --planes")
if a.planes:
    symmetries_bench() if a.symmetries else planes_bench()
    sys.exit(0)
gspec = azhip.ConnectFourSpec()
with azhip.Engine(game=0, oracle=azhip.ORACLE_HASH, num_workers=4096, batch_size=4096, num_iters_per_turn=8, reset_every=1,
                  dirichlet_noise_eps=0.25, cpuct=1.0, temperature=([0], [1.0])) as e:
    t0 = time.perf_counter()
    games, moves, ng, nm, stats = e.selfplay_run(a.games)
    print("generated %d games, %d positions in %.2f s (hash oracle, 8 sims/move)" % (ng, nm, time.perf_counter() - t0))
mem = azhip.MemoryBuffer(gspec, 4 * nm)
t0 = time.perf_counter()
mem.push_records(games, moves, ng, nm, 1.0)
t1 = time.perf_counter()
print("push_trace!: %d samples in %.1f ms = %.1f M samples/s (incl. the 64 B/sample H2D copy)" % (nm, 1e3 * (t1 - t0), nm / (t1 - t0) / 1e6))
for _ in range(2):
    t0 = time.perf_counter()
    d = mem.dataset(use_symmetries=True, use_position_averaging=True, weighing_policy=azhip.LOG_WEIGHT)
    t1 = time.perf_counter()
    print("data set: %d samples -> x2 symmetries -> %d merged boards (+ W,X,A,P,V tensors) in %.1f ms = %.1f M input samples/s"
          % (nm, len(d), 1e3 * (t1 - t0), nm / (t1 - t0) / 1e6))
    d.close()
hp = azhip.ResNetHP(num_blocks=5, num_filters=a.filters, num_policy_head_filters=32, num_value_head_filters=32)
nn = azhip.ResNet(gspec, hp, seed=1)
lp = azhip.LearningParams(samples_weighing_policy=azhip.LOG_WEIGHT, l2_regularization=1e-4, loss_computation_batch_size=1024)
with azhip.Trainer(gspec, nn, mem, lp, use_symmetries=True) as tr:
    tr.learning_status()
    t0 = time.perf_counter()
    st = tr.learning_status()
    t1 = time.perf_counter()
    print("learning_status: %d boards, 5x%d net, batches of 1024: %.1f ms = %.2f M boards/s   L=%.4f Lp=%.4f Lv=%.4f Hp=%.4f"
          % (tr.num_samples(), a.filters, 1e3 * (t1 - t0), tr.num_samples() / (t1 - t0) / 1e6, st.loss.L, st.loss.Lp, st.loss.Lv, st.Hp))
