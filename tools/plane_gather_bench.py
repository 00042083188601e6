"""Measurement: az_comm_gather_push_planes on one rank against what a host had to do before it existed.

Go geometry, a batch of 2^17 samples in games of 128 positions, an outbox of capacity 2^18, a destination of capacity 2^20.  After a
warm-up call, five times alternately:
  device   Comm.gather_push_planes(src, dst): gather_ms / total_ms from az_gather_stats, the HIP-event time of k_pg_pack and
           k_pg_scatter (az_debug_comm_plane_kernel_ms) and the bytes they move (each reads and writes one 2304-byte row per sample)
           as a share of the HBM peak;
  host     src.samples() followed by dst.push_samples(...) in the same process: the only route without the call (two PCIe crossings,
           and it does not even order the samples by game id).
Prints one JSON line; --out writes it to a file (profiles/plane_gather/bench.json).  The all-gather over xGMI with more than one rank
cannot be measured on one GPU: nothing here estimates it."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "alphazero.jl_amd"))
import azhip  # noqa: E402
from azhip import comm  # noqa: E402
from azhip._lib import check, lib  # noqa: E402

HBM_PEAK_TBS = 8.0            # MI355X HBM3E, specification; a float4 copy reaches about 6.3 TB/s of it

ap = argparse.ArgumentParser()
ap.add_argument("--log2-batch", type=int, default=17)
ap.add_argument("--game-len", type=int, default=128)
ap.add_argument("--log2-src", type=int, default=18)
ap.add_argument("--log2-dst", type=int, default=20)
ap.add_argument("--calls", type=int, default=5)
ap.add_argument("--out", default=None)
a = ap.parse_args()

gspec = azhip.Go9PlanesSpec()
nA, B, glen = gspec.num_actions(), 1 << a.log2_batch, a.game_len
w, h, c = gspec.state_dim()
rng = np.random.default_rng(5)
X = rng.integers(0, 2, size=(B, c, h, w)).astype(np.float32)
A = (rng.random((B, nA)) < 0.6).astype(np.float32)
A[np.arange(B), rng.integers(0, nA, B)] = 1.0
P = rng.random((B, nA)) * A
P /= P.sum(axis=1, keepdims=True)
rewards, white = rng.integers(-1, 2, B).astype(np.float64), rng.integers(0, 2, B).astype(np.uint8)

src, dst = azhip.PlaneMemoryBuffer(gspec, 1 << a.log2_src), azhip.PlaneMemoryBuffer(gspec, 1 << a.log2_dst)
ids = rng.permutation(B // glen)                                     # games are pushed in no particular order of id
for k, gid in enumerate(ids):
    sl = slice(k * glen, (k + 1) * glen)
    src.push_trace(X[sl], A[sl], P[sl], rewards[sl], white[sl], 1.0, game_id=int(gid))

kernel_ms = lib().az_debug_comm_plane_kernel_ms
kernel_ms.argtypes, kernel_ms.restype = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)], C.c_int
row_bytes = 4 * (c * h * w + nA) + 8 * (nA + 2) + 8                  # what a kernel reads per sample; it writes as much
dev, host = [], []
with comm.Comm(0, 0, 1, comm.unique_id()) as cm:
    cm.gather_push_planes(src, dst)                                   # warm-up
    for _ in range(a.calls):
        st = cm.gather_push_planes(src, dst)
        pk, sc = C.c_double(), C.c_double()
        check(kernel_ms(cm._h, C.byref(pk), C.byref(sc)))
        dev.append({"gather_ms": st.gather_ms, "total_ms": st.total_ms, "pack_ms": pk.value, "scatter_ms": sc.value, "bytes": st.bytes})
        t0 = time.perf_counter()
        s = src.samples()
        t1 = time.perf_counter()
        dst.push_samples(*s)
        t2 = time.perf_counter()
        host.append({"read_ms": 1e3 * (t1 - t0), "push_ms": 1e3 * (t2 - t1), "total_ms": 1e3 * (t2 - t0)})
assert len(s[3]) == B


def stat(rows, key):
    v = np.array([r[key] for r in rows])
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max())}


moved = 2.0 * row_bytes * B
out = {
    "what": "az_comm_gather_push_planes, 1 rank", "geometry": "go9", "samples": B, "game_len": glen, "record_bytes": row_bytes,
    "src_capacity": 1 << a.log2_src, "dst_capacity": 1 << a.log2_dst, "calls": a.calls,
    "device": {k: stat(dev, k) for k in ("gather_ms", "total_ms", "pack_ms", "scatter_ms")},
    "host": {k: stat(host, k) for k in ("read_ms", "push_ms", "total_ms")},
    "bytes_received_per_call": dev[0]["bytes"],
    "hbm_peak_TBs": HBM_PEAK_TBS,
}
for name in ("pack", "scatter"):
    ms = out["device"][name + "_ms"]["median"]
    out[name + "_TBs"] = moved / (ms * 1e-3) / 1e12
    out[name + "_share_of_hbm_peak"] = out[name + "_TBs"] / HBM_PEAK_TBS
out["host_over_device_total"] = out["host"]["total_ms"]["median"] / out["device"]["total_ms"]["median"]
line = json.dumps(out)
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
