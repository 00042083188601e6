"""Measurements of the SimpleNet engine (csrc/simplenet.h), written to profiles/simplenet/ as JSON.

  kernel     k_simplenet at 128, 1024 and 4096 Tic-tac-toe boards with the shipped hyperparameters (games/tictactoe/params.jl: width 200,
             depth_common 6, batch norm): HIP events through az_prof in the steady state (the same launch repeated after a warm-up, the
             weights L2-resident as they are between the waves of a search); beside the time the executed FLOP (padded tiles included)
             over the fp32 MFMA peak and the bytes of weights every workgroup streams.
  selfplay   a self-play phase with the shipped Tic-tac-toe parameters (400 simulations, cpuct 1, noise 0.2, reset_every 4) at 128 and at
             4096 workers: SimpleNet engine against the 5x64 ResNet engine on the same slots and simulations, in the same process:
             network time per wave (az_prof tower + heads) and simulations per second.
  train      milliseconds per optimiser step of the dense chain at batch 32 (CyclicNesterov) and at batch 1024 (Adam).
  experiment two iterations of examples/tictactoe_experiment.py as shipped: wall time of each and its two benchmark results.
--what kernel,selfplay,train,experiment picks; --out names the JSON file."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "alphazero.jl_amd"))
import azhip  # noqa: E402
from azhip.network import ResNetHP, SimpleNetHP, random_params, simple_param_layout, simple_random_params  # noqa: E402

PEAK_FP32_MFMA = 256 * 4 * 64 * 2.4e9          # FLOP/s: 256 CUs x 4 SIMDs x 64 FLOP per clock at 2.4 GHz
TTT = azhip.GAME_TICTACTOE
HP = SimpleNetHP(width=200, depth_common=6, use_batch_norm=True, batch_norm_momentum=1.0)

ap = argparse.ArgumentParser()
ap.add_argument("--what", default="kernel,selfplay,train,experiment")
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "simplenet", "bench.json"))
a = ap.parse_args()
out = {"library": os.environ.get("AZHIP_LIB", "libazhip.so")}


def pad(n, m):
    return -(-n // m) * m


def executed_flop_and_weight_bytes(game, hp):
    flop = frag = 0
    for name, shape in simple_param_layout(game, hp):
        if name.endswith(".W"):
            o, i = shape
            flop += 2 * pad(o, 16) * pad(i, 16)
            frag += pad(o, 16) * pad(i, 16)
    return flop, 4 * frag


def positions(n, seed=1):
    """n Tic-tac-toe keys reached by random play (repeats allowed: the network seam has no cache)"""
    rng = np.random.default_rng(seed)
    with azhip.Engine(game=TTT, oracle=azhip.ORACLE_UNIFORM, num_workers=1, batch_size=1, num_iters_per_turn=2) as e:
        keys = np.tile(np.array(e.init_key(), dtype=np.uint64), (n, 1))
        for _ in range(4):
            X, A = e.encode(keys)
            act = np.array([rng.choice(np.nonzero(m)[0]) if rng.random() < 0.7 else -1 for m in A], dtype=np.int32)
            nxt, term, _ = e.play(keys, act)
            keys = np.where(term[:, None], keys, nxt)
    return keys


if "kernel" in a.what:
    flop, wbytes = executed_flop_and_weight_bytes(TTT, HP)
    rows = []
    for n in (128, 1024, 4096):
        keys = positions(n)
        with azhip.Engine(game=TTT, simplenet=HP, num_workers=n, batch_size=n, num_iters_per_turn=2) as e:
            e.net_set_params(simple_random_params(TTT, HP, seed=1))
            X, A = e.encode(keys)
            for _ in range(20):
                e.net_forward(X, A)
            e.prof_enable(True, classes=["tower"])
            e.prof_reset()
            for _ in range(a.reps):
                e.net_forward(X, A)
            p = e.prof_get()["tower"]
            us = 1e3 * p["ms"] / p["launches"]
            rows.append(dict(boards=n, launches=p["launches"], us_per_launch=round(us, 2), executed_gflop=round(flop * pad(n, 16) / 1e9, 3),
                             share_of_fp32_mfma_peak=round(flop * pad(n, 16) / (us * 1e-6) / PEAK_FP32_MFMA, 4),
                             weight_bytes_per_workgroup=wbytes, workgroups=pad(n, 16) // 16, kernel=e.net_last_kernel()))
            print(rows[-1])
    out["kernel"] = rows

if "selfplay" in a.what:
    rhp = ResNetHP(num_blocks=5, num_filters=64, num_policy_head_filters=32, num_value_head_filters=32)
    rows = []
    for workers in (128, 4096):
        games = 2 * workers
        kw = dict(game=TTT, num_workers=workers, batch_size=workers, num_iters_per_turn=400, cpuct=1.0, dirichlet_noise_eps=0.2,
                  dirichlet_noise_alpha=1.0, temperature=((0,), (1.0,)), reset_every=4, seed=1)
        for name, mk, blob in (("SimpleNet 200x6", lambda: azhip.Engine(simplenet=HP, **kw), simple_random_params(TTT, HP, seed=1)),
                               ("ResNet 5x64", lambda: azhip.Engine(oracle=azhip.ORACLE_RESNET, num_blocks=5, num_filters=64, num_policy_head_filters=32,
                                                                    num_value_head_filters=32, **kw), random_params(TTT, rhp, seed=1))):
            with mk() as e:
                e.net_set_params(blob)
                e.selfplay_run(workers, device_only=True)               # warm-up phase
                t0 = time.perf_counter()
                _, _, ng, _, st = e.selfplay_run(games, first_game_id=workers, device_only=True)
                wall = time.perf_counter() - t0
                e.prof_enable(True, classes=["tower", "heads"])
                e.prof_reset()
                _, _, _, _, sp = e.selfplay_run(games, first_game_id=3 * workers, device_only=True)
                p = e.prof_get()
                net_ms = p["tower"]["ms"] + p["heads"]["ms"]
                rows.append(dict(network=name, workers=workers, games=int(ng), simulations=int(st.simulations), seconds=round(wall, 3),
                                 msims_per_s=round(st.simulations / wall / 1e6, 3), waves=int(st.waves), leaf_evals=int(st.leaf_evals),
                                 profiled_network_launches=p["tower"]["launches"], network_us_per_wave=round(1e3 * net_ms / max(1, p["tower"]["launches"]), 2),
                                 # what the launches of the PROFILED phase held: the leaves the trees consumed less those the evaluation cache answered, and the grid's upper bound
                                 profiled_leaf_evals=int(sp.leaf_evals), profiled_evals_reused=int(sp.evals_reused),
                                 boards_per_launch=round((sp.leaf_evals - sp.evals_reused) / max(1, p["tower"]["launches"]), 1),
                                 grid_bound_per_launch=round(p["tower"]["units"] / max(1, p["tower"]["launches"]), 1), kernel=e.net_last_kernel()))
                print(rows[-1])
    out["selfplay"] = rows

if "train" in a.what:
    # the optimiser step of the dense chain (train.hip): wall time of 200 steps enqueued back to back / 200, after a warm-up call
    gspec = azhip.TicTacToeSpec()
    nn = azhip.SimpleNet(gspec, HP, seed=1)
    with azhip.Engine(game=TTT, simplenet=HP, num_workers=128, batch_size=128, num_iters_per_turn=64, cpuct=1.0, dirichlet_noise_eps=0.2,
                      temperature=((0,), (1.0,)), reset_every=4, seed=1) as e:
        e.net_set_params(nn.params())
        games, moves, ng, nm, _ = e.selfplay_run(400)
    mem = azhip.MemoryBuffer(gspec, 80_000)
    mem.push_records(games, moves, ng, nm, 1.0)
    rows = []
    for batch, opt in ((32, azhip.CyclicNesterov(lr_base=1e-3, lr_high=1e-2, lr_low=1e-3, momentum_high=0.9, momentum_low=0.8)), (1024, azhip.Adam(lr=1e-3))):
        lp = azhip.LearningParams(samples_weighing_policy=azhip.LOG_WEIGHT, l2_regularization=1e-4, batch_size=batch, loss_computation_batch_size=2048, optimiser=opt)
        with azhip.Trainer(gspec, nn, mem, lp, use_symmetries=True) as tr:
            tr.batch_updates(20)
            t0 = time.perf_counter()
            tr.batch_updates(200)
            dt = time.perf_counter() - t0
            rows.append(dict(batch=tr.batch_size(), samples=tr.num_samples(), optimiser=type(opt).__name__, ms_per_step=round(1e3 * dt / 200, 4)))
            print(rows[-1])
    mem.close()
    out["train"] = rows

if "experiment" in a.what:
    # one whole shipped iteration of examples/tictactoe_experiment.py and its two benchmark duels
    import importlib.util
    spec = importlib.util.spec_from_file_location("tictactoe_experiment", os.path.join(ROOT, "examples", "tictactoe_experiment.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    rows = []
    for k, r in enumerate(mod.main(iters=2)):
        ck = r["learning"].checkpoints[-1]
        rows.append(dict(iteration=k + 1, seconds_self_play_and_learning=round(r["seconds"], 2), samples_in_memory=int(r["self_play"].memory_size),
                         batch_updates=int(len(r["learning"].losses)), status_L_before=float(r["learning"].initial_status.loss.L),
                         status_L_after=float(ck.status_after.loss.L), arena_avg_reward=float(ck.evaluation.avgr), nn_replaced=bool(ck.nn_replaced),
                         benchmark=[dict(duel=ev.legend, avg_reward=round(float(ev.avgr), 4), seconds=round(ev.time, 2)) for ev in r["benchmark"]]))
    out["experiment"] = rows

os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(out, f, indent=1)
print(json.dumps(out))
