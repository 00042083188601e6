"""The reference's grid-world experiment (games/grid-world) through the device search trees of a host-stepped game in chance mode:
a one-player MDP whose play! is random, with search, replay memory, optimiser step and evaluation on the MI355X; the host keeps
the rules (azhip.GridWorldRules) and one env per simulation.

  world       9 x 9 with the reference's four reward cells, slip 0.4, on the 9 x 9 x 4-plane / 82-action geometry (Go9PlanesSpec):
              the position is plane 0, the four moves are the actions 0..3.  The shipped 10 x 10 world on a SimpleNet has no geometry
              here, so the network is an fp32 ResNet, not the one games/grid-world/params.jl names
  self-play   params.jl's MCTS: 50 simulations, cpuct 1, temperature 0 (the first of the most visited actions), no noise, MCTS.reset!
              every 16 episodes of a worker; HostTree(engine=..., chance=True) evaluates every state it is shown on the device
  learning    episodes -> PlaneMemoryBuffer.push_trace (rewards, gamma) -> Trainer on the plane memory: CONSTANT_WEIGHT, L2 1e-4,
              rewards_renormalization 10, nonvalidity penalty 1, Adam(5e-3)
  arena       the one-player compare_networks of src/training.jl:159-174: the mean total reward of the new network's episodes minus
              the old one's; the new network replaces the old one when that reaches update_threshold 0

One JSON line per iteration: mean return, loss before and after, seconds, and the steps a worker takes per simulation (one host
round trip per ply: its mean path length; once the 77 states of the world are known a simulation only ends on a reward cell or
at the time bound, so --max-moves bounds it).

    python examples/grid_world_host_stepped.py [--iters 3] [--workers 16] [--episodes 1] [--sims 50] [--max-moves 16] [--steps 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "alphazero.jl_amd"))
import azhip  # noqa: E402
from azhip import GridWorldRules, HostSteppedEnv, HostTree, PlaneMemoryBuffer  # noqa: E402

GAMMA, CPUCT, RESET_EVERY, UPDATE_THRESHOLD = 1.0, 1.0, 16, 0.0


def make_rules(gspec, seed, max_moves):
    """the 9 x 9 world; an episode ends after max_moves moves at the latest (time > episode_length_bound)"""
    return GridWorldRules(size=(9, 9), gspec=gspec, episode_length_bound=max_moves - 1, rng=np.random.Generator(np.random.Philox(seed)))


def start_state(rules):
    s = rules.init()
    while rules.terminal(s):
        s = rules.init()
    return s


def play_episodes(nn, rules, workers, episodes, sims, nodes_per_worker=128):
    """`episodes` episodes on each of `workers` workers, in lock step, searched by chance trees in engine mode on nn's engine.
    A 9 x 9 world has 77 states that are not terminal, so 128 nodes per worker never run out.
    -> (traces in finishing order: dicts of worker, states, actions, X, A, pi, rewards; the trees' counters)"""
    gspec = nn.gspec
    nA = gspec.num_actions()
    traces = []
    with HostTree(nA, workers, nodes_per_worker, edge_slots_per_worker=4 * nodes_per_worker, max_depth=rules.episode_length_bound + 2,
                  engine=nn.engine(), gamma=GAMMA, cpuct=CPUCT, chance=True) as tree:
        env = HostSteppedEnv(rules, tree)
        games = {w: start_state(rules) for w in range(workers)}
        cur = {w: dict(worker=w, states=[], actions=[], X=[], A=[], pi=[], rewards=[]) for w in range(workers)}
        done = {w: 0 for w in range(workers)}
        move = 0
        while games:
            ws = sorted(games)
            stopped = env.explore([games[w] for w in ws], sims, workers=ws, game_ids=ws, moves=[move] * len(ws))
            if stopped:
                raise RuntimeError("a worker's pools or max_depth were too small: %r" % (stopped,))
            N = tree.root_stats(ws)[0]
            acts = [int(np.argmax(N[i])) for i in range(len(ws))]          # temperature 0
            for i, w in enumerate(ws):
                t = cur[w]
                t["states"].append(games[w]); t["actions"].append(acts[i])
                t["X"].append(rules.planes(games[w])); t["A"].append(np.asarray(rules.mask(games[w]), np.float32))
                t["pi"].append(N[i] / N[i].sum())
            env.advance(ws, acts)
            finished = []
            for w in ws:
                games[w] = env.roots[w]
                cur[w]["rewards"].append(np.float32(rules.reward(games[w])))
                if rules.terminal(games[w]):
                    traces.append(cur[w])
                    done[w] += 1
                    if done[w] % RESET_EVERY == 0:
                        finished.append(w)
                    if done[w] < episodes:
                        games[w], cur[w] = start_state(rules), dict(worker=w, states=[], actions=[], X=[], A=[], pi=[], rewards=[])
                    else:
                        del games[w]
            if finished:
                env.reset(finished)
            move += 1
        stats = tree.stats()
    return traces, stats


def total_reward(trace, gamma=GAMMA):
    """trace.jl:45-47"""
    return float(sum(gamma ** i * float(r) for i, r in enumerate(trace["rewards"])))


def push_traces(memory, traces, gamma=GAMMA):
    for k, t in enumerate(traces):
        memory.push_trace(np.stack(t["X"]), np.stack(t["A"]), np.stack(t["pi"]), np.array(t["rewards"], np.float64), np.ones(len(t["X"]), bool),
                          gamma, game_id=k)


def learn(nn, memory, steps, batch_size, seed=1):
    """`steps` optimiser steps on the plane memory -> (the trained network, the step losses)"""
    lp = azhip.LearningParams(samples_weighing_policy=azhip.CONSTANT_WEIGHT, l2_regularization=1e-4, loss_computation_batch_size=2048,
                              batch_size=batch_size, use_position_averaging=False, rewards_renormalization=10.0, nonvalidity_penalty=1.0,
                              optimiser=azhip.Adam(lr=5e-3))
    with azhip.Trainer(nn.gspec, nn, memory, lp) as tr:
        losses = tr.batch_updates(steps, seed=seed)
        new = azhip.ResNet(nn.gspec, nn.hyper, params=tr.trained_params())
    return new, losses


def main(iters=3, workers=16, episodes=1, sims=50, max_moves=16, steps=20, batch_size=64, blocks=1, filters=64, seed=1, quiet=False):
    gspec = azhip.Go9PlanesSpec()
    hp = azhip.ResNetHP(num_blocks=blocks, num_filters=filters, num_policy_head_filters=32, num_value_head_filters=32)
    best = azhip.ResNet(gspec, hp, seed=seed)
    out = []
    with PlaneMemoryBuffer(gspec, 80_000) as memory:
        for it in range(iters):
            t0 = time.perf_counter()
            traces, st = play_episodes(best, make_rules(gspec, 1000 * seed + 3 * it, max_moves), workers, episodes, sims)
            memory.new_batch()
            push_traces(memory, traces)
            cur, losses = learn(best, memory, steps, batch_size, seed=seed + it)
            # compare_networks for a one-player game: both networks play their own episodes, on equal generator streams
            tc, _ = play_episodes(cur, make_rules(gspec, 1000 * seed + 3 * it + 1, max_moves), workers, 1, sims)
            tb, _ = play_episodes(best, make_rules(gspec, 1000 * seed + 3 * it + 1, max_moves), workers, 1, sims)
            avgr = float(np.mean([total_reward(t) for t in tc]) - np.mean([total_reward(t) for t in tb]))
            replaced = avgr >= UPDATE_THRESHOLD
            best.gc()
            if replaced:
                best = cur
            else:
                cur.gc()
            line = dict(iteration=it + 1, episodes=len(traces), samples=len(memory), mean_return=float(np.mean([total_reward(t) for t in traces])),
                        loss_before=float(losses[0]), loss_after=float(losses[-1]), arena_avgr=avgr, nn_replaced=bool(replaced),
                        seconds=time.perf_counter() - t0, steps_per_simulation=st["nodes_traversed"] / max(st["simulations"], 1),
                        tree_steps=st["steps"], evaluations=st["evaluations"], transposition_hits=st["transposition_hits"])
            if not quiet:
                print(json.dumps(line), flush=True)
            out.append(line)
    best.gc()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    for name, default in (("iters", 3), ("workers", 16), ("episodes", 1), ("sims", 50), ("max-moves", 16), ("steps", 20), ("batch-size", 64),
                          ("blocks", 1), ("filters", 64), ("seed", 1)):
        ap.add_argument("--" + name, type=int, default=default)
    a = ap.parse_args()
    main(a.iters, a.workers, a.episodes, a.sims, a.max_moves, a.steps, a.batch_size, a.blocks, a.filters, a.seed)
