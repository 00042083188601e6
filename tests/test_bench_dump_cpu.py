"""bench.py's --dump-outputs on the CPU: the window of game ids is a function of the arguments alone, the records of its games are
picked out of az_selfplay_collect results whatever else they hold, and the arrays written are float32 / float64 that hold the
integers exactly (state keys as 32-bit words).  tests/test_bench_outputs_gpu.py runs the real thing twice and compares."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _records(ids, moves_per_game):
    from azhip._lib import GameRec, MoveRec
    games = (GameRec * len(ids))()
    moves = (MoveRec * (len(ids) * moves_per_game))()
    m = 0
    for i, gid in enumerate(ids):
        g = games[i]
        g.game_id, g.slot, g.num_moves, g.first_move, g.nodes = gid, 1000 + i, moves_per_game, m, 10 * gid
        g.total_simulations, g.total_nodes_traversed = 7, 8
        g.final_key[0], g.final_key[1] = (1 << 63) + gid, gid
        for k in range(moves_per_game):
            mv = moves[m]
            mv.key[0], mv.key[1] = (gid << 40) + k + 0xFFFFFFFF, (1 << 62) | k
            for a in range(10):
                mv.N[a] = gid + a + k
            mv.action, mv.reward = k % 7, 0.5 * k - 1
            m += 1
    return games, moves, len(ids), m


class _Engine:
    num_actions = 7

    def net_evaluate_keys(self, keys):
        keys = np.asarray(keys, dtype=np.uint64).reshape(-1, 2)
        P = np.tile(np.arange(7, dtype=np.float32), (len(keys), 1)) + (keys[:, :1] % np.uint64(5)).astype(np.float32)
        return P, (keys[:, 1] % np.uint64(3)).astype(np.float32)


def test_the_window_depends_on_the_arguments_alone():
    import bench
    a = bench.DumpWindow(0, 0, 400, 4096, 20, 5, False)
    b = bench.DumpWindow(0, 0, 400, 4096, 20, 5, False)
    assert (a.lo, a.hi) == (b.lo, b.hi) and a.hi - a.lo == bench.DUMP_GAMES
    # games that end about when the timed steps do: past the first generation, within the ids the warm-up hands out
    assert 4096 < a.lo < 4096 + int(bench.mixing_warmup(0, 400, bench.HEADLINE_WARMUP_GAME_LENGTHS) * 4096 / (400 * 23))
    assert bench.DumpWindow(1 << 24, 0, 400, 4096, 20, 5, False).lo == a.lo + (1 << 24)
    assert bench.DumpWindow(0, 0, 400, 4096, 2000, 5, False).lo > a.lo                   # more timed steps: later games


def test_the_window_keeps_its_own_games_and_writes_exact_float_arrays(tmp_path):
    import bench
    w = bench.DumpWindow(0, 0, 400, 512, 20, 5, False)
    w.lo, w.hi = 100, 104                                            # a small window for the test
    w.keep(_records([98, 101, 99, 103], 3))
    w.keep(_records([], 3))
    assert w.missing() == [100, 102] and w.missing(aborted={102}) == [100]
    w.keep(_records([100, 102, 104], 5))
    assert w.missing() == []
    info = w.write(_Engine(), str(tmp_path / "out"))
    assert info["games"] == 4 and info["positions"] == 5 + 3 + 5 + 3 and info["game_ids"] == [100, 104]
    d = {f[:-4]: np.load(tmp_path / "out" / f) for f in os.listdir(tmp_path / "out")}
    assert sorted(d) == sorted(f[:-4] for f in info["files"])
    assert all(a.dtype in (np.float32, np.float64) for a in d.values())
    assert sum(a.nbytes for a in d.values()) == info["bytes"] <= bench.DUMP_MAX_BYTES
    assert d["game_id"].tolist() == [100, 101, 102, 103] and d["game_num_moves"].tolist() == [5, 3, 5, 3]
    assert d["game_nodes"].tolist() == [1000, 1010, 1020, 1030]
    assert d["move_game_id"].tolist() == [100] * 5 + [101] * 3 + [102] * 5 + [103] * 3
    g, m = _records([100, 101, 102, 103], 1)[:2]
    fk = d["game_final_key"].astype(np.uint64)
    assert [int(fk[i, 0]) | int(fk[i, 1]) << 32 for i in range(4)] == [int(g[i].final_key[0]) for i in range(4)]
    mk = d["move_key"].astype(np.uint64)
    assert d["move_key"].shape == (16, 4) and int(mk[5, 0]) | int(mk[5, 1]) << 32 == (101 << 40) + 0 + 0xFFFFFFFF
    assert int(mk[5, 2]) | int(mk[5, 3]) << 32 == 1 << 62
    assert d["move_visits"].shape == (16, 10) and d["move_visits"][6].tolist() == [101 + a + 1 for a in range(10)]
    assert d["move_action"][:5].tolist() == [0, 1, 2, 3, 4] and d["move_reward"][:3].tolist() == [-1.0, -0.5, 0.0]
    assert d["move_policy"].shape == (16, 7) and d["move_value"].shape == (16,)


def test_help_names_the_full_and_dump_switches():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs" in r.stdout, r.stdout + r.stderr
