"""The host side of the Pons benchmark (azhip/pons.py) without a GPU: the shipped data files, the file-name rule and the order of
games/connect-four/scripts/pons_benchmark.jl:31-75, optimal_on (101-107) and state_of_string (92-99) against the oracle's game."""
import os

import numpy as np
import pytest

import azref as R
from azhip import pons as Pons

PONS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pons")


def test_load_benchmarks_reads_the_six_sets_in_the_reference_order():
    bs = Pons.load_benchmarks(PONS)
    assert [(b.stage, b.difficulty) for b in bs] == [("beginning", "easy"), ("middle", "easy"), ("end", "easy"),
                                                     ("beginning", "medium"), ("middle", "medium"), ("beginning", "hard")]
    assert Pons.STAGES == ["beginning", "middle", "end"] and Pons.DIFFICULTIES == ["easy", "medium", "hard"]
    for b in bs:
        assert len(b.entries) == 1000
        lo, hi = {"beginning": (0, 14), "middle": (15, 28), "end": (29, 41)}[b.stage]
        assert all(lo <= len(s) <= hi and set(s) <= set("1234567") and -21 <= sc <= 21 for s, sc in b.entries), (b.stage, b.difficulty)
    first = open(os.path.join(PONS, "Test_L3_R1")).readline().split()
    assert bs[2].entries[0] == (first[0], int(first[1]))
    scores = [l.split() for l in open(os.path.join(PONS, "..", "c4_scores.txt"))]     # the 1300 the rules test already holds are these files' entries
    by_set = {(b.stage, b.difficulty): dict(b.entries) for b in bs}
    names = {"Test_L%d_R%d" % (i + 1, j + 1): (st, df) for i, st in enumerate(Pons.STAGES) for j, df in enumerate(Pons.DIFFICULTIES)}
    assert all(by_set[names[n]][s] == int(sc) for n, s, sc in scores)


def test_file_name_rule(tmp_path):
    assert Pons.parse_test_filename("Test_L1_R3") == ("beginning", "hard") and Pons.parse_test_filename("Test_L3_R1") == ("end", "easy")
    for bad in ("Test_L1_R3.txt", "test_L1_R3", "Test_L4_R1", "Test_L0_R1", "Test_L1_R", "README.md", "xTest_L1_R1"):
        assert Pons.parse_test_filename(bad) is None, bad
    (tmp_path / "Test_L2_R2").write_text("4455 3\n\n121212 -2\n")
    (tmp_path / "Test_L1_R1").write_text("4 1\n")
    (tmp_path / "README").write_text("not a set\n")
    (tmp_path / "Test_L3_R3").mkdir()                                 # a directory with a set's name is no set
    bs = Pons.load_benchmarks(str(tmp_path))
    assert [(b.stage, b.difficulty, b.entries) for b in bs] == [("beginning", "easy", [("4", 1)]), ("middle", "medium", [("4455", 3), ("121212", -2)])]
    with pytest.raises(FileNotFoundError):
        Pons.load_benchmarks(str(tmp_path / "nowhere"))


def test_optimal_on():
    assert all(Pons.optimal_on([-3, -1, -7], k) for k in range(3))                  # every move loses: every move is optimal
    assert [Pons.optimal_on([-2, 0, -5, 0], k) for k in range(4)] == [False, True, False, True]     # a draw among losses
    assert [Pons.optimal_on([4, 1, 0, -2], k) for k in range(4)] == [True, True, False, False]      # any win is optimal, however slow
    assert Pons.optimal_on([0], 0) and Pons.optimal_on(np.array([-1, 1], dtype=np.int8), 1)
    # the first-maximum rule of the script's argmax(π): a tie in π goes to the first action
    pi, avail = np.array([0.0, 0.4, 0.4, 0.0, 0.2, 0.0, 0.0]), np.array([0, 1, 1, 0, 1, 1, 0], dtype=bool)
    assert Pons._first_argmax(pi, avail) == 1
    assert Pons._first_argmax(np.array([0.9, 0.0, 0.1, 0, 0, 0, 0]), np.array([0, 1, 1, 0, 0, 0, 0], dtype=bool)) == 2   # never an unavailable action
    assert Pons._first_argmax(np.zeros(7), np.array([0, 0, 0, 1, 0, 1, 0], dtype=bool)) == 3


class _OracleSpec:
    """a game spec over the oracle's Connect Four with the GameEnv calls state_of_string makes"""
    class Env:
        def __init__(self):
            self.g, self.played = R.Game(R.C4), []

        def play(self, action):
            assert self.g.actions_mask()[action - 1] and not self.g.terminated()
            self.g.play(action - 1)
            self.played.append(action)

    def init(self):
        return _OracleSpec.Env()


def test_state_of_string_plays_the_columns_in_order_from_the_empty_board():
    for b in Pons.load_benchmarks(PONS):
        for s, _ in b.entries[:50]:
            env = Pons.state_of_string(s, _OracleSpec())
            assert env.played == [int(c) for c in s]
            want = R.Game(R.C4)
            for c in s:
                want.play(int(c) - 1)
            assert env.g.key() == want.key() and not env.g.terminated()
            assert env.g.white_playing() == (len(s) % 2 == 0)
