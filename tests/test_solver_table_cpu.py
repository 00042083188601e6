"""The Connect Four solver's search with a transposition table, on the host: csrc/solver_search.h is what the kernels of
csrc/solver.h run, and tests/solver_table_driver.cpp (built here with g++, no HIP) runs it over a std::vector<uint64_t> table, a
state at a time: 7 first passes, then the second pass, as the kernel does.

References: the recorded scores of tests/golden/pons, and azref.c4_solve (the oracle's CPU negamax) for q-values, as
tests/test_solver_gpu.py::end_set builds them.  Nothing here asserts which positions finish under a budget, except the coverage
condition of test_coverage, which the issue sets (at most half as many unknown values as the tableless path)."""
import functools
import os
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import azref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PONS = os.path.join(ROOT, "tests", "golden", "pons")
NA, UNSOLVED = -128, 127
BUDGET = 1 << 18
SIZES = (0, 4, 10, 20)


@functools.lru_cache(maxsize=None)
def driver():
    exe = os.path.join(tempfile.mkdtemp(prefix="solver_table_"), "solver_table_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas",
                           os.path.join(ROOT, "tests", "solver_table_driver.cpp"), "-o", exe])
    return exe


def run(lines):
    """the driver over `lines` -> value (n,), q (n, 7), nodes (n,) of the positions among them, in order"""
    out = subprocess.run([driver()], input="".join(l + "\n" for l in lines), capture_output=True, text=True, check=True).stdout
    rows = np.array([[int(x) for x in l.split()] for l in out.splitlines()], dtype=np.int64).reshape(-1, 9)
    assert rows.shape[0] == sum(1 for l in lines if not l.startswith("#"))
    return rows[:, 0], rows[:, 1:8], rows[:, 8]


def entries(name, k=None):
    return [(l.split()[0], int(l.split()[1])) for l in open(os.path.join(PONS, name)) if l.strip()][:k]


def game_of(s):
    g = R.Game(R.C4)
    for c in s:
        g.play(int(c) - 1)
    return g


def reference_q(ents, limit):
    """per entry the q-values by full action index: NA on a full column, UNSOLVED where the CPU negamax needs more than `limit` nodes"""
    Q = np.full((len(ents), 7), NA, dtype=np.int64)
    for i, (s, _) in enumerate(ents):
        g, moves = game_of(s), [int(c) - 1 for c in s]
        for a in g.available_actions():
            c = g.clone()
            c.play(a)
            if c.terminated():
                Q[i, a] = 0 if c.white_reward() == 0 else 21 - len(s) // 2
            else:
                sc, _ = R.c4_solve(moves + [int(a)], limit)
                Q[i, a] = -sc if sc < 98 else UNSOLVED
    return Q


@functools.lru_cache(maxsize=None)
def middle():
    """the first 200 of Test_L2_R2: entries, scores, the q-values the CPU negamax finds within 200 000 nodes"""
    ents = entries("Test_L2_R2", 200)
    return ents, np.array([sc for _, sc in ents], dtype=np.int64), reference_q(ents, 200_000)


def middle_lines(log2, per_position_clear=False, ents=None):
    ents = middle()[0] if ents is None else ents
    lines = ["#table %d" % log2, "#budget %d" % BUDGET]
    for s, _ in ents:
        lines += (["#clear"] if per_position_clear else []) + [s]
    return lines


@functools.lru_cache(maxsize=None)
def middle_runs():
    """every configuration of the 200 middle / medium positions, each run once: {(log2, cleared per position): (value, q, nodes)}; -1 = no table"""
    cfgs = [(-1, False)] + [(lg, cl) for lg in SIZES for cl in (False, True)]
    driver()
    with ThreadPoolExecutor(4) as pool:
        return dict(zip(cfgs, pool.map(lambda c: run(middle_lines(*c)), cfgs)))


def check_exact(value, q, score, Q=None, weak=False):
    want = np.sign(score) if weak else score
    known = value != UNSOLVED
    assert np.array_equal(value[known], want[known])
    solved = (q != NA) & (q != UNSOLVED)
    assert (q <= want[:, None])[solved].all()
    if Q is not None:
        assert np.array_equal(q == NA, Q == NA)
        both = solved & (Q != UNSOLVED)
        assert np.array_equal(q[both], (np.sign(Q) if weak else Q)[both])
    return known


def test_end_set():
    """(a) all 1000 of Test_L3_R1, 2^16 entries, 4096 nodes: every q is the reference's, every value the recorded score"""
    ents = entries("Test_L3_R1")
    Q = reference_q(ents, 20_000_000)
    assert (Q != NA).sum() == 3217 and not (Q == UNSOLVED).any()
    value, q, nodes = run(["#table 16", "#budget 4096"] + [s for s, _ in ents])
    assert np.array_equal(q, Q)
    assert np.array_equal(value, np.array([sc for _, sc in ents]))
    plain = run(["#table -1", "#budget 4096"] + [s for s, _ in ents])
    assert np.array_equal(plain[0], value) and np.array_equal(plain[1], q)


@pytest.mark.parametrize("cleared", [False, True])
@pytest.mark.parametrize("log2", SIZES)
def test_middle_medium_is_exact_at_every_table_size(log2, cleared):
    """(b) a table of one entry replaces on every store; kept across the positions or cleared before each"""
    ents, score, Q = middle()
    value, q, nodes = middle_runs()[log2, cleared]
    known = check_exact(value, q, score, Q)
    print("2^%d entries, %s: %d of 200 values known, %d nodes" % (log2, "cleared per position" if cleared else "kept", known.sum(), nodes.sum()))


def test_coverage():
    """(c) the table of 2^20 entries leaves a value unknown on at most half as many positions as the tableless host path"""
    ents, score, Q = middle()
    plain, table = middle_runs()[-1, False], middle_runs()[20, False]
    check_exact(plain[0], plain[1], score, Q)
    left_plain, left_table = int((plain[0] == UNSOLVED).sum()), int((table[0] == UNSOLVED).sum())
    print("values unknown of 200 at 2^18 nodes: %d without a table, %d with 2^20 entries" % (left_plain, left_table))
    assert left_plain > 0 and 2 * left_table <= left_plain


def test_stale_entries_are_harmless_and_a_warm_table_helps():
    """(d) a table filled by another set's positions, then this set twice: exact, and the second pass enters strictly fewer nodes
    and solves a superset"""
    ents, score, Q = middle()
    other = entries("Test_L2_R1", 200)
    lines = ["#table 20", "#budget %d" % BUDGET] + [s for s, _ in other] + [s for s, _ in ents] + [s for s, _ in ents]
    value, q, nodes = run(lines)
    check_exact(value[:200], q[:200], np.array([sc for _, sc in other]))
    first, second = slice(200, 400), slice(400, 600)
    k1 = check_exact(value[first], q[first], score, Q)
    k2 = check_exact(value[second], q[second], score, Q)
    print("known %d then %d of 200, nodes %d then %d" % (k1.sum(), k2.sum(), nodes[first].sum(), nodes[second].sum()))
    assert (k2 | ~k1).all() and nodes[second].sum() < nodes[first].sum()


def test_mixed_modes():
    """(e) weak after strong and strong after weak on one table: weak is the sign of strong wherever both are solved"""
    ents, score, Q = middle()
    pos = [s for s, _ in ents[:100]]
    for order in ((0, 1), (1, 0)):
        lines = ["#table 16", "#budget %d" % (1 << 16)]
        for weak in order:
            lines += ["#weak %d" % weak] + pos
        value, q, _ = run(lines)
        out = {weak: (value[k * 100:(k + 1) * 100], q[k * 100:(k + 1) * 100]) for k, weak in enumerate(order)}
        check_exact(out[0][0], out[0][1], score[:100], Q[:100])
        check_exact(out[1][0], out[1][1], score[:100], Q[:100], weak=True)
        both = (out[0][0] != UNSOLVED) & (out[1][0] != UNSOLVED)
        assert both.any() and np.array_equal(np.sign(out[0][0][both]), out[1][0][both])
        qb = (out[0][1] != UNSOLVED) & (out[1][1] != UNSOLVED) & (out[0][1] != NA)
        assert np.array_equal(np.sign(out[0][1][qb]), out[1][1][qb])
