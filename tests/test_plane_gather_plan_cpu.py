"""The plan of az_comm_gather_push_planes (csrc/plane_gather.h) without a GPU and without the library: tests/plane_gather_driver.cpp
(host compiler, that header only) prints the plan for given per-rank game tables, and a few lines of numpy restate what the header
promises: the samples of all ranks in ascending game id, a run keeping its order; every (rank, row) of the packed batches maps to a
distinct position q in [0, T); the round count is ceil(max B_r / R); a duplicate id is reported with the id.  The driver is also built
once with AddressSanitizer and UBSan and run as the stand-alone program it is.  Then the header, the mirror and the Julia list."""
import os
import re
import subprocess

import numpy as np
import pytest

from azhip import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "plane_gather_driver.cpp")

# (round rows, destination capacity, per-rank tables [(id, len), ...] in push order)
CASES = {
    "one-rank-interleaved": (4, 25, [[(40, 5), (3, 9), (17, 1), (8, 7), (21, 6)]]),
    "one-rank-divides": (7, 100, [[(2, 7), (1, 7), (0, 14)]]),
    "three-ranks-one-empty": (4, 30, [[(9, 3), (6, 1), (3, 5), (0, 2)], [], [(10, 9), (7, 4), (4, 6), (1, 8)]]),
    "three-ranks-T-above-capacity": (5, 20, [[(5, 4), (2, 7)], [(4, 1), (1, 9), (7, 2)], [(0, 3), (3, 3), (6, 5)]]),
    "eight-ranks": (3, 1000, [[(r + 8 * k, 1 + (r * 5 + k * 3) % 9) for k in reversed(range(r % 4))] for r in range(8)]),
    "eight-ranks-one-round": (1 << 20, 40, [[(8 * k + (7 - r), 1 + (r + k) % 6) for k in range(3)] for r in range(8)]),
    "all-empty": (4, 10, [[], [], []]),
}


def build(tmp, flags, name):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"] + flags + [SRC, "-o", exe])
    return exe


def run(exe, R, cap, tables):
    args = [",".join("%d:%d" % g for g in t) if t else "-" for t in tables]
    text = subprocess.run([exe, str(R), str(cap)] + args, capture_output=True, text=True, check=True).stdout
    out = {"game": [], "row": [], "send": [], "rb": [], "rows": []}
    for kind, *val in (ln.split() for ln in text.splitlines()):
        if kind == "plan":
            out["plan"] = [int(v) for v in val]
        else:
            out[kind].append([int(v) for v in val])
    return out, text


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build(tmp_path_factory.mktemp("plane_gather"), [], "plane_gather_driver")


def restate(tables):
    """(rank, sample of its batch in push order) of every position q: ascending id, a run in the order it was pushed"""
    runs = []
    for r, t in enumerate(tables):
        off = 0
        for gid, n in t:
            runs.append((gid, r, off, n))
            off += n
    seq = []
    for gid, r, off, n in sorted(runs):
        seq += [(r, off + i) for i in range(n)]
    return seq


@pytest.mark.parametrize("case", sorted(CASES))
def test_plan_orders_every_sample_by_game_id(driver, case):
    R, cap, tables = CASES[case]
    out, _ = run(driver, R, cap, tables)
    W, T, maxB, gotR, rounds, skip, dup, dup_id = out["plan"]
    Bs = [sum(n for _, n in t) for t in tables]
    assert (W, T, maxB, gotR) == (len(tables), sum(Bs), max(Bs), R) and (dup, dup_id) == (0, -1)
    assert rounds == -(-max(Bs) // R) and skip == max(0, T - cap)
    # the games of a rank: packed in ascending id, prefix sums over the packed order, src = where the run lies in push order
    for r, t in enumerate(tables):
        games = [g[2:] for g in out["game"] if g[0] == r]
        ids = [g[0] for g in games]
        assert ids == sorted(i for i, _ in t)
        off = {gid: sum(n for _, n in t[:k]) for k, (gid, _) in enumerate(t)}
        assert [g[1] for g in games] == [dict(t)[i] for i in ids] and [g[2] for g in games] == [off[i] for i in ids]
        assert [g[3] for g in games] == list(np.concatenate([[0], np.cumsum([g[1] for g in games])])[:-1].astype(int))
    # every (rank, packed row) -> a distinct q in [0, T), and position q holds the sample the restatement puts there
    rows = out["row"]
    assert len(rows) == T and sorted(q for *_, q in rows) == list(range(T))
    want = restate(tables)
    for r, s, rnd, j, q in rows:
        assert want[q] == (r, j) and rnd == s // R
    for r in range(W):                                                   # a rank's packed rows are its samples by (id, offset): q ascends with s
        qs = [q for rr, s, _, _, q in sorted(rows) if rr == r]
        assert qs == sorted(qs) and len(qs) == Bs[r]
    # the round split: every rank runs `rounds` rounds, sends its rows [k R, (k + 1) R) and padding after them
    for r in range(W):
        sent = [n for rr, k, n in out["send"] if rr == r]
        assert len(sent) == rounds and sum(sent) == Bs[r] and all(0 <= n <= R for n in sent)
        assert sent == [max(0, min(R, Bs[r] - k * R)) for k in range(rounds)]


def test_duplicate_ids_are_reported_with_the_id(driver):
    one, _ = run(driver, 4, 100, [[(5, 2), (9, 1), (5, 3)], [(1, 1)]])                 # twice on one rank
    assert one["plan"][6:] == [1, 5]
    two, _ = run(driver, 4, 100, [[(5, 2), (9, 1)], [(1, 1)], [(12, 4), (9, 3), (1, 2)]])   # twice across ranks: the smallest id is named
    assert two["plan"][6:] == [1, 1]
    none, _ = run(driver, 4, 100, [[(5, 2), (9, 1)], [(1, 1)], [(12, 4), (8, 3), (0, 2)]])
    assert none["plan"][6:] == [0, -1]


def test_record_bytes_and_default_round_rows(driver):
    out, _ = run(driver, 1, 1, [[(0, 1)]])
    assert out["rb"] == [[36, 11, 240], [133, 9, 616], [76, 8, 376], [406, 84, 2304]]
    for W, rb, rows in out["rows"]:
        assert W * rows * rb <= 256 << 20 < W * (rows + 1) * rb             # the largest R with W R rb <= 256 MiB


def test_driver_under_address_and_undefined_sanitizers(tmp_path, driver):
    """the same program, -fsanitize=address,undefined: every case once, clean and with the same output"""
    exe = build(tmp_path, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "plane_gather_driver_san")
    for case in sorted(CASES):
        assert run(exe, *CASES[case])[1] == run(driver, *CASES[case])[1], case
    assert run(exe, 4, 100, [[(5, 2), (9, 1), (5, 3)], [(1, 1)]])[0]["plan"][6:] == [1, 5]


def test_header_mirror_and_julia_list_know_the_entry_point():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "azhip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+az_comm_gather_push_planes\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)
    assert m and len(m.group(1).split(",")) == 7
    assert len(L.SYMBOLS["az_comm_gather_push_planes"]) == 7
    assert re.search(r"#define AZ_ABI_VERSION 4\b", hdr) and L.ABI_VERSION == 4
    jl = open(os.path.join(ROOT, "julia", "AlphaZeroHIPExtras.jl")).read()
    unbound = re.search(r"const UNBOUND = Dict\((.*?)\n\)", jl, flags=re.S).group(1)
    assert re.search(r":az_comm_gather_push_planes\s*=>\s*\"[^\"]+\"", unbound)
    eng = open(os.path.join(ROOT, "alphazero.jl_amd", "csrc", "engine.h")).read()
    assert "az_debug_comm_plane_round_rows(az_comm* c, int64_t rows)" in eng and "az_debug_comm_plane_round_rows" not in hdr
