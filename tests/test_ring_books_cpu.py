"""The books of the replay memories' circular buffer (csrc/ring_books.h) without a GPU and without the library:
tests/ring_books_driver.cpp (host compiler, that header only) replays a script of pushes, new_batch and empty and prints what the
record then answers; tests/ring_books_cases.py holds the scripts and the model, a deque(maxlen=cap) of sequence numbers and an
unclamped batch counter.  The sample with sequence number q sits in slot q % cap, so the pieces the record hands out for a selection
must walk exactly the slots of the deque's entries, in at most two runs, none of them empty.  For one push of n, skip is how many of
its entries never get stored; where that is more than none it equals min_seq minus the total before the push."""
import os
import subprocess

import pytest

import ring_books_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "ring_books_driver.cpp")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ring_books") / "ring_books_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", SRC, "-o", exe])
    return exe


def replay(exe, cap, script):
    args = [":".join(str(int(v)) if not isinstance(v, str) else v for v in op) for op in script]
    text = subprocess.run([exe, str(cap)] + args, capture_output=True, text=True, check=True).stdout
    out = {"pushes": []}
    for ln in text.splitlines():
        key, *vals = ln.split()
        if key == "push":
            out["pushes"].append(dict(zip(("n", "skip", "min_seq", "total_before"), (int(v) for v in vals))))
        elif key.startswith("runs"):
            out[key] = [tuple(int(x) for x in v.split(":")) for v in vals]
        elif key.startswith("select"):
            out[key] = (int(vals[0]), int(vals[1]))
        else:
            out[key] = int(vals[0])
    return out


def pieces(cap, seq0, count):
    """the slots of seq0 .. seq0 + count as contiguous pieces, restated"""
    first = min(count, cap - seq0 % cap)
    return [(p, r) for p, r in ((seq0 % cap, first), (0, count - first)) if r > 0]


def check_pushes(got, cap):
    for p in got["pushes"]:
        assert p["skip"] == max(0, p["n"] - cap)
        assert p["min_seq"] == max(0, p["total_before"] + p["n"] - cap)
        if p["skip"] > 0:
            assert p["skip"] == p["min_seq"] - p["total_before"]


@pytest.mark.parametrize("name", sorted(RC.CASES))
def test_script_against_the_deque(driver, name):
    cap, script = RC.CASES[name]
    got, want = replay(driver, cap, script), RC.model(cap, script)
    for key in ("len", "batch", "stored_batch", "total"):
        assert got[key] == want[key], key
    assert [p["skip"] for p in got["pushes"]] == want["skips"]
    check_pushes(got, cap)
    for sel, runs, entries in (("select0", "runs0", want["experience"]), ("select1", "runs1", want["last_batch"])):
        n0, seq0 = got[sel]
        assert n0 == len(entries)
        assert seq0 == (entries[0] if entries else want["total"])
        assert len(got[runs]) <= 2 and all(0 <= p and 0 < r and p + r <= cap for p, r in got[runs])
        assert [s for p, r in got[runs] for s in range(p, p + r)] == [q % cap for q in entries]
        assert got[runs] == pieces(cap, seq0, n0)
    # what the case is about, written out
    exp = RC.EXPECT.get(name, {})
    for key in ("len", "batch", "stored_batch"):
        if key in exp:
            assert got[key] == exp[key], key
    if "runs" in exp:
        assert got["runs0"] == exp["runs"]
    if "skips" in exp:
        assert [p["skip"] for p in got["pushes"]] == exp["skips"]
    for key in ("experience", "last_batch"):
        if key in exp:
            assert want[key] == exp[key], key


def test_every_listed_expectation_names_a_case():
    assert set(RC.EXPECT) <= set(RC.CASES)
    assert all(cap <= 8 for cap, _ in RC.CASES.values())            # the device test runs them all


def test_largest_capacity_far_into_its_life(driver):
    """cap = 2^31 - 1, total = 2^40 + 3, a batch counter past 2^33: every figure against Python's integers, which do not overflow"""
    cap = RC.BIG_CAP
    got = replay(driver, cap, RC.BIG)
    (_, total, cur), (_, n1, _), (_, n2, _) = RC.BIG
    assert [p["total_before"] for p in got["pushes"]] == [total, total + n1]
    check_pushes(got, cap)
    assert got["pushes"][1]["skip"] == 2 * cap + 2
    total += n1 + n2
    assert got["total"] == total and got["len"] == cap and got["stored_batch"] == cur + n1 and got["batch"] == cap
    assert got["select0"] == got["select1"] == (cap, total - cap)
    for runs in (got["runs0"], got["runs1"]):
        assert runs == pieces(cap, total - cap, cap)
        assert len(runs) <= 2 and all(0 <= p and 0 < r <= cap and p + r <= cap for p, r in runs) and sum(r for _, r in runs) == cap
    # the same ring before the two pushes: the batch is larger than the ring, the selection one wrapped piece pair
    got = replay(driver, cap, RC.BIG[:1])
    total = RC.BIG[0][1]
    assert got["batch"] == cap and got["stored_batch"] == cur
    assert got["runs0"] == [(total % cap, cap - total % cap), (0, total % cap)]
