"""The host's book-keeping rules of a self-play phase (csrc/phase_books.h) without a GPU and without the library:
tests/phase_books_driver.cpp (host compiler, that header only) prints what retire_slots and order_by_game_id decide, and a few lines of
Python restate the rule as include/azhip.h states it (az_selfplay_stats.aborted_games, AZ_REPLACEMENT_GAME_BIT): a retired slot's game
is reported as aborted; an original id gets ONE replacement, id | bit 30, in the same slot; a replacement that retires is given up and
counted as done, and its slot takes the phase's next id while there is one -- else it stays idle and its group has one active slot
fewer.  Ids are handed out in slot order.  An unbounded phase hands out ids up to AZ_REPLACEMENT_GAME_BIT - 1 and no further, which
no GPU test reaches.  Finished games are handed over in game-id order; games with one id keep the order they finished in."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "phase_books_driver.cpp")
BIT = 0x40000000                                    # AZ_REPLACEMENT_GAME_BIT


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("phase_books") / "phase_books_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", SRC, "-o", exe])
    return exe


def retire(exe, total, first, nxt, per_group, ngroups, retired):
    args = [str(v) for v in (total, first, nxt, per_group, ngroups)] + ["%d:%d" % sg for sg in retired]
    text = subprocess.run([exe, "retire"] + args, capture_output=True, text=True, check=True).stdout
    out = {ln.split()[0]: ln.split()[1:] for ln in text.splitlines()}
    return {"aborted": [int(v) for v in out["aborted"]],
            "refill": [tuple(int(x) for x in v.split(":")) for v in out["refill"]],
            "given_up": int(out["given_up"][0]), "next_game": int(out["next_game"][0]),
            "idle": [int(v) for v in out["idle"]]}


def restate(total, first, nxt, per_group, ngroups, retired):
    """the rule, in slot order"""
    r = {"aborted": [], "refill": [], "given_up": 0, "idle": [0] * ngroups}
    for slot, gid in retired:
        r["aborted"].append(gid)
        new = None
        if not gid & BIT:
            new = gid | BIT                         # the phase still owes the caller this game
        else:
            r["given_up"] += 1
            if (first + nxt < BIT) if total < 0 else (nxt < total):
                new, nxt = first + nxt, nxt + 1
        if new is None:
            r["idle"][slot // per_group] += 1
        else:
            r["refill"].append((slot, new))
    r["next_game"] = nxt
    return r


# (total_games, first_game_id, next_game, slots per group, groups, [(retired slot, its game id), ...] in slot order)
CASES = {
    "original": (8, 100, 4, 4, 1, [(2, 101)]),
    "replacement-ids-left": (8, 100, 4, 4, 1, [(2, 101 | BIT)]),
    "replacement-no-ids-left": (8, 100, 8, 4, 2, [(5, 103 | BIT)]),
    "several-two-groups": (12, 7, 9, 4, 2, [(0, 8 | BIT), (1, 9), (3, 12 | BIT), (4, 15 | BIT), (6, 13), (7, 10 | BIT)]),
    "several-ids-run-out": (11, 7, 9, 4, 2, [(1, 8 | BIT), (2, 9 | BIT), (5, 12 | BIT), (6, 13 | BIT)]),
    "unbounded-one-below-bit": (-1, BIT - 16, 15, 4, 1, [(0, 3 | BIT), (3, 5 | BIT)]),
    "unbounded-at-bit": (-1, BIT - 16, 16, 4, 1, [(0, 3 | BIT), (3, 5)]),
}
# what the cases above must give, written out where the issue of a case is one number
EXPECT = {
    "original": {"aborted": [101], "refill": [(2, 101 | BIT)], "given_up": 0, "next_game": 4, "idle": [0]},
    "replacement-ids-left": {"aborted": [101 | BIT], "refill": [(2, 104)], "given_up": 1, "next_game": 5, "idle": [0]},
    "replacement-no-ids-left": {"aborted": [103 | BIT], "refill": [], "given_up": 1, "next_game": 8, "idle": [0, 1]},
    "several-two-groups": {"refill": [(0, 16), (1, 9 | BIT), (3, 17), (4, 18), (6, 13 | BIT)], "given_up": 4, "next_game": 12,
                           "idle": [0, 1]},
    "unbounded-one-below-bit": {"refill": [(0, BIT - 1)], "given_up": 2, "next_game": 16, "idle": [1]},
    "unbounded-at-bit": {"refill": [(3, 5 | BIT)], "given_up": 1, "next_game": 16, "idle": [1]},
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_retire_slots(driver, name):
    got = retire(driver, *CASES[name])
    assert got == restate(*CASES[name])
    for key, val in EXPECT.get(name, {}).items():
        assert got[key] == val, key
    assert len(got["aborted"]) == len(CASES[name][5]) == len(got["refill"]) + sum(got["idle"])
    assert [s for s, _ in got["refill"]] == sorted(s for s, _ in got["refill"])
    fresh = [g for _, g in got["refill"] if not g & BIT]
    assert fresh == sorted(fresh) and all(g < BIT for g in fresh)


@pytest.mark.parametrize("ids", [[], [4], [3, 1, 2, 0], [5, 3, 5, 1, 3, 5], [7, 7, 7], [2 | BIT, 9, 2, 9 | BIT, 0]])
def test_order_by_game_id(driver, ids):
    text = subprocess.run([driver, "order"] + [str(i) for i in ids], capture_output=True, text=True, check=True).stdout
    assert [int(v) for v in text.split()[1:]] == sorted(range(len(ids)), key=lambda i: ids[i])   # (sorted is stable)
