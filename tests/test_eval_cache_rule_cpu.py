"""The rules of the evaluation cache (csrc/eval_cache_rule.h) without a GPU and without the library: tests/eval_cache_rule_driver.cpp
(host compiler, that header only) answers queries, this file restates the rules in Python and sweeps both.

  ec_pick_victim  every combination of the four states x {at or below the floor, stale, fresh, from the future} for both ways, with
                  and without the state's own key in either way -- against the restatement, and a list of cases written out by hand
  ec_size_log2    slots x simulations x free memory x override, against the restatement and against the sizes the engine had before
                  the table grew (small engines keep them)
  ec_set_of       the two entries of a set are the two halves of one 128-byte line
  ec_way_hit      READY, above the floor, the key, the checksum: each of them alone refuses

The driver is built a second time with -fsanitize=address,undefined (a program with its own main, run on its own) and must give
the same answers with nothing reported."""
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "eval_cache_rule_driver.cpp")

EMPTY, PENDING, READY, FILLING = 0, 1, 2, 3
STALE_AFTER = 64
M64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    d = tmp_path_factory.mktemp("eval_cache_rule")
    plain, san = str(d / "driver"), str(d / "driver_san")
    base = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", SRC]
    subprocess.check_call(base + ["-O1", "-o", plain])
    subprocess.check_call(base + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", san])
    return plain, san


def ask(drivers, queries):
    """every query through both builds; the sanitized one must agree and report nothing"""
    text = "".join(" ".join(str(v) for v in q) + "\n" for q in queries)
    outs = []
    for exe in drivers:
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "", (exe, r.returncode, r.stderr[-2000:])
        outs.append(r.stdout.splitlines())
    assert outs[0] == outs[1] and len(outs[0]) == len(queries)
    return outs[0]


# ---------------------------------------------------------------- the restatement
def mix64(x):
    x ^= x >> 30
    x = x * 0xbf58476d1ce4e5b9 & M64
    x ^= x >> 27
    x = x * 0x94d049bb133111eb & M64
    return x ^ (x >> 31)


def hash_key(a, b):
    return mix64(a ^ mix64((b + 0x9e3779b97f4a7c15) & M64))


def set_of(a, b, mask):
    return (hash_key(a, b) >> 17) & 0xffffffff & mask


def checksum(px, a, b, vbits, ready_meta):
    h = mix64(hash_key(a, b) ^ (px << 32 | vbits))
    h = mix64((h + ready_meta) & M64)
    return (h >> 32) ^ (h & 0xffffffff)


def way_kind(meta, seq, floor):
    n = meta >> 2
    if meta == 0 or n <= floor:
        return "free"
    if meta & 3 == READY:
        return "answered"
    age = (seq - n + (1 << 31)) % (1 << 32) - (1 << 31)               # signed: a claim of a launch with a higher number is young
    return "stale" if age > STALE_AFTER else "fresh"


def pick_victim(m0, m1, same0, same1, seq, floor):
    kinds = [way_kind(m0, seq, floor), way_kind(m1, seq, floor)]
    if any(k == "fresh" and s for k, s in zip(kinds, (same0, same1))):
        return -1
    for want in ("free", "stale"):
        for w in (0, 1):
            if kinds[w] == want:
                return w
    answered = [w for w in (0, 1) if kinds[w] == "answered"]
    if not answered:
        return -1
    return min(answered, key=lambda w: ((m0, m1)[w] >> 2, w))        # the older claim number, way 0 on a tie


def size_log2(G, sims, override, free_bytes, big_mult, big_cap):
    if override > 0:
        return min(max(override, 4), 28)
    work = max(G, 1) * max(sims, 1)
    lg = 16
    while lg < 24 and (1 << lg) < 8 * work:
        lg += 1
    if lg == 24:
        while lg < big_cap and (1 << lg) < big_mult * work:
            lg += 1
    while lg > 16 and (64 << lg) > free_bytes // 8:
        lg -= 1
    return lg


def size_before(G, sims):
    """the engine's rule before the table grew: 8 x slots x simulations, 2^16 .. 2^24"""
    lg = 16
    while lg < 24 and (1 << lg) < 8 * G * max(1, sims):
        lg += 1
    return lg


# ---------------------------------------------------------------- ec_pick_victim
SEQ, FLOOR = 2000, 1000
CLAIMS = {"floor": (FLOOR, 500, 1), "stale": (SEQ - STALE_AFTER - 1, FLOOR + 1), "fresh": (SEQ - STALE_AFTER, SEQ - 1, SEQ),
          "future": (SEQ + 1, SEQ + 50)}


def metas():
    out = [(0, "zero")]
    for state in (EMPTY, PENDING, READY, FILLING):
        for cls, ns in CLAIMS.items():
            out += [(n << 2 | state, "%d/%s" % (state, cls)) for n in ns]
    return out


def test_pick_victim_sweep(drivers):
    ms = [m for m, _ in metas()]
    cases = [(m0, m1, s0, s1, SEQ, FLOOR) for m0, m1 in itertools.product(ms, ms) for s0, s1 in itertools.product((0, 1), (0, 1))]
    got = [int(x) for x in ask(drivers, [("victim",) + c for c in cases])]
    want = [pick_victim(*c) for c in cases]
    bad = [(c, g, w) for c, g, w in zip(cases, got, want) if g != w]
    assert not bad, bad[:5]
    assert {-1, 0, 1} == set(got)
    # properties, not through the restatement: a fresh or future claim (PENDING or FILLING, above the floor) is never the victim
    for c, g in zip(cases, got):
        if g >= 0:
            m = c[g]
            assert not ((m & 3) in (PENDING, FILLING) and (m >> 2) > FLOOR and (m >> 2) >= SEQ - STALE_AFTER), (c, g)


def M(n, state):
    return n << 2 | state


@pytest.mark.parametrize("m0,m1,same0,same1,want", [
    (0, 0, 0, 0, 0),                                                        # both empty: way 0
    (M(1990, READY), 0, 0, 0, 1),                                           # the empty way before the answered one
    (M(1990, READY), M(900, READY), 0, 0, 1),                               # at or below the floor counts as empty
    (M(1000, PENDING), M(1990, READY), 0, 0, 0),                            # ... whatever its state, exactly at the floor too
    (M(1990, READY), M(1500, PENDING), 0, 0, 1),                            # a stale claim before an answer
    (M(1935, FILLING), M(1500, READY), 0, 0, 0),                            # age 65: stale
    (M(1936, FILLING), M(1500, READY), 0, 0, 1),                            # age 64: still fresh, the answer goes
    (M(1990, READY), M(1980, READY), 0, 0, 1),                              # two answers: the older claim goes
    (M(1980, READY), M(1990, READY), 0, 0, 0),
    (M(1985, READY), M(1985, READY), 0, 0, 0),
    (M(1999, PENDING), M(1990, READY), 0, 0, 1),                            # a fresh claim stays, the answer beside it goes
    (M(1999, PENDING), M(2000, FILLING), 0, 0, -1),                         # both fresh: no claim
    (M(2040, PENDING), M(2001, PENDING), 0, 0, -1),                         # claims from the future of another slot group are fresh
    (M(2040, PENDING), M(1990, READY), 0, 0, 1),
    (M(1999, PENDING), 0, 1, 0, -1),                                        # the state's own key is PENDING: the empty way is NOT claimed
    (0, M(1999, PENDING), 0, 1, -1),
    (M(1990, READY), M(2001, PENDING), 0, 1, -1),
    (M(1500, PENDING), 0, 1, 0, 1),                                         # a stale claim under the own key no longer stands for an answer to come
    (M(900, PENDING), M(1990, READY), 1, 0, 0),                             # nor does one below the floor
    (M(1990, READY), 0, 1, 0, 1),                                           # an answer under the own key that the look refused (checksum): no bar
])
def test_pick_victim_cases_written_out(drivers, m0, m1, same0, same1, want):
    assert int(ask(drivers, [("victim", m0, m1, same0, same1, SEQ, FLOOR)])[0]) == want == pick_victim(m0, m1, same0, same1, SEQ, FLOOR)


def test_pick_victim_where_the_launch_number_is_small_or_huge(drivers):
    """seq below EC_STALE_AFTER (a young engine: nothing is stale), and seq near the 2^29 the host wipes the table at"""
    cases = [(M(1, PENDING), M(2, READY), 0, 0, 3, 0), (M(1, PENDING), M(2, PENDING), 0, 0, 60, 0), (M(1, PENDING), M(2, PENDING), 0, 0, 66, 0),
             (M((1 << 29) - 1, PENDING), M((1 << 29) - 70, PENDING), 0, 0, (1 << 29) - 1, 5), (M((1 << 29) - 1, READY), M((1 << 29) - 2, READY), 0, 0, (1 << 29) - 1, 5)]
    got = [int(x) for x in ask(drivers, [("victim",) + c for c in cases])]
    assert got == [pick_victim(*c) for c in cases] == [1, -1, 0, 1, 1]


# ---------------------------------------------------------------- ec_size_log2
BIG_MULT, BIG_CAP = 64, 27                                       # eval_cache_rule.h EC_BIG_MULT, EC_BIG_CAP_LOG2
GB = 1 << 30


def test_size_sweep(drivers):
    cases = [(G, sims, ov, free) for G in (8, 128, 4096, 8192) for sims in (8, 100, 400, 800) for free in (1 * GB, 16 * GB, 256 * GB) for ov in (0, 4, 28)]
    got = [int(x) for x in ask(drivers, [("size",) + c for c in cases])]
    for (G, sims, ov, free), lg in zip(cases, got):
        assert lg == size_log2(G, sims, ov, free, BIG_MULT, BIG_CAP), (G, sims, ov, free)
        if ov:
            assert lg == ov                                         # the override is taken as it is
            continue
        assert 16 <= lg <= BIG_CAP
        assert lg == 16 or (64 << lg) <= free // 8                  # never more than 1/8 of the free memory
        if G <= 128 and free >= 16 * GB:
            assert lg == size_before(G, sims)                       # test engines and the arena's players stay as small as they were
        assert lg >= min(size_before(G, sims), size_log2(G, sims, 0, free, 8, 24))   # nobody's table shrank, but for the memory rule
    by = dict(zip(cases, got))
    assert by[(8, 8, 0, 256 * GB)] == 16 and by[(128, 800, 0, 256 * GB)] == 20
    assert by[(4096, 400, 0, 256 * GB)] == BIG_CAP and by[(8192, 800, 0, 256 * GB)] == BIG_CAP    # the headline, and a larger engine
    assert by[(4096, 100, 0, 256 * GB)] == 22                       # 8 x does not fill 2^24: the size it had
    assert by[(4096, 400, 0, 1 * GB)] == 21 and by[(4096, 400, 0, 16 * GB)] == 25                 # 128 MB, 2 GB
    # an override outside 4 .. 28 (env.h clamps it before; the rule clamps again)
    assert [int(x) for x in ask(drivers, [("size", 4096, 400, 2, GB), ("size", 4096, 400, 31, GB)])] == [4, 28]


# ---------------------------------------------------------------- ec_set_of, ec_way_hit
def test_both_entries_of_a_set_share_a_line(drivers):
    keys = [(0, 0), (1, 0), (0, 1), (M64, M64), (0x123456789abcdef, 0xfedcba9876543210)] + [(mix64(i), mix64(i + 77)) for i in range(200)]
    cases = [(a, b, mask) for a, b in keys for mask in (0, 7, (1 << 23) - 1, (1 << 27) - 1)]
    seen = set()
    for (a, b, mask), ln in zip(cases, ask(drivers, [("set",) + c for c in cases])):
        s, off0, off1 = (int(x) for x in ln.split())
        assert s == set_of(a, b, mask) and 0 <= s <= mask
        assert off0 == 128 * s and off1 == off0 + 64 and off0 // 128 == off1 // 128 == (off1 + 63) // 128
        if mask == 7:
            seen.add(s)
    assert seen == set(range(8))                                    # eight sets (AZHIP_EVAL_CACHE_LOG2 = 4) are all in use


def test_way_hit_needs_every_condition(drivers):
    a, b, vbits, px, floor = 0x1122334455667788, 0x99aabbccddeeff00, 0x3f000000, 0xdeadbeef, 10
    ready = M(50, READY)
    cs = checksum(px, a, b, vbits, ready)
    assert int(ask(drivers, [("checksum", px, a, b, vbits, ready)])[0]) == cs
    q = lambda meta=ready, fl=floor, ka=a, kb=b, v=vbits, c=cs, p=px, xa=a, xb=b: ("hit", meta, fl, ka, kb, v, c, p, xa, xb)
    cases = [q(), q(meta=M(50, PENDING)), q(meta=M(50, FILLING)), q(meta=0), q(fl=50), q(fl=49), q(ka=a ^ 1), q(kb=b ^ 1), q(xa=a ^ 1, ka=a),
             q(v=vbits ^ 1), q(c=cs ^ 1), q(p=px ^ 1),
             q(meta=M(51, READY))]                                  # the checksum covers the claim number: words of two claims do not mix
    assert [int(x) for x in ask(drivers, cases)] == [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0]
