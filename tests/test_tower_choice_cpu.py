"""Which network kernel serves a launch (csrc/tower_choice.h), without a GPU and without the library.
tests/tower_choice_driver.hip (hipcc --offload-host-only; no HIP runtime call) runs the rule over the facts csrc/net_impl.h takes from
the real form descriptors of the four geometries and prints where the answer changes:
  * `table`: the facts and the sweeps A (automatic choice), B (split tower) and C (forced forms).  They must equal
    tests/golden/tower_choice.txt line for line -- what pick_tower of the commit before tower_choice.h gave for the same sweeps (the
    file's header says how it was made).
  * `wave` (sweep D): the two rules a search wave puts on top -- the 176-register paired form where the background search's workgroups
    cost the launch a round, and the mixed launch -- and the stop flag.  The commit before had them inline between launches, so they are
    restated here from its text: wgs > rounds * (cu - bg) - 14, and seen > first and seen + 16 <= first + cu * TB7.
  * `heads` (sweep E): the four-way choice of the dense heads' kernel, against a restatement of its four branches."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "alphazero.jl_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "tower_choice.txt")


def golden_lines():
    with open(GOLDEN) as f:
        return [ln.rstrip("\n") for ln in f if not ln.startswith("#")]


def sweeps(lines):
    """{header line: [(from n, form), ...]} of the break-point sweeps in `lines`, and the facts {(game, F, id, bf16): {field: text}}"""
    out, facts, cur = {}, {}, None
    for ln in lines:
        if ln.startswith("  "):
            cur.append(tuple(int(v) for v in ln.split()))
        elif ln.startswith("facts "):
            w = ln.split()
            kv = dict(x.split("=") for x in w[2:])
            facts[(w[1], int(kv["F"]), int(kv["id"]), int(kv["bf16"]))] = kv
        else:
            cur = out.setdefault(ln, [])
    return out, facts


def at(points, n):
    """the value a break-point list gives at n"""
    return [p for p in points if p[0] <= n][-1][1:]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tower_choice") / "tower_choice_driver")
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-host-only", "-I/opt/rocm/include", "-I" + CSRC, "-O1", "-std=c++17",
                           "-fconstexpr-steps=200000000", "-Wall", "-Werror", "-Wno-unused-function",
                           os.path.join(ROOT, "tests", "tower_choice_driver.hip"), "-o", exe])
    return lambda what: subprocess.run([exe, what], capture_output=True, text=True, check=True).stdout.splitlines()


def test_table_equals_the_parent_rule(driver):
    got, want = driver("table"), golden_lines()
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, "line %d: got %r, golden %r" % (i + 1, a, b)
    assert len(got) == len(want)
    # the sweeps the golden file must hold: 4 geometries x (A: 2 F x 2 x 2 x 3, B: 3 x 4 x 2 x 6, C: 2 F x 2 x 10), 22 facts each
    heads = [ln for ln in want if not ln.startswith("  ")]
    assert [sum(h.startswith(k) for h in heads) for k in ("facts ", "A ", "B ", "C ")] == [4 * 22, 4 * 24, 4 * 144, 4 * 40]
    assert at(sweeps(want)[0]["A ConnectFour F=64 bf16=0 groups=1 cu=256"], 1537) == (21,)


def restate_wave(seen, needy, off, lookup, tb8, tb7, apad, N=4096, cu=256):
    """the wave rules as the commit before tower_choice.h had them inline; `off` = the gate that is off, lookup(groups, n) = sweep A"""
    groups, pick = (2 if off == "groups" else 1), (21 if off == "tower_pick" else 0)
    npick = N if seen < 0 else max(1, min(N, seen + seen // 8 + 8))
    tw = 21 if pick == 21 else lookup(groups, npick)
    if tw == 21 and off != "fr_on" and groups == 1 and pick == 0 and off != "fr_kbg" and off != "needy_on" and seen > 0:
        wgs = (seen + tb8 - 1) // tb8
        rounds, bg = (wgs + cu - 1) // cu, (max(needy, 0) * apad + 255) // 256
        if wgs > rounds * (cu - bg) - 14:
            tw = 20
    first = cu * tb8
    mixed = tw == 21 and off != "tower_mixed" and pick == 0 and N > first and seen > first and seen + 16 <= first + cu * tb7
    return tw, int(mixed), int(off != "bg_signal" and tw in (19, 20, 21))


def test_wave_rules(driver):
    table, facts = sweeps(golden_lines())
    lookup = lambda groups, n: at(table["A ConnectFour F=64 bf16=0 groups=%d cu=256" % groups], n)[0]
    tb8, tb7 = (int(facts[("ConnectFour", 64, i, 0)]["TB"]) for i in (21, 19))
    lines = driver("wave")
    assert lines[0].split()[:2] == ["D", "APAD=8"]
    got, _ = sweeps(lines[1:])
    assert len(got) == 8 * 5
    seen_20 = seen_mixed = 0
    for off in ("none", "fr_on", "groups", "fr_kbg", "tower_pick", "tower_mixed", "bg_signal", "needy_on"):
        for needy in (-1, 0, 64, 256, 1024):
            points = got["D off=%s needy=%d" % (off, needy)]
            want, last = [], None
            for seen in range(-1, 4097):
                now = restate_wave(seen, needy, off, lookup, tb8, tb7, 8)
                if now != last:
                    want.append((seen,) + now)
                    last = now
            assert points == want, (off, needy)
            seen_20 += any(p[1] == 20 for p in points)
            seen_mixed += any(p[2] for p in points)
    assert seen_20 and seen_mixed                                   # the sweep reaches both rules
    # by hand: every gate on, no background workgroups: beyond 2 x 256 - 14 = 498 workgroups of 8 boards the 176-register form; two
    # background workgroups (64 slots x 8 words / 256) take one CU each per round: beyond 2 x 254 - 14 = 494.  The mixed launch
    # from the paired form's first size above 2048 boards to 2048 + 256 x 7 - 16
    assert at(got["D off=none needy=0"], 3984) == (21, 0, 1) and at(got["D off=none needy=0"], 3985) == (20, 0, 1)
    assert at(got["D off=none needy=64"], 3952) == (21, 0, 1) and at(got["D off=none needy=64"], 3953) == (20, 0, 1)
    assert at(got["D off=none needy=0"], 3824) == (21, 1, 1) and at(got["D off=none needy=0"], 3825) == (21, 0, 1)


def restate_heads(pick, hd16, hd, n, groups, cu):
    small = pick == 16 or (pick != 32 and (n <= 1024 or groups == 1))
    tiles = (n + 15) // 16
    if hd16 and small and 2 * tiles <= (cu if cu > 0 else 256):
        return 0
    if hd16 and small:
        return 1
    return 2 if hd else 3


def test_heads_choice(driver):
    got, _ = sweeps(driver("heads"))
    assert len(got) == 3 * 2 * 2 * 2 * 3
    for pick in (0, 16, 32):
        for hd16 in (0, 1):
            for hd in (0, 1):
                for groups in (1, 2):
                    for cu in (256, 64, 0):
                        want, last = [], None
                        for n in range(1, 4201):                    # past 1024 and past 2 * tiles = cus (2048 boards at 256 CUs, 512 at 64)
                            k = restate_heads(pick, hd16, hd, n, groups, cu)
                            if k != last:
                                want.append((n, k))
                                last = k
                        assert got["E heads_pick=%d hd16_ok=%d hd_ok=%d groups=%d cu=%d" % (pick, hd16, hd, groups, cu)] == want
    assert got["E heads_pick=0 hd16_ok=1 hd_ok=1 groups=2 cu=256"] == [(1, 0), (1025, 2)]
    assert got["E heads_pick=0 hd16_ok=1 hd_ok=1 groups=1 cu=256"] == [(1, 0), (2049, 1)]
