"""The AZHIP_* overrides of libazhip.so (csrc/env.h), without a GPU and without the library.
  * static: env.h is the only file of csrc/ that calls getenv; the names inside struct EnvCreate are azhip.engine.CREATE_ENV (the
    engine cache's key); the names of the file are the rows of DESIGN.md's override table, and the reverse;
  * semantics: tests/env_driver.cpp (host compiler, env.h only) prints the filled structs; every override is run unset, at a
    typical value and at its edge values.  The expected values were worked out from the readers these structs replaced (the
    table of DESIGN.md states the same rules), not from env.h."""
import glob
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "alphazero.jl_amd", "csrc")
ENV_H = re.sub(r"//.*", "", open(os.path.join(CSRC, "env.h")).read())          # code only: the comments name overrides too


def names_in(code):
    return set(re.findall(r'"(AZHIP_[A-Z0-9_]+)"', code))


def read_at(moment):
    """the names inside `struct Env<Moment> { ... };`: a member's initialiser is its reader"""
    m = re.search(r"^struct Env%s \{(.*?)^\};" % moment.capitalize(), ENV_H, flags=re.S | re.M)
    assert m, moment
    return names_in(m.group(1))


def test_env_h_is_the_only_reader_of_the_environment():
    files = glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h"))
    assert len(files) >= 15
    for f in files:
        if os.path.basename(f) != "env.h":
            assert "getenv" not in open(f).read(), f
    incs = re.findall(r"#include\s+(\S+)", ENV_H)
    assert incs and all(re.fullmatch(r"<c[a-z]+>", i) for i in incs), incs       # plain C++: a host compiler builds it alone (the driver below)


def test_creation_time_names_are_the_engine_cache_key():
    from azhip import engine as E
    create = read_at("create")
    assert len(create) == 17 and "AZHIP_EXPLORE_K" in create
    assert create == set(E.CREATE_ENV) and len(E.CREATE_ENV) == len(set(E.CREATE_ENV))
    moments = ("create", "phase", "process", "arena", "trainer", "comm")
    by_moment = [read_at(m) for m in moments]
    assert all(by_moment) and sum(len(s) for s in by_moment) == len(set().union(*by_moment))   # every name is read at one moment only
    assert set().union(*by_moment) == names_in(ENV_H)                           # ... and inside one of the structs


def test_design_md_lists_every_override_and_no_other():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    start = design.index("**Environment overrides.**")
    rows = re.findall(r"^\| `(AZHIP_[A-Z0-9_]+)` \|([^|]*)\|([^|]*)\|([^|]*)\|([^|]*)\|$", design[start:], flags=re.M)
    table = [r[0] for r in rows]
    assert len(table) == len(set(table)) and set(table) == names_in(ENV_H), set(table) ^ names_in(ENV_H)
    when = {"create": "az_engine_create", "phase": "az_selfplay_begin", "process": "once per process", "arena": "az_arena_run",
            "trainer": "az_trainer_create", "comm": "first az_comm"}
    for name, _, _, read, _ in rows:                                            # the "when read" column agrees with the reader that holds the name
        moment = [m for m in when if name in read_at(m)]
        assert len(moment) == 1 and when[moment[0]] in read, (name, read)


# ---------------------------------------------------------------------------------------------------------------- semantics
DEFAULTS = dict(tower_pick="0", tower_mixed="0", heads_pick="0", use_graphs="0", tree_sort="0", bk_mode="0", explore_k="8",
                xch_fail_at="0", xch_epoch0="0", pooled_queue="0", tag_mask="65535", epoch0="1", vmm="-1", vmm_keys="1",
                eval_cache="-1", eval_cache_log2="0", pool_gb="-1",
                free_run="-1", run_k="3", run_kbg="-1", round_waves="128", bg_stop="1", bg_prio="0", trace="0",
                fin_inside="0", conv_nt6="1", one_stream="0", wg_late="0", rccl_lib="(null)")
# (variable, value, field, expected): -1 in vmm / eval_cache / free_run / run_kbg / pool_gb and 0 in eval_cache_log2 mean "unset, decided at the point of use"
CASES = [
    ("AZHIP_TOWER", "16", "tower_pick", 16), ("AZHIP_HEADS", "32", "heads_pick", 32), ("AZHIP_GRAPH", "1", "use_graphs", 1),
    ("AZHIP_TOWER_MIXED", "1", "tower_mixed", 1), ("AZHIP_TOWER_MIXED", "0", "tower_mixed", 0),
    ("AZHIP_TREE_SORT", "1", "tree_sort", 1), ("AZHIP_TREE_SORT", "0", "tree_sort", 0),
    ("AZHIP_TREE_ATOMIC", "1", "bk_mode", 1), ("AZHIP_TREE_ATOMIC", "2", "bk_mode", 2), ("AZHIP_TREE_ATOMIC", "3", "bk_mode", 0),
    ("AZHIP_EXPLORE_K", "1", "explore_k", 1), ("AZHIP_EXPLORE_K", "0", "explore_k", 0), ("AZHIP_EXPLORE_K", "12", "explore_k", 12),
    ("AZHIP_XCH_FAIL_AT", "5", "xch_fail_at", 5), ("AZHIP_XCH_FAIL_AT", "5000000000", "xch_fail_at", 5000000000),
    ("AZHIP_XCH_EPOCH0", "12", "xch_epoch0", 12), ("AZHIP_XCH_EPOCH0", "0xfffff0", "xch_epoch0", 0xfffff0),
    ("AZHIP_POOLED_QUEUE", "1", "pooled_queue", 1), ("AZHIP_POOLED_QUEUE", "0", "pooled_queue", 1), ("AZHIP_POOLED_QUEUE", "", "pooled_queue", 1),
    ("AZHIP_HT_TAG_BITS", "4", "tag_mask", 15), ("AZHIP_HT_TAG_BITS", "0", "tag_mask", 0), ("AZHIP_HT_TAG_BITS", "1", "tag_mask", 1),
    ("AZHIP_HT_TAG_BITS", "16", "tag_mask", 0xffff), ("AZHIP_HT_TAG_BITS", "99", "tag_mask", 0xffff), ("AZHIP_HT_TAG_BITS", "-3", "tag_mask", 0),
    ("AZHIP_HT_EPOCH0", "65000", "epoch0", 65000), ("AZHIP_HT_EPOCH0", "0", "epoch0", 1), ("AZHIP_HT_EPOCH0", "65534", "epoch0", 65534),
    ("AZHIP_HT_EPOCH0", "65535", "epoch0", 1),
    ("AZHIP_VMM", "1", "vmm", 1), ("AZHIP_VMM", "0", "vmm", 0), ("AZHIP_VMM_KEYS", "1", "vmm_keys", 1), ("AZHIP_VMM_KEYS", "0", "vmm_keys", 0),
    ("AZHIP_EVAL_CACHE", "1", "eval_cache", 1), ("AZHIP_EVAL_CACHE", "0", "eval_cache", 0),
    ("AZHIP_EVAL_CACHE_LOG2", "20", "eval_cache_log2", 20), ("AZHIP_EVAL_CACHE_LOG2", "1", "eval_cache_log2", 4),
    ("AZHIP_EVAL_CACHE_LOG2", "40", "eval_cache_log2", 28),
    ("AZHIP_FREE_RUN", "1", "free_run", 1), ("AZHIP_FREE_RUN", "0", "free_run", 0),
    ("AZHIP_RUN_K", "5", "run_k", 5), ("AZHIP_RUN_K", "0", "run_k", 1),
    ("AZHIP_RUN_KBG", "16", "run_kbg", 16), ("AZHIP_RUN_KBG", "0", "run_kbg", 0), ("AZHIP_RUN_KBG", "-1", "run_kbg", 0),
    ("AZHIP_FR_ROUND", "64", "round_waves", 64), ("AZHIP_FR_ROUND", "0", "round_waves", 1),
    ("AZHIP_BG_STOP", "0", "bg_stop", 0), ("AZHIP_BG_STOP", "1", "bg_stop", 1), ("AZHIP_BG_PRIO", "3", "bg_prio", 3),
    ("AZHIP_TRACE_ARENA", "1", "trace", 1), ("AZHIP_TRACE_ARENA", "0", "trace", 1),
    ("AZHIP_TRAIN_FINISH_INSIDE", "1", "fin_inside", 1), ("AZHIP_TRAIN_FINISH_INSIDE", "0", "fin_inside", 0),
    ("AZHIP_TRAIN_ONE_STREAM", "1", "one_stream", 1), ("AZHIP_TRAIN_ONE_STREAM", "0", "one_stream", 0),
    ("AZHIP_TRAIN_WG_LATE", "1", "wg_late", 1), ("AZHIP_TRAIN_WG_LATE", "0", "wg_late", 0),
    ("AZHIP_TRAIN_NT6", "1", "conv_nt6", 1), ("AZHIP_TRAIN_NT6", "0", "conv_nt6", 0),
    ("AZHIP_POOL_GB", "2", "pool_gb", 2), ("AZHIP_POOL_GB", "0.5", "pool_gb", 0.5), ("AZHIP_POOL_GB", "0", "pool_gb", 0),
    ("AZHIP_RCCL_LIB", "/tmp/librccl_stub.so", "rccl_lib", "/tmp/librccl_stub.so"),
]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("env") / "env_driver")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "env_driver.cpp"), "-o", exe])

    def run(**env):
        base = {k: v for k, v in os.environ.items() if not k.startswith("AZHIP_")}
        out = subprocess.run([exe], env=dict(base, **env), capture_output=True, text=True, check=True).stdout
        return dict(line.split("=", 1) for line in out.splitlines())
    return run


def test_unset_environment_gives_the_defaults(driver):
    assert driver() == DEFAULTS


def test_every_override_has_a_case():
    assert {c[0] for c in CASES} == names_in(ENV_H)


@pytest.mark.parametrize("var,value,field,want", CASES, ids=["%s=%s" % c[:2] for c in CASES])
def test_override_semantics(driver, var, value, field, want):
    assert driver(**{var: value}) == dict(DEFAULTS, **{field: str(want)})          # ... and no other field moves
