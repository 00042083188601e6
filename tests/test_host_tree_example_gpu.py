"""examples/host_stepped_go9 --device-trees: the host-stepped example with its search trees in HBM (az_host_tree_*, engine mode).
The flag is off by default (tests/test_host_stepped_example.py holds the default mode); with it the workers keep only Go states by
node id and answer the tree's requests, and the JSON line names the mode."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "examples", "host_stepped_go9")


def _run(*args):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples")], stdout=subprocess.DEVNULL)
    r = subprocess.run([EXE, *args], capture_output=True, text=True, timeout=120, cwd="/tmp")
    line = next((ln for ln in r.stdout.splitlines() if ln.startswith("{")), None)
    return r, (json.loads(line) if line else None)


def test_device_trees_need_the_gpu_and_say_so():
    r, d = _run("--dry", "--device-trees", "--workers", "32", "--sims", "8", "--seconds", "0.2")
    assert r.returncode == 1 and d is None and "--device-trees" in r.stderr


@pytest.mark.gpu
def test_device_trees_play_whole_moves_and_report_the_mode():
    r, d = _run("--device-trees", "--workers", "128", "--sims", "32", "--seconds", "1", "--tree-gb", "2")
    assert r.returncode == 0, r.stderr
    assert d["mode"] == "device-trees" and d["value"] > 1000 and d["moves"] > 128 and d["kernel"].startswith("k_tower16b<Go9Planes,128")
    assert 32 < d["boards_per_launch"] <= 64                            # two halves of 64 workers take turns; nearly every simulation asks once
    assert d["tree_full_resets"] == 0 and d["tree_kernel_ms_per_step"] > 0 and d["evaluations"] > d["transposition_hits"] >= 0
    assert 0 < d["avg_exploration_depth"] < 40 and 0.0 < d["step_call_share"] <= 1.01
