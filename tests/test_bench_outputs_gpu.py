"""A plain `bench.py --gpus 1 --steps K --warmup W` run is the headline alone, and `--dump-outputs DIR` writes the same arrays for
the same arguments run after run: two runs at 512 slots, their lines and their files compared."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("extra", "cpu_baseline", "value_long", "value_cache_off", "value_lock_step", "roofline_kernel_alone", "roofline_tree",
             "summary", "phase", "learning", "gather")


def _run(out_dir):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "3", "--slots", "512",
                        "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=300, cwd=ROOT)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0 and len(lines) == 1, r.stdout[-2000:] + r.stderr[-2000:]
    return json.loads(lines[0]), {f[:-4]: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))}


def test_plain_run_is_the_headline_and_its_outputs_repeat(tmp_path):
    a, da = _run(tmp_path / "a")
    b, db = _run(tmp_path / "b")
    for d in (a, b):
        assert d["steps"] == 7 and d["ms_per_step"] > 0 and d["value"] > 0 and d["unit"] == "sims/s"
        assert d["higher_is_better"] is True and d["dtype"] == "f32" and d["full"] is False
        assert not [k for k in FULL_ONLY if k in d], sorted(d)
    assert sorted(da) == sorted(a["dump_outputs"]["files"][i][:-4] for i in range(len(a["dump_outputs"]["files"])))
    assert all(x.dtype in (np.float32, np.float64) for x in da.values())
    assert 0 < sum(x.nbytes for x in da.values()) <= 64 << 20
    assert a["dump_outputs"]["game_ids"] == b["dump_outputs"]["game_ids"] and a["dump_outputs"]["games"] == 256
    n = len(da["move_key"])
    assert n == da["game_num_moves"].sum() and da["move_policy"].shape == (n, 7)
    assert np.allclose(da["move_policy"].sum(axis=1), 1.0, atol=1e-5) and np.all(np.abs(da["move_value"]) <= 1.0)
    # every move of a game is 400 simulations of that game's explore!: the root's visits of the 7 columns
    assert np.all(da["move_visits"][:, :7].sum(axis=1) >= 399)
    assert sorted(da) == sorted(db)
    for k in da:
        assert da[k].dtype == db[k].dtype and np.array_equal(da[k], db[k]), k
