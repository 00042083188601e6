"""examples/grid_world_host_stepped.py at a small size: 8 workers, 16 simulations, 2 episodes per worker of at most 30 moves, one
optimiser step at batch 32.  What the chance trees played is what the plane memory holds, with the z of push_trace!'s recursion over
the episode's Float32 rewards; the step's loss is finite; equal seeds give equal traces.  No claim that it learns."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKERS, EPISODES, SIMS, MAX_MOVES, GAMMA = 8, 2, 16, 30, 0.9


@pytest.fixture(scope="module")
def played():
    import azhip
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import grid_world_host_stepped as ex
    gspec = azhip.Go9PlanesSpec()
    nn = azhip.ResNet(gspec, azhip.ResNetHP(num_blocks=1, num_filters=64, num_policy_head_filters=32, num_value_head_filters=32), seed=4)
    runs = [ex.play_episodes(nn, ex.make_rules(gspec, 7, MAX_MOVES), WORKERS, EPISODES, SIMS) for _ in range(2)]
    yield ex, gspec, nn, runs
    nn.gc()


def test_equal_seeds_give_equal_traces(played):
    _, _, _, ((ta, sa), (tb, sb)) = played
    assert len(ta) == len(tb) == WORKERS * EPISODES and sa == sb
    for a, b in zip(ta, tb):
        assert a["worker"] == b["worker"] and a["states"] == b["states"] and a["actions"] == b["actions"]
        assert np.array_equal(np.stack(a["pi"]), np.stack(b["pi"])) and a["rewards"] == b["rewards"]
    assert sa["simulations"] == SIMS * sum(len(t["states"]) for t in ta) and sa["sims_without_host"] == 0
    assert sa["steps"] > sa["simulations"] / WORKERS                    # more than one host round trip per simulation


def test_the_plane_memory_holds_the_moves_played_with_push_trace_s_z(played):
    import azhip
    ex, gspec, nn, ((traces, _), _) = played
    with azhip.PlaneMemoryBuffer(gspec, 4096) as mem:
        ex.push_traces(mem, traces, GAMMA)
        X, A, P, z, t, n = mem.samples()
        assert len(mem) == sum(len(tr["states"]) for tr in traces) == mem.cur_batch_size()
        k = 0
        for tr in traces:
            m = len(tr["states"])
            assert 1 <= m <= MAX_MOVES and all(tr["rewards"][i] == 0 for i in range(m - 1))     # only the last move can pay
            wr = 0.0
            for j, i in enumerate(reversed(range(m))):                   # pushed last position first
                x, y, time = tr["states"][i]
                assert time == i
                want = np.zeros((4, 9, 9), np.float32)
                want[0, y - 1, x - 1] = 1.0
                assert np.array_equal(X[k + j], want) and A[k + j, :4].all() and not A[k + j, 4:].any()
                assert np.array_equal(P[k + j], tr["pi"][i]) and P[k + j, tr["actions"][i]] == P[k + j].max() and abs(P[k + j].sum() - 1) < 1e-12
                wr = GAMMA * wr + float(tr["rewards"][i])                  # push_trace!: Float64 over the Float32 rewards
                assert z[k + j] == wr and t[k + j] == float(m - i) and n[k + j] == 1
            k += m
        nn2, losses = ex.learn(nn, mem, 1, 32)
        assert len(losses) == 1 and np.isfinite(losses).all()
        assert nn2.params().shape == nn.params().shape and np.isfinite(nn2.params()).all() and not np.array_equal(nn2.params(), nn.params())
