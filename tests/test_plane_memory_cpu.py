"""The numpy restatement of merge_by_state over (X, A) rows that tests/test_plane_memory_gpu.py trusts, held to the oracle's
merge_by_state (oracle/azref.py) on Tic-tac-toe samples: there vectorize_state is injective, so rows and state keys are in bijection
and both groupings must be the same, with the same Float64 sums."""
import numpy as np

import azref as R
import test_plane_memory_gpu as G


def _positions(ngames, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(ngames):
        g = R.Game(R.TTT)
        while not g.terminated():
            out.append((g.key(), g.vectorize().reshape(3, 3, 3), g.actions_mask().astype(np.float32)))
            g.play(rng.choice(g.available_actions()))
    return [out[i] for i in rng.permutation(len(out))]


def test_row_restatement_is_the_oracle_s_merge_by_state():
    pos = _positions(60, seed=3)
    rng = np.random.default_rng(4)
    n = len(pos)
    row_of_key, key_of_row = {}, {}
    samples, rows = [], []
    for key, X, A in pos:
        row = X.tobytes() + A.tobytes()
        assert row_of_key.setdefault(key, row) == row and key_of_row.setdefault(row, key) == key       # a bijection
        pi = rng.random(9) * A
        pi /= pi.sum()
        z, t, nv = rng.uniform(-1, 1), float(rng.integers(1, 10)), int(rng.integers(1, 300))
        e = R.Sample()
        e.key[0], e.key[1] = key
        for a in range(9):
            e.pi[a] = pi[a]
        e.z, e.t, e.n = z, t, nv
        samples.append(e)
        rows.append((X, A, pi, z, t, nv))
    assert len(row_of_key) < 0.8 * n                                 # repeated positions: there is something to merge
    want = {(int(e.key[0]), int(e.key[1])): e for e in R.merge_by_state(R.TTT, samples)}
    got = G.ref_merge(rows)
    assert len(got) == len(want) == len(row_of_key)
    first_seen = list(dict.fromkeys(key for key, _, _ in pos))
    for k, (X, A, pi, z, t, nv) in enumerate(got):
        key = key_of_row[X.tobytes() + A.tobytes()]
        assert key == first_seen[k]                                  # rows come out in order of first occurrence
        e = want[key]
        assert np.array_equal(np.array(e.pi[:9]).view(np.uint64), pi.view(np.uint64))
        assert (np.float64(e.z).tobytes(), np.float64(e.t).tobytes(), e.n) == (np.float64(z).tobytes(), np.float64(t).tobytes(), nv)
    # convert_samples' P and V are the oracle's for these rows (CONSTANT and LINEAR weights; LOG is pinned on the device against the keyed path)
    order = [want[key_of_row[X.tobytes() + A.tobytes()]] for X, A, *_ in got]
    for policy in (G.CONSTANT, G.LINEAR):
        for name, a, b in zip("WXAPV", G.ref_convert(got, policy), R.convert_samples(R.TTT, policy, order)):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (policy, name)


def test_ref_memory_is_a_circular_buffer_with_the_reference_s_batch_count():
    """memory.jl:35-65 on numbers small enough to follow by hand"""
    m = G.RefMemory(5)
    X, A = np.zeros((4, 3, 3, 3), dtype=np.float32), np.ones((4, 9), dtype=np.float32)
    P = np.full((4, 9), 1 / 9)
    m.push_trace(X, A, P, [0, 0, 0, 1.0], [1, 0, 1, 0], 0.5)
    assert [e[3] for e in m.get_experience()] == [-1.0, 0.5, -0.25, 0.125] and [e[4] for e in m.get_experience()] == [1.0, 2.0, 3.0, 4.0]
    assert (len(m), m.cur_batch_size()) == (4, 4)
    m.push_trace(X, A, P, [0, 0, 0, -1.0], [1, 1, 0, 1], 1.0)       # a free turn: white moves twice
    assert (len(m), m.cur_batch_size()) == (5, 5)
    assert [e[3] for e in m.get_experience()] == [0.125, -1.0, 1.0, -1.0, -1.0]
    m.cur = 0
    m.push(X[0], A[0], P[0], 0.0, 1.0, 3)
    assert m.cur_batch_size() == 0 and m.last_batch() == [] and m.get_experience()[-1][5] == 3
