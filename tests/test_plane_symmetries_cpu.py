"""What tests/test_plane_symmetries_gpu.py trusts, held to the oracle without a device: its numpy gather of the symmetric images
(gather_images) under the tables of azhip.plane_symmetries must be the oracle's augment_with_symmetries (oracle/azref.py,
memory.jl:114-130) followed by the oracle's encoding -- row for row, in the order n0 + i * nsym + k -- on real Tic-tac-toe and
Connect Four positions; and the Go tables, which no oracle game stands behind, must be the dihedral group acting on the 9 x 9 cells."""
import numpy as np
import pytest

import azref as R
import test_plane_symmetries_gpu as S

REF = {S.TTT: R.TTT, S.C4: R.C4}


def _encode(game, key):
    g = R.Game(REF[game], R.unpack_key(REF[game], key))
    return g.vectorize().reshape(S.DIMS[game]), g.actions_mask().astype(np.float32)


def _samples(game, ngames, seed):
    """oracle TrainingSamples of random games and the same samples as plane samples (X, A, pi, z, t, n)"""
    rng = np.random.default_rng(seed)
    nA = S.NUM_ACTIONS[game]
    es, rows = [], []
    for _ in range(ngames):
        g = R.Game(REF[game])
        while not g.terminated():
            key = g.key()
            X, A = _encode(game, key)
            pi = rng.random(nA) * A
            pi /= pi.sum()
            e = R.Sample()
            e.key[0], e.key[1] = key
            for a in range(nA):
                e.pi[a] = pi[a]
            e.z, e.t, e.n = rng.uniform(-1, 1), float(rng.integers(1, 10)), int(rng.integers(1, 300))
            es.append(e)
            rows.append((X, A, pi, e.z, e.t, e.n))
            g.play(rng.choice(g.available_actions()))
    cols = list(zip(*rows))
    return es, (np.stack(cols[0]), np.stack(cols[1]), np.stack(cols[2]), np.array(cols[3]), np.array(cols[4]), np.array(cols[5], dtype=np.int64))


@pytest.mark.parametrize("game", [S.TTT, S.C4], ids=["ttt", "c4"])
def test_gather_and_tables_are_the_oracle_s_augment_with_symmetries(game):
    import azhip
    xperm, aperm = azhip.plane_symmetries(getattr(azhip, S.SPECS[game])())
    nsym = {S.TTT: 7, S.C4: 1}[game]
    assert xperm.shape == (nsym, int(np.prod(S.DIMS[game]))) and aperm.shape == (nsym, S.NUM_ACTIONS[game]) and xperm.dtype == aperm.dtype == np.int32
    es, s = _samples(game, 12 if game == S.TTT else 4, seed=1)
    n0, nA = len(es), S.NUM_ACTIONS[game]
    want = R.augment_with_symmetries(REF[game], es)
    X, A, P, z, t, n = S.gather_images(xperm, aperm, s)
    assert len(want) == n0 * (1 + nsym) == len(z) and n0 > 60
    moved = 0
    for r, e in enumerate(want):
        eX, eA = _encode(game, (int(e.key[0]), int(e.key[1])))
        assert np.array_equal(eX, X[r]) and np.array_equal(eA, A[r]), r
        assert np.array_equal(np.array(e.pi[:nA]).view(np.uint64), P[r].view(np.uint64)), r
        assert (e.z, e.t, e.n) == (z[r], t[r], n[r]), r
        if r >= n0:
            i = (r - n0) // nsym
            moved += not np.array_equal(X[r], X[i])
    assert moved > 0.5 * n0 * nsym                                   # most images differ from their sample: the comparison has teeth


def test_go_tables_are_the_dihedral_group_on_the_cells():
    import azhip
    xperm, aperm = azhip.plane_symmetries(azhip.Go9PlanesSpec())
    assert xperm.shape == (7, 324) and aperm.shape == (7, 82)
    ident = np.arange(81)
    cell = aperm[:, :81]
    assert np.all(aperm[:, 81] == 81)                                # the pass action is fixed
    for k in range(7):
        assert sorted(xperm[k]) == list(range(324)) and sorted(aperm[k]) == list(range(82))
        for c in range(4):                                           # every plane moves as the cells do
            assert np.array_equal(xperm[k, 81 * c:81 * c + 81], cell[k] + 81 * c)
    group = [tuple(ident)] + [tuple(p) for p in cell]
    assert len(set(group)) == 8
    for p in group:
        for q in group:
            assert tuple(np.array(p)[np.array(q)]) in group          # closed under composition
    # the reference's order (games/tictactoe/game.jl:149-168 at n = 9): rot takes (x, y) to (y, 8 - x), flip to (x, 8 - y)
    at = lambda x, y: y * 9 + x
    assert cell[0][at(0, 0)] == at(0, 8) and cell[1][at(0, 0)] == at(8, 8) and cell[2][at(0, 0)] == at(8, 0)
    assert cell[3][at(2, 0)] == at(2, 8)
    rot, flip = cell[0], cell[3]
    assert np.array_equal(cell[1], rot[rot]) and np.array_equal(cell[2], rot[rot][rot])
    assert np.array_equal(cell[4], flip[rot]) and np.array_equal(cell[5], flip[rot[rot]]) and np.array_equal(cell[6], flip[rot[rot][rot]])
    # the 3 x 3 tables are the same construction: the device twin's (the keyed path) are pinned to these on the GPU
    x3, a3 = azhip.plane_symmetries(azhip.TicTacToeSpec())
    assert x3.shape == (7, 27) and np.array_equal(a3[0], [6, 3, 0, 7, 4, 1, 8, 5, 2])
    xm, am = azhip.plane_symmetries(azhip.MancalaSpec())
    assert xm.shape == (0, 70) and am.shape == (0, 6)


def test_random_tables_are_bijections_that_are_not_involutions():
    for game in (S.TTT, S.MANCALA, S.C4, S.GO9):
        for table in S.random_tables(game, 15, seed=game):
            assert table.dtype == np.int32 and len(table) == 15
            for p in table:
                assert sorted(p) == list(range(len(p))) and not np.array_equal(p[p], np.arange(len(p)))
