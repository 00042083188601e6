"""The exact networks of tests/exact_nets.py, checked without a GPU: that their bf16 arithmetic really is exact, that the blob
and the emulation agree with the CPU oracle's fp32 forward, and that the comparison tests/test_net_bf16_exact_gpu.py makes
(device vs emulation within TOL = 1e-5) has the power it claims: every single dropped tap, shifted skip, misplaced weight
or wrong rounding moves the emulation's own P or V by at least 10 x TOL -- errors that the 1.5e-2 bound of
tests/test_net_bf16_gpu.py lets pass.

Smallest effects measured (the larger of max|dP| and max|dV| over the 64 boards; printed by the tests -- figures, not bounds:
the bound is 10 x TOL):
  dropped tap, every layer x every tap that can be on the board, border classes rotating:
      c4-10x128 1.8e-2 / 7.6e-3 (seed 0 / 1), c4-5x64 8.4e-3 / 9.8e-3, go9-10x128 7.7e-3 / 9.8e-3, ttt 5.3e-2 / 7.3e-2 (64 / 128),
      mancala 3.3e-2 / 3.6e-2, the twelve dense-layer networks 1.1e-3 .. 2.6e-2
  skip connection shifted by one cell, every block: >= 4.3e-2;  one weight at the neighbouring input channel, every layer: >= 4.4e-3
  rounding leg: truncation 2.4e-3 / 3.2e-3 (64 / 128 filters), half away from zero 1.0e-3 / 1.1e-3, unrounded skip 7.7e-4 / 7.7e-4
With purely random wiring (no guarantee that every channel has a reader) and 2 weights per output channel, a tenth of these
mutations had NO effect at all: the wiring of exact_nets._ternary and the weight counts in CONFIGS are what this test demands."""
import numpy as np
import pytest
import torch

import azref as R
import exact_nets as E
from test_net import TOL

NAMES = sorted(E.CONFIGS)
NMUT = E.NBOARDS                                    # the whole batch: what every GPU case sends to every form


@pytest.mark.parametrize("name", NAMES)
def test_construction_is_exact_and_alive(name):
    """Conditions, not measurements: a seed that violates one is replaced in CONFIGS, never tolerated."""
    game, hp, blob, X, A, keys = E.build(name)
    P, V, acts, stats = E.reference(name)
    print(name, "max activation per layer", [int(s[1]) for s in stats], "active share %.2f .. %.2f" % (min(s[2] for s in stats), max(s[2] for s in stats)))
    assert [s[0] for s in stats] == [0] * len(stats)                 # bf16 rounding changes NO stored activation
    assert max(s[1] for s in stats) <= 255                           # integers up to 256 are exact in bf16; partial sums < 9 * 128 * 255 < 2^24
    assert all(float(a.frac().abs().max()) == 0.0 for a in acts)
    assert min(s[2] for s in stats) >= 0.15                          # no layer has died
    out = acts[-1].flatten(1).numpy()
    assert len({o.tobytes() for o in out}) == len(out)               # no two boards share a tower output
    assert np.median(P.max(1)) < 0.5 and np.abs(V).max() < 0.9       # heads not saturated
    assert np.all(P[A == 0] == 0) and np.allclose(P.sum(1), 1, atol=1e-5)
    assert keys is None or len({tuple(k) for k in keys.tolist()}) == len(keys)


@pytest.mark.parametrize("name", NAMES)
def test_fp32_oracle_agrees_with_the_emulation(name):
    """Nothing rounds in the tower, so the fp32 forward and the bf16 scheme coincide: the blob layout (Julia shapes, flipped
    kernels) and the emulation are held to an implementation that is already trusted."""
    game, hp, blob, X, A, _ = E.build(name)
    P, V = E.reference(name)[:2]
    Pr, Vr, _ = R.net_forward_normalized(game, (hp.num_blocks, hp.num_filters, 32, 32), blob, X, A)
    print(name, "fp32 oracle vs emulation dP %.2e dV %.2e" % (np.abs(P - Pr).max(), np.abs(V - Vr).max()))
    assert np.abs(P - Pr).max() < TOL and np.abs(V - Vr).max() < TOL


def border_class(y, x, H, W):
    return ("interior", "edge", "corner")[(y in (0, H - 1)) + (x in (0, W - 1))] if H > 1 else ("edge", "corner")[x in (0, W - 1)]


def tap_mutations(H, W, nlayers, rng):
    """per layer: every tap that can be on the board, at a cell whose border class rotates with the tap, so that every
    class (corner, edge, interior -- those the geometry has) occurs with some tap in every layer"""
    cells = {}
    for y in range(H):
        for x in range(W):
            cells.setdefault(border_class(y, x, H, W), []).append((y, x))
    classes = sorted(cells)
    out = []
    for layer in range(nlayers):
        seen = set()
        for t in range(9):
            ky, kx = divmod(t, 3)
            for c in range(len(classes)):
                cls = classes[(t + layer + c) % len(classes)]
                ok = [(y, x) for y, x in cells[cls] if 0 <= y + ky - 1 < H and 0 <= x + kx - 1 < W]
                if ok:
                    y, x = ok[int(rng.integers(len(ok)))]
                    out.append(("tap", layer, ky, kx, y, x))
                    seen.add(cls)
                    break
        assert seen == set(classes), (layer, seen)
    return out


def telling_weight(p, hp, base, k):
    """(co, ci, kx) of a middle-row weight of layer k >= 1 whose misplacement at input channel ci ^ 1 must show: the input
    channels ci and ci ^ 1 differ most, the output channel varies most (some channels are constant over a batch)"""
    w = E._torch_w(p[E._layer_names(hp)[k][0] + ".W"])[:, :, 1, :]
    x, out = base[k - 1], base[k]
    d = (x - x[:, torch.arange(x.shape[1]) ^ 1]).abs().mean((0, 2, 3))
    score = out.std((0, 2, 3)).view(-1, 1) * d.view(1, -1) * (w != 0).any(2)
    co, ci = divmod(int(torch.argmax(score)), x.shape[1])
    assert score[co, ci] > 0
    return co, ci, int(torch.nonzero(w[co, ci])[0])


@pytest.mark.parametrize("name", NAMES)
def test_every_injected_error_moves_the_reference(name):
    game, hp, blob, X, A, _ = E.build(name)
    p = E.params64(game, hp, blob)
    X, A = X[:NMUT], A[:NMUT]
    base, _ = E.tower_bf16(p, hp, X)
    P0, V0 = E.heads_bf16(p, base[-1], A)
    H, W = X.shape[2:]
    nlayers = 2 * hp.num_blocks + 1
    muts = tap_mutations(H, W, nlayers, np.random.default_rng(1))
    assert {m[1] for m in muts} == set(range(nlayers)) and {(m[2], m[3]) for m in muts} >= {(1, kx) for kx in range(3)}
    assert H == 1 or {(m[1], m[2], m[3]) for m in muts} == {(k, ky, kx) for k in range(nlayers) for ky in range(3) for kx in range(3)}
    muts += [("skip", b) for b in range(hp.num_blocks)] + [("chan", k) + telling_weight(p, hp, base, k) for k in range(1, nlayers)]
    small = {}
    for m in muts:
        acts, _ = E.tower_bf16(p, hp, X, mutate=m, base=base)
        P, V = E.heads_bf16(p, acts[-1], A)
        eff = max(np.abs(P - P0).max(), np.abs(V - V0).max())
        small[m[0]] = min(small.get(m[0], np.inf), eff)
        assert eff >= 10 * TOL, (m, eff)
    print(name, "smallest effect of", len(muts), "injected errors:", {k: "%.1e" % v for k, v in small.items()})


# ---------------------------------------------------------------------------------------------------- rounding leg
@pytest.mark.parametrize("F", [64, 128])
def test_rounding_leg_sees_the_rounding_mode_and_the_skip(F):
    game, hp, blob, X, A, _ = E.rounding_net(F)
    p = E.params64(game, hp, blob)
    acts, raw = E.tower_bf16(p, hp, X)
    stem = set(acts[0].unique().tolist())
    assert {256.0, 260.0, 258.0, 1.0, 3.0, 0.0} == stem, stem        # 257 -> 256 and 259 -> 260 (ties to even), 257.5 -> 258, 1 + 2^-8 -> 1
    assert E.tower_stats(acts, raw)[0][0] > 0                        # the stem's store does round
    out = set(acts[2].unique().tolist())
    assert out == {0.0, 512.0, 520.0, 516.0, 2.0, 6.0}, out          # even channels: skip - stored = 0; odd: twice the stored value
    P0, V0 = E.heads_bf16(p, acts[-1], A)
    assert np.median(P0.max(1)) < 0.5 and np.abs(V0).max() < 0.9
    for what, kw in (("truncation", dict(rnd=E.bf16_trunc)), ("half away from zero", dict(rnd=E.bf16_half_away)), ("unrounded skip", dict(skip_unrounded=True))):
        P, V = E.torch_forward_bf16(game, hp, blob, X, A, **kw)
        eff = max(np.abs(P - P0).max(), np.abs(V - V0).max())
        print("rounding leg F = %d, %s: moves the output by %.2e" % (F, what, eff))
        assert eff >= 10 * TOL, (what, eff)


def test_wrong_roundings_are_what_they_say():
    x = torch.tensor([257.0, 259.0, 257.5, 1.0 + 2.0 ** -8, -257.0, -259.0, 3.0], dtype=torch.float64)
    assert E.bf16(x).tolist() == [256.0, 260.0, 258.0, 1.0, -256.0, -260.0, 3.0]
    assert E.bf16_trunc(x).tolist() == [256.0, 258.0, 256.0, 1.0, -256.0, -258.0, 3.0]
    assert E.bf16_half_away(x).tolist() == [258.0, 260.0, 258.0, 1.0 + 2.0 ** -7, -258.0, -260.0, 3.0]
