"""CPU: the restatement tests/cut_pursuit_ref.py against definitions that need no algorithm.

* the min cut against the enumeration of all 2^V labellings (V <= 12): the value is the minimum, and the sink side is
  the smallest sink side among the minimisers (the intersection of all of them, itself a minimiser);
* the locally dominant matching against the sequential sorted walk on random gains with ties and gains <= 0;
* the random stream, the scale rule and the canonical ids, which the device has to reproduce bit for bit.
"""
import numpy as np
import pytest

import cut_pursuit_ref as cp


def _enumerate(src, snk, arc, cap):
    V = len(src)
    sides = ((np.arange(2 ** V)[:, None] >> np.arange(V)) & 1).astype(bool)              # [2^V, V], True = sink side
    value = (sides * src.astype(np.int64)).sum(1) + (~sides * snk.astype(np.int64)).sum(1)
    for t, h, c in zip(arc["tail"], arc["head"], cap):
        value = value + (~sides[:, t] & sides[:, h]) * int(c)
    best = value.min()
    return best, sides[value == best]


@pytest.mark.parametrize("seed", range(40))
def test_min_cut_is_the_smallest_sink_side_of_a_minimum_cut(seed):
    rng = np.random.default_rng(seed)
    V = int(rng.integers(1, 13))
    src, snk, source, target, cap = cp.random_network(V, int(rng.integers(0, 4)), int(rng.integers(0, 6)),
                                                      int(rng.integers(0, 3)), int(rng.integers(1, 5)), seed)
    arc = cp.arcs(source, target, V)
    cap = cap[arc["arc"]]
    side, value = cp.min_cut(src, snk, arc, cap)
    best, minimisers = _enumerate(src, snk, arc, cap)
    assert value == best == cp.cut_value(src, snk, arc, cap, side)
    assert np.array_equal(side.astype(bool), minimisers.all(0))


def test_min_cut_minimisers_are_not_all_unique():
    """the enumeration test means something only if some networks have several minimum cuts"""
    several = 0
    for seed in range(40):
        rng = np.random.default_rng(seed)
        V = int(rng.integers(1, 13))
        src, snk, source, target, cap = cp.random_network(V, int(rng.integers(0, 4)), int(rng.integers(0, 6)),
                                                          int(rng.integers(0, 3)), int(rng.integers(1, 5)), seed)
        arc = cp.arcs(source, target, V)
        several += len(_enumerate(src, snk, arc, cap[arc["arc"]])[1]) > 1
    assert several >= 5


@pytest.mark.parametrize("seed", range(30))
def test_locally_dominant_matching_is_the_sequential_walk(seed):
    rng = np.random.default_rng(100 + seed)
    C = int(rng.integers(2, 40))
    B = int(rng.integers(1, 4 * C))
    a = rng.integers(0, C - 1, B)
    b = a + 1 + rng.integers(0, C - 1 - a)                      # a < b < C; pairs may repeat
    gain = rng.integers(-2, 5, B).astype(np.float64) * 0.25     # many ties, some <= 0
    taken, rounds = cp.merge_rounds(a, b, gain, C)
    assert np.array_equal(taken, cp.merge_sequential(a, b, gain, C))
    assert not taken[gain <= 0].any() and rounds <= B
    ends = np.concatenate([a[taken], b[taken]])
    assert len(np.unique(ends)) == len(ends)


def test_random_stream_and_scale_rule():
    assert cp.mix(0) == 0
    draws = [cp.draw(0, 1, r, 0, k) for r in range(2) for k in range(2)]
    assert len(set(draws)) == 4 and all(0 <= d <= cp.M32 for d in draws)
    assert cp.draw(7, 3, 2, 11, 1) != cp.draw(7, 3, 2, 12, 1)
    for largest, want in ((0.0, 1.0), (1.0, 2.0 ** -29), (0.75, 2.0 ** -30), (2.0 ** 29, 1.0), (2.0 ** 30 - 1, 1.0),
                          (2.0 ** 30, 2.0), (3e-3, 2.0 ** -38)):
        s = cp.scale_of(largest)
        assert s == want and (largest == 0 or 2 ** 29 <= largest / s < 2 ** 30)


def test_quantize_keeps_integers_and_stays_within_half_a_step():
    rng = np.random.default_rng(3)
    term = rng.integers(-2 ** 24 + 1, 2 ** 24, 500).astype(np.float64)
    term[0] = 2.0 ** 29
    w = rng.integers(0, 2 ** 24, 300).astype(np.float32)
    arc_edge = np.concatenate([np.arange(300), np.arange(300)])
    src, snk, cap, s = cp.quantize(term, w, None, 1.0, arc_edge)
    assert s == 1.0
    assert np.array_equal(src.astype(np.float64) - snk, term) and np.array_equal(cap[:300].astype(np.float32), w)
    term, w = rng.normal(0, 3, 500), rng.random(300).astype(np.float32)
    src, snk, cap, s = cp.quantize(term, w, None, 0.03, arc_edge)
    assert np.frexp(s)[0] == 0.5
    assert np.abs((src.astype(np.float64) - snk) * s - term).max() <= s / 2
    assert np.abs(cap[:300] * s - 0.03 * w.astype(np.float64)).max() <= s / 2


def test_canonical_ids_and_energy():
    comp, C = cp.canonical(np.array([5, 5, 2, 9, 2, 5]))
    assert C == 3 and comp.tolist() == [0, 0, 1, 2, 1, 0]
    f = np.array([[0.0], [2.0], [10.0]], dtype=np.float32)
    fid, pen = cp.energy(f, [0, 1, 1], [1, 2, 2], np.array([1.0, 2.0, 4.0], np.float32), 0.5, [0, 0, 1])
    assert fid == 1.0 and pen == 3.0
