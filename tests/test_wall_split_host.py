"""CPU: the host side of the S3DIS wall split (inference.get_room_walls) and its numpy oracle (tests/plane_ref.py):
the oracle against a brute-force loop, the plane fit, the seeded sampler, open3d's selection rule, the refusals that
need no device, and the C ABI of the two kernels."""
import ctypes
import math
import os

import numpy as np
import pytest

import plane_ref
import wsis_native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("wsis_plane_score_workspace_bytes", "wsis_plane_score", "wsis_plane_mark")


def test_oracle_matches_a_brute_force_double_loop():
    rng = np.random.default_rng(0)
    xyz = (rng.random((50, 3)) * 2).astype(np.float32)
    planes, valid = plane_ref.planes_from_triples(xyz[plane_ref.draw_triples(50, 7, rng).reshape(-1)].reshape(7, 3, 3))
    assert valid.all()
    thr = 0.3
    count, sumsq, gap = plane_ref.score(xyz, planes, thr)
    want_gap = math.inf
    for h in range(7):
        a, b, c, d = (float(v) for v in planes[h])
        n, s = 0, []
        for i in range(50):
            x, y, z = (float(v) for v in xyz[i])
            dist = abs(((a * x + b * y) + c * z) + d)          # Python floats: IEEE fp64, one rounding per operation
            want_gap = min(want_gap, abs(dist - thr))
            assert bool(plane_ref.mark(xyz, planes[h], thr)[i]) == (dist < thr)
            if dist < thr:
                n += 1
                s.append(dist * dist)
        assert count[h] == n and 3 <= n < 50
        assert sumsq[h] == pytest.approx(math.fsum(s), rel=50 * 2.0 ** -52, abs=0)
    assert gap == want_gap and gap > plane_ref.GAP


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_oracle_on_the_synthetic_rooms_keeps_the_guard_and_finds_the_two_large_walls(seed):
    """5 x 4 x 2.6 m, walls of 11,000 / 7,000 / 5,000 / 3,000 points: two rounds (each wall also takes the corner strips
    of its neighbours and the clutter next to it), then fewer than 10,000 points remain; no distance within GAP of the
    threshold and no shared top count, so the GPU tests may compare masks exactly"""
    xyz = plane_ref.make_room(seed)
    assert xyz.dtype == np.float32 and xyz.shape == (28000, 3)
    walls, info = plane_ref.get_room_walls_ref(xyz, np.ones(len(xyz), bool), max_num=10, seed=100 + seed)
    assert info["gap"] > plane_ref.GAP and info["top_ties"] == 0
    assert len(walls) == 2 and len(info["samples"]) == 2 and not (walls[0] & walls[1]).any()
    assert 11000 <= walls[0].sum() <= 11600 and 6800 <= walls[1].sum() <= 7300
    assert info["remaining"] == 28000 - walls[0].sum() - walls[1].sum() < 10000


def test_plane_fit_unit_normal_through_the_points_and_degenerate_triples():
    import inference
    rng = np.random.default_rng(1)
    pts = rng.random((40, 3, 3)) * 5
    pts[3] = np.array([[0.0, 0.0, 0.0], [1.0, 2.0, 4.0], [2.0, 4.0, 8.0]])      # collinear
    pts[7, 1] = pts[7, 0]                                      # a repeated point
    pts[9] = pts[9, 0]                                         # three times the same point
    pts[11, 2, 1] = np.nan
    for fit in (plane_ref.planes_from_triples, inference.planes_from_triples):
        planes, valid = fit(pts)
        assert planes.shape == (40, 4) and planes.dtype == np.float64
        assert valid.tolist() == [h not in (3, 7, 9, 11) for h in range(40)]
        n = planes[valid, :3]
        assert np.abs(np.sqrt((n * n).sum(1)) - 1).max() <= 4 * 2.0 ** -52
        for h in np.nonzero(valid)[0]:
            assert plane_ref.distances(pts[h], planes[h]).max() <= 1e-12
    assert np.array_equal(plane_ref.planes_from_triples(pts)[0], inference.planes_from_triples(pts)[0])


def test_seeded_sampler_is_reproducible_distinct_and_in_range():
    import inference
    for n in (3, 4, 1000):
        a = inference.sample_triples(n, 200, np.random.default_rng(7))
        b = inference.sample_triples(n, 200, np.random.default_rng(7))
        assert a.shape == (200, 3) and np.array_equal(a, b)
        assert a.min() >= 0 and a.max() < n
        assert (a[:, 0] != a[:, 1]).all() and (a[:, 0] != a[:, 2]).all() and (a[:, 1] != a[:, 2]).all()
        assert np.array_equal(a, plane_ref.draw_triples(n, 200, np.random.default_rng(7)))
    assert not np.array_equal(a, inference.sample_triples(1000, 200, np.random.default_rng(8)))
    with pytest.raises(ValueError):
        inference.sample_triples(2, 5, np.random.default_rng(0))


@pytest.mark.parametrize("count,sumsq,want", [
    ([5, 9, 7], [1.0, 9.0, 0.1], 1),                 # the count decides, whatever the sums
    ([9, 9, 7], [2.0, 1.0, 0.1], 1),                 # equal counts: the smaller sum of squares
    ([9, 4, 9, 9], [1.5, 0.0, 1.5, 1.5], 0),         # an exact duplicate hypothesis: the earliest
    ([4, 9, 9, 9], [0.0, 1.5, 1.0, 1.0], 2),
    ([3], [0.25], 0),
])
def test_selection_rule_count_then_sumsq_then_earliest(count, sumsq, want):
    import inference
    assert inference.choose_plane(np.array(count, np.int64), np.array(sumsq)) == want
    assert plane_ref.choose(np.array(count, np.int64), np.array(sumsq)) == want


def test_selection_of_nothing():
    import inference
    assert inference.choose_plane(np.zeros(0, np.int64), np.zeros(0)) == -1


def test_init_n_other_than_three_and_cpu_device_are_refused():
    import inference
    xyz = plane_ref.make_room(0, walls=(40, 30, 20, 10), clutter=5)
    wall = np.ones(len(xyz), bool)
    with pytest.raises(ValueError):
        inference.get_room_walls(xyz, wall, init_n=4)
    with pytest.raises(wsis_native.WsisError):
        inference.get_room_walls(xyz, wall, device="cpu")


def test_device_wrappers_refuse_cpu_tensors():
    import inference
    import torch
    with pytest.raises(wsis_native.WsisError):
        inference.plane_score(torch.zeros(8, 3), torch.zeros(2, 4, dtype=torch.float64), 0.1)
    with pytest.raises(wsis_native.WsisError):
        inference.plane_mark(torch.zeros(8, 3), torch.zeros(4, dtype=torch.float64), 0.1)


def test_workspace_query_is_monotone_and_refuses_bad_h():
    q = wsis_native.hip().wsis_plane_score_workspace_bytes
    ns = [0, 1, 2047, 2048, 2049, 10007, 10 ** 5, 10 ** 6, 10 ** 7]
    hs = [1, 3, 64, 200, 1024]
    table = np.array([[q(n, h) for h in hs] for n in ns])
    assert (table > 0).all()
    assert (np.diff(table, axis=0) >= 0).all() and (np.diff(table, axis=1) >= 0).all()
    assert table[-1, -1] > table[0, 0] and q(10 ** 6, 200) > q(10 ** 5, 200) > q(10 ** 5, 3)
    for h in (0, -1, 1025):
        assert q(1000, h) < 0
    assert q(-1, 8) < 0


def test_new_symbols_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "wsis_hip.h")).read()
    lib = ctypes.CDLL(os.path.join(ROOT, "3d-wsis_amd", "libwsis_hip.so"))
    _, hip_names = wsis_native.declared_symbols()
    for name in NEW_SYMBOLS:
        assert name + "(" in text and hasattr(lib, name) and name in hip_names
    assert "utils/planeSegment.py:29-63" in text and "segment_plane" in text
    assert wsis_native.hip().wsis_plane_score.argtypes is not None
