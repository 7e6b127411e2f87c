"""GPU: the S3DIS wall split -- wsis_plane_score / wsis_plane_mark (csrc/plane.hip), inference.get_room_walls and the
``wall_class`` keyword of inference.clustering_in_graph -- against the fp64 numpy oracle of tests/plane_ref.py.

The device evaluates |((a*x + b*y) + c*z) + d| in fp64 without contraction, which is bit for bit the oracle's
expression, so inlier counts and masks are compared EXACTLY; every comparison first asserts that no distance of the case
lies within plane_ref.GAP of the threshold (the strict `<` then cannot depend on a last bit).  Sums of squares are sums
of N non-negative fp64 terms in another order: they agree within N * 2^-52 relative, and bit for bit between two calls.

Shapes: a workgroup takes 2048 points (four waves of 64 lanes x 8 points) and stages 128 planes at a time, so N runs
over the wave and workgroup edges (63..65, 511..513, 2047/2049, several workgroups with a ragged tail) and H over one
plane, a partial chunk, two chunks with a ragged second one (200) and the maximum (1024)."""
import functools
import os

import numpy as np
import pytest
import torch

import plane_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
THR = 0.1


@functools.lru_cache(maxsize=None)
def _room():
    xyz = plane_ref.make_room(0)
    return xyz


@functools.lru_cache(maxsize=None)
def _score_case(N, H):
    """points = the first N of the room, planes from H random triples of the whole room; oracle results"""
    room = _room()
    rng = np.random.default_rng(1000 * H + N)
    planes, valid = plane_ref.planes_from_triples(room[plane_ref.draw_triples(len(room), H, rng).reshape(-1)].reshape(H, 3, 3))
    assert valid.all()
    xyz = np.ascontiguousarray(room[:N])
    count, sumsq, gap = plane_ref.score(xyz, planes, THR)
    assert gap > plane_ref.GAP
    return xyz, planes, count, sumsq


def _poisoned(N, H):
    import wsis_native as _n
    count = torch.full((H,), -1, dtype=torch.int64, device=DEV)
    sumsq = torch.full((H,), float("nan"), dtype=torch.float64, device=DEV)
    ws = torch.full((int(_n.hip().wsis_plane_score_workspace_bytes(N, H)),), 0xFF, dtype=torch.uint8, device=DEV)
    return count, sumsq, ws


def _device_score(xyz, planes, thr=THR):
    import inference
    N, H = len(xyz), len(planes)
    count, sumsq, ws = _poisoned(N, H)
    inference.plane_score(torch.from_numpy(xyz).to(DEV), torch.from_numpy(planes).to(DEV), thr, out=(count, sumsq),
                          workspace=ws)
    return count.cpu(), sumsq.cpu()


SCORE_CASES = [(1, 1), (1, 200), (63, 3), (64, 200), (65, 1024), (511, 3), (512, 1), (513, 200), (2047, 3), (2049, 200),
               (2049, 1024), (10007, 1), (10007, 200)]


@pytest.mark.parametrize("N,H", SCORE_CASES)
def test_plane_score_counts_are_exact_and_sums_reproducible(N, H):
    xyz, planes, want_count, want_sumsq = _score_case(N, H)
    count, sumsq = _device_score(xyz, planes)
    assert count.dtype == torch.int64 and torch.equal(count, torch.from_numpy(want_count))
    got = sumsq.numpy()
    assert np.isfinite(got).all()
    err = np.abs(got - want_sumsq)
    print(f"N={N} H={H}: max inliers {int(want_count.max())}, max rel err of sumsq "
          f"{float((err / np.maximum(want_sumsq, 1e-300)).max()):.3e}")
    assert (err <= N * 2.0 ** -52 * want_sumsq).all()
    count2, sumsq2 = _device_score(xyz, planes)
    assert torch.equal(count2, count)
    assert torch.equal(sumsq2.view(torch.int64), sumsq.view(torch.int64)), "sumsq is bit-reproducible run to run"


def test_plane_score_of_no_points_is_zero():
    import inference
    count, sumsq, ws = _poisoned(0, 3)
    inference.plane_score(torch.zeros(0, 3, device=DEV), torch.zeros(3, 4, dtype=torch.float64, device=DEV), THR,
                          out=(count, sumsq), workspace=ws)
    assert count.tolist() == [0, 0, 0] and sumsq.tolist() == [0.0, 0.0, 0.0]
    assert bool((ws == 0xFF).all()), "nothing was launched"


def test_plane_mark_equals_oracle_and_its_popcount_is_the_score():
    import inference
    xyz, planes, want_count, _ = _score_case(10007, 200)
    count, _ = _device_score(xyz, planes)
    xyz_d, planes_d = torch.from_numpy(xyz).to(DEV), torch.from_numpy(planes).to(DEV)
    for h in sorted({0, 1, 127, 128, 199, int(want_count.argmax()), int(want_count.argmin())}):
        out = torch.full((len(xyz),), 7, dtype=torch.uint8, device=DEV)
        mask = inference.plane_mark(xyz_d, planes_d[h], THR, out=out).cpu().numpy()
        assert set(np.unique(mask)) <= {0, 1}
        assert np.array_equal(mask.astype(bool), plane_ref.mark(xyz, planes[h], THR))
        assert int(mask.sum()) == int(count[h]) == int(want_count[h])


def test_nan_and_inf_coordinates_are_never_inliers_and_change_nothing_else():
    """a NaN in workgroup 0 and a +inf in workgroup 1, both at points that are inliers of some plane when finite.
    Against the same cloud with the two points moved far away (never inliers, 0.0 at the same place of every sum):
    counts equal, sums BIT-equal; against the oracle on the poisoned cloud: exact counts and masks."""
    import inference
    xyz, planes, clean_count, _ = _score_case(2049, 200)
    i_nan, i_inf = 5, 2048
    inl = np.stack([plane_ref.mark(xyz[[i_nan, i_inf]], p, THR) for p in planes])
    assert inl[:, 0].any() and inl[:, 1].any()
    bad, far = xyz.copy(), xyz.copy()
    bad[i_nan, 1], bad[i_inf, 0] = np.nan, np.inf
    far[i_nan], far[i_inf] = 1e6, -1e6
    want_count, want_sumsq, gap = plane_ref.score(bad, planes, THR)
    assert gap > plane_ref.GAP and (want_count < clean_count).any()
    assert np.array_equal(want_count, plane_ref.score(far, planes, THR)[0])
    count, sumsq = _device_score(bad, planes)
    count_far, sumsq_far = _device_score(far, planes)
    assert torch.equal(count, torch.from_numpy(want_count)) and torch.equal(count, count_far)
    assert np.isfinite(sumsq.numpy()).all()
    assert torch.equal(sumsq.view(torch.int64), sumsq_far.view(torch.int64))
    assert (np.abs(sumsq.numpy() - want_sumsq) <= len(xyz) * 2.0 ** -52 * want_sumsq).all()
    h = int(np.nonzero(inl[:, 0] & inl[:, 1])[0][0]) if (inl[:, 0] & inl[:, 1]).any() else int(np.nonzero(inl[:, 0])[0][0])
    mask = inference.plane_mark(torch.from_numpy(bad).to(DEV), torch.from_numpy(planes[h]).to(DEV), THR).cpu().numpy()
    assert mask[i_nan] == 0 and mask[i_inf] == 0
    assert np.array_equal(mask.astype(bool), plane_ref.mark(bad, planes[h], THR)) and int(mask.sum()) == int(count[h])


# ---- get_room_walls ---------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _cloud():
    """the 28,000-point room as a NON-prefix subset of a 33,000-point cloud: 5,000 non-wall points inside the room
    (they would be inliers if wall_ind were ignored) interleaved at random positions"""
    room = _room()
    rng = np.random.default_rng(55)
    N = len(room) + 5000
    wall = np.zeros(N, dtype=bool)
    wall[rng.permutation(N)[:len(room)]] = True
    full = np.empty((N, 3), dtype=np.float32)
    full[wall] = room
    full[~wall] = (rng.random((5000, 3)) * np.array([5.0, 4.0, 2.6])).astype(np.float32)
    assert not wall[:len(room)].all()
    return full, wall


@functools.lru_cache(maxsize=None)
def _ref_walls(seed, max_num, min_points):
    full, wall = _cloud()
    walls, info = plane_ref.get_room_walls_ref(full, wall, distance=THR, iter=200, max_num=max_num, seed=seed,
                                               min_points=min_points)
    assert info["gap"] > plane_ref.GAP
    return walls, info


def _check_walls(got, want, full, wall):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == bool and g.shape == (len(full),)
        assert not g[~wall].any()
        assert np.array_equal(g, w)
    if got:
        assert np.stack(got).sum(0).max() == 1, "walls are disjoint"


def test_get_room_walls_matches_the_oracle_on_given_samples():
    import inference
    full, wall = _cloud()
    want, info = _ref_walls(100, 10, 10000)
    assert len(want) == 2 and info["top_ties"] == 0 and info["remaining"] < 10000
    got = inference.get_room_walls(full, wall, distance=THR, iter=200, max_num=10, samples=info["samples"])
    _check_walls(got, want, full, wall)
    first = inference.get_room_walls(full, wall, max_num=1, samples=info["samples"])
    _check_walls(first, want[:1], full, wall)


def test_get_room_walls_finds_all_four_walls_with_a_lower_min_points():
    import inference
    full, wall = _cloud()
    want, info = _ref_walls(100, 10, 2000)
    sizes = [int(w.sum()) for w in want]
    assert len(want) == 4 and sizes == sorted(sizes, reverse=True)
    got = inference.get_room_walls(full, wall, max_num=10, samples=info["samples"], min_points=2000)
    _check_walls(got, want, full, wall)


def test_get_room_walls_seeded_sampler_is_reproducible_and_matches_the_oracle():
    import inference
    full, wall = _cloud()
    want, _ = _ref_walls(7, 10, 10000)
    a = inference.get_room_walls(full, wall, max_num=10, seed=7)
    b = inference.get_room_walls(torch.from_numpy(full).to(DEV), torch.from_numpy(wall).to(DEV), max_num=10, seed=7)
    assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))
    _check_walls(a, want, full, wall)


def test_degenerate_hypotheses():
    """a round whose triples span no plane returns no wall and ends the loop; invalid triples among valid ones are
    ignored (the result is the oracle's with and without those rows)"""
    import inference
    room = _room()[:3000]
    line = np.array([[0.5, 0.25, 0.125], [1.0, 0.5, 0.25], [2.0, 1.0, 0.5], [4.0, 2.0, 1.0]], dtype=np.float32)
    xyz = np.concatenate([line, room])
    wall = np.ones(len(xyz), dtype=bool)
    collinear = np.array([[0, 1, 2], [1, 2, 3], [3, 0, 2], [2, 2, 2], [5, 5, 9], [7, 8, 7]])
    assert not plane_ref.planes_from_triples(xyz[collinear.reshape(-1)].reshape(-1, 3, 3))[1].any()
    assert inference.get_room_walls(xyz, wall, samples=[collinear, collinear], min_points=100) == []
    # round 1 degenerate (repeated indices: whatever points remain) after a good round 0: exactly one wall
    repeated = collinear[3:]
    rng = np.random.default_rng(9)
    good = plane_ref.draw_triples(len(xyz), 50, rng)
    mixed = good.copy()
    mixed[[0, 5, 17]] = collinear[[0, 3, 4]]
    keep = np.ones(50, dtype=bool)
    keep[[0, 5, 17]] = False
    want, info = plane_ref.get_room_walls_ref(xyz, wall, max_num=2, samples=[mixed, repeated], min_points=100)
    want_dropped, _ = plane_ref.get_room_walls_ref(xyz, wall, max_num=2, samples=[mixed[keep], repeated], min_points=100)
    assert info["gap"] > plane_ref.GAP and len(want) == 1 and np.array_equal(want[0], want_dropped[0])
    got = inference.get_room_walls(xyz, wall, max_num=2, samples=[mixed, repeated], min_points=100)
    _check_walls(got, want, xyz, wall)
    with pytest.raises(ValueError):
        inference.get_room_walls(xyz, wall, samples=[np.array([[0, 1, len(xyz)]])], min_points=100)


# ---- clustering_in_graph(wall_class=...) ----------------------------------------------------------------------------

class _Graph(object):          # the one igraph method the reference calls
    def __init__(self, lists):
        self.lists = lists

    def neighbors(self, vertex, mode="all"):
        return [int(v) for v in self.lists[int(vertex)]]


def test_clustering_in_graph_appends_the_walls_and_is_unchanged_without_wall_class():
    import inference
    from oracle import cluster_ref
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cluster_golden.npz"))
    S = len(g["s_sem"])
    graph = _Graph(cluster_ref.neighbour_lists(g["s_edges"], S))
    args = ("golden", g["s_xyz"], g["s_superpoint"], graph, g["s_sem"], g["s_off"], g["s_occ"], g["s_size"])
    kw = dict(semantic_ind2label=inference.S3DIS_LABEL_IDX, valid_labels=inference.S3DIS_VALID_LABELS,
              radius_factor=0.8, stuff_classes=(0, 1))
    conf0, label0, masks0 = inference.clustering_in_graph(*args, **kw)
    conf1, label1, masks1 = inference.clustering_in_graph(*args, wall_class=None, wall_kwargs=None, **kw)
    assert np.array_equal(conf0, conf1) and np.array_equal(label0, label1) and np.array_equal(masks0, masks1)
    assert np.array_equal(label0, g["s_label_id"]) and 3 not in label0
    assert np.array_equal(masks0, np.unpackbits(g["s_masks"], axis=1)[:, :masks0.shape[1]].astype(np.int64))

    # the fixture has 2444 predicted wall points: min_points = 500 lets the oracle find walls
    wall = g["s_sem"][g["s_superpoint"]] == 2
    want, info = plane_ref.get_room_walls_ref(g["s_xyz"], wall, distance=0.1, iter=200, max_num=10, seed=3, min_points=500)
    assert info["gap"] > plane_ref.GAP and len(want) >= 1
    conf, label, masks = inference.clustering_in_graph(
        *args, wall_class=2, wall_kwargs={"min_points": 500, "samples": info["samples"]}, **kw)
    n0 = len(conf0)
    assert len(conf) == len(label) == len(masks) == n0 + len(want)
    assert np.array_equal(conf[:n0], conf0) and np.array_equal(label[:n0], label0) and np.array_equal(masks[:n0], masks0)
    assert (conf[n0:] == 1).all() and (label[n0:] == 3).all() and masks.dtype == masks0.dtype
    assert np.array_equal(masks[n0:].astype(bool), np.stack(want))


# ---- refusals -------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_outputs_untouched():
    import inference
    import wsis_native as _n
    xyz, planes, _, _ = _score_case(513, 200)
    xyz_d, planes_d = torch.from_numpy(xyz).to(DEV), torch.from_numpy(planes).to(DEV)

    def untouched(count, sumsq):
        torch.cuda.synchronize()
        return bool((count == -1).all()) and bool(torch.isnan(sumsq).all())

    count, sumsq, ws = _poisoned(513, 200)
    with pytest.raises(_n.WsisError, match="workspace too small"):
        inference.plane_score(xyz_d, planes_d, THR, out=(count, sumsq), workspace=ws[:ws.numel() - 256])
    assert untouched(count, sumsq)
    status = _n.hip().wsis_plane_score(_n.ptr(xyz_d), 513, _n.ptr(planes_d), 200, THR, _n.ptr(count), _n.ptr(sumsq), None,
                                       ws.numel(), _n.stream_ptr())
    assert status != 0 and _n.hip().wsis_last_error() and untouched(count, sumsq)

    big = torch.zeros(1025, 4, dtype=torch.float64, device=DEV)
    big[:, 2] = 1.0
    count, sumsq, _ = _poisoned(513, 1024)
    count, sumsq = torch.cat([count, count[:1]]), torch.cat([sumsq, sumsq[:1]])
    ws = torch.zeros(int(_n.hip().wsis_plane_score_workspace_bytes(513, 1024)) * 2, dtype=torch.uint8, device=DEV)
    with pytest.raises(_n.WsisError, match="1024"):
        inference.plane_score(xyz_d, big, THR, out=(count, sumsq), workspace=ws)
    assert untouched(count, sumsq)
    with pytest.raises(_n.WsisError):
        inference.plane_score(xyz_d, big, THR)                  # the workspace query refuses H = 1025 as well
    assert _n.hip().wsis_plane_score(_n.ptr(xyz_d), -1, _n.ptr(planes_d), 200, THR, _n.ptr(count), _n.ptr(sumsq),
                                     _n.ptr(ws), ws.numel(), _n.stream_ptr()) != 0
    assert _n.hip().wsis_plane_score(None, 513, _n.ptr(planes_d), 200, THR, _n.ptr(count), _n.ptr(sumsq),
                                     _n.ptr(ws), ws.numel(), _n.stream_ptr()) != 0
    assert untouched(count, sumsq)

    count, sumsq, ws = _poisoned(513, 200)
    with pytest.raises(_n.WsisError):
        inference.plane_score(torch.from_numpy(xyz), planes_d, THR, out=(count, sumsq), workspace=ws)
    with pytest.raises(_n.WsisError):
        inference.plane_score(xyz_d, torch.from_numpy(planes), THR, out=(count, sumsq), workspace=ws)
    assert untouched(count, sumsq)
    mask = torch.full((513,), 7, dtype=torch.uint8, device=DEV)
    with pytest.raises(_n.WsisError):
        inference.plane_mark(torch.from_numpy(xyz), planes_d[0], THR, out=mask)
    assert _n.hip().wsis_plane_mark(_n.ptr(xyz_d), 513, None, THR, _n.ptr(mask), _n.stream_ptr()) != 0
    torch.cuda.synchronize()
    assert bool((mask == 7).all())
