"""Runs on any machine: every input of tests/point_ops_cases.py has the property it is named after, the independent
references agree with each other, the host library reproduces the oracle on the new voxelization_idx and bfs_cluster
cases, and the grid walk of the ball query -- replayed in numpy -- equals the oracle with masked cell keys and does not
without the mask (the reasoning behind cell_key() of csrc/cluster.hip, pinned without a GPU)."""
import numpy as np
import pytest
import torch

import point_ops_cases as P
import pointgroup_ops
from oracle import pg_ops


# ---------------------------------------------------------------- ball query
@pytest.mark.parametrize("name", sorted(P.SCENES))
def test_ballquery_references_agree(name):
    s = P.SCENES[name]()
    idx, sl = P.oracle_flat(name)
    k_idx, k_sl = P.kd_flat(s)
    assert np.array_equal(sl, k_sl) and np.array_equal(idx, k_idx)
    assert np.array_equal(np.minimum(P.true_counts(s), P.BQ_CAP), sl[:, 1])      # integer arithmetic on the lattice


@pytest.mark.parametrize("name", ["origin", "straddle", "offset", "far_z", "far_y"])
def test_lattice_scenes_are_exact_and_full_of_ties(name):
    s = P.lattice_scene(name)
    assert P.tie_pairs(s) >= 1000
    assert np.array_equal(P.units_of(s) * P.UNIT, s.xyz.astype(np.float64))
    hit, tie = P.hits_int(s)
    # the fp32 expression of the kernel gives the integer answer on every pair, ties included
    e = s.xyz[:, None, :] - s.xyz[None, :, :]
    d2 = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
    assert d2.dtype == np.float32
    r2 = np.float32(s.radius) * np.float32(s.radius)
    same = s.batch_idx[:, None] == s.batch_idx[None, :]
    assert np.array_equal(same & (d2 < r2), hit) and np.array_equal(same & (d2 == r2), tie)


def test_lattice_block_has_the_tie_count_stated():
    assert P.tie_pairs(P.lattice_scene("origin")) > 1000
    s = P.lattice_scene("origin")
    one = P.Scene("one", s.xyz, np.zeros_like(s.batch_idx), np.array([0, len(s.xyz)], np.int32), s.radius)
    assert P.tie_pairs(one) > P.tie_pairs(s)          # pairs across the two batch items do not count


def test_cap_scene_has_every_kind_of_point():
    s = P.cap_scene()
    cnt = P.true_counts(s)
    _, sl = P.oracle_flat("cap")
    assert (sl[:, 1] == np.minimum(cnt, P.BQ_CAP)).all() and (cnt > P.BQ_CAP).sum() > 100
    assert s.batch_off[1] % 64 and (s.batch_off[2] - s.batch_off[1]) % 64


def test_large_scene_reaches_the_second_trip():
    s, counts, lists = P.large_scene()
    assert len(s.xyz) == 2048 * 256 + 1 and len(lists) == (len(s.xyz) + 63) // 64
    p = max(lists)
    assert counts[p] == len(lists[p]) and (np.diff(lists[p]) > 0).all()


@pytest.mark.parametrize("name", P.FAR)
def test_grid_walk_needs_the_key_mask(name):
    s = P.lattice_scene(name)
    want = P.oracle_flat(name)[1][:, 1]
    c = P.cells_fp32(s)[0]
    # z past the top of its field sets the lowest y bit (18 keys left); y below 0 sign-extends over the whole x field (9)
    assert len(set(P.neighbour_keys(0, c, True))) == 27
    assert len(set(P.neighbour_keys(0, c, False))) == {"far_z": 18, "far_y": 9}[name]
    assert np.array_equal(P.grid_walk_counts(s, masked=True), want)
    bad = P.grid_walk_counts(s, masked=False)
    assert (bad != want).sum() > len(want) // 2 and (bad >= want).all() and (bad <= 3 * want).all()


def test_grid_walk_without_mask_is_right_near_the_origin():
    s = P.lattice_scene("straddle")
    want = P.oracle_flat("straddle")[1][:, 1]
    assert np.array_equal(P.grid_walk_counts(s, masked=False), want)
    assert np.array_equal(P.grid_walk_counts(s, masked=True), want)


# ---------------------------------------------------------------- bfs_cluster
@pytest.mark.parametrize("name", sorted(P.BFS_CASES))
def test_host_bfs_cluster_reproduces_the_oracle(name):
    case = P.bfs_case(name)
    root, size = P.components(case)
    for thr in case.thresholds:
        ri, ro = pg_ops.bfs_cluster(case.sem, case.idx, case.start_len, thr)
        hi, ho = pointgroup_ops.bfs_cluster(torch.from_numpy(case.sem), torch.from_numpy(case.idx),
                                            torch.from_numpy(case.start_len), thr)
        assert np.array_equal(ho.numpy(), ro) and np.array_equal(hi.numpy().reshape(-1, 2), ri.reshape(-1, 2))
        # the kept clusters are scipy's components of at least thr points, seeded at their smallest index, in seed order
        seeds = np.flatnonzero((root == np.arange(len(root))) & (size >= thr))
        assert np.array_equal(ri[ro[:-1], 1] if len(seeds) else np.zeros(0, np.int32), seeds)
        assert np.array_equal(np.diff(ro), size[seeds])


def test_bfs_cases_cover_what_they_are_named_after():
    assert len(pg_ops.bfs_cluster(*P.bfs_case("stars")[:3], 1028)[1]) == 1                 # nothing kept
    assert len(pg_ops.bfs_cluster(*P.bfs_case("singletons")[:3], 1)[1]) == 70001
    assert P.bfs_case("fallback").start_len[:, 1].max() >= 1000
    assert P.bfs_case("no_lists").idx.size == 0 and len(P.bfs_case("none").sem) == 0
    assert max(len(f) for f in P.frontier_sizes(P.bfs_case("chain"))) == 2001


# ---------------------------------------------------------------- voxelization_idx
def _host_vi(coords):
    locs, p2v, v2p = pointgroup_ops.voxelization_idx(torch.from_numpy(np.array(coords)), 2, 4)
    return locs.numpy(), p2v.numpy(), v2p.numpy()


def _same3(got, want):
    return all(np.array_equal(g, w) and g.shape == w.shape for g, w in zip(got, want))


@pytest.mark.parametrize("name", sorted(P.VI_CASES))
def test_host_voxelization_idx_reproduces_the_oracles(name):
    coords = P.vi_case(name)
    want = P.first_occurrence(coords)
    assert _same3(_host_vi(coords), want)
    if len(coords) <= P.VI_DICT_ORACLE_MAX:
        assert _same3(pg_ops.voxelization_idx(coords), want)


def test_host_voxelization_idx_on_small_random_inputs():
    for seed in range(64):
        coords = P.vi_random_small(seed)
        want = pg_ops.voxelization_idx(coords)
        assert _same3(_host_vi(coords), want) and _same3(P.first_occurrence(coords), want)


def test_wrap_case_starts_three_voxels_in_the_last_slot():
    coords = P.vi_case("wrap")
    cap = P.table_cap(len(coords))
    home = [P.hash4(r) & (cap - 1) for r in coords.tolist()]
    assert len({tuple(r) for r, h in zip(coords.tolist(), home) if h == cap - 1}) == 3
    assert P.mix64(0) == 0 and P.mix64(1) == 0xb456bcfc34c2cb2c       # MurmurHash3's fmix64


# ---------------------------------------------------------------- voxelization
def test_voxelization_maps_and_the_derived_bound():
    small, large = P.vox_small(), P.vox_large()
    assert large.v2p.shape[0] * P.VOX_LARGE_C == 524292
    for case, C, mode in ((small, 3, 4), (small, 8, 3), (large, P.VOX_LARGE_C, 4)):
        feats = P.vox_feats(case.n_points, C, 7)
        seq = pg_ops.voxelization(feats, case.v2p, mode)
        ref, bound = P.vox_fp64(feats, case.v2p, mode)
        assert (np.abs(seq - ref) <= bound).all() and (seq[case.v2p[:, 0] == 0] == 0).all()
        g = P.vox_feats(case.v2p.shape[0], C, 8)
        dseq = pg_ops.voxelization_backward(g, case.v2p, case.n_points, mode)
        dref, dbound = P.vox_bwd_fp64(g, case.v2p, case.n_points, mode)
        assert (np.abs(dseq - dref) <= dbound).all()
        assert (dref == 0).all(1).sum() >= 61
