"""GPU: the pointgroup_ops drop-in against independent references at the edges of its kernels (tests/point_ops_cases.py
builds the inputs and the references; tests/test_point_ops_cases_host.py checks them on any machine).

  ball query        csrc/cluster.hip       exact ties of the strict `<` on a dyadic lattice; cells across 0 (floorf); cell
                                           indices outside the 18-bit key fields; count == 1000 (grid path) against 1001
                                           (overflow scan), a cut inside a ballot, batch offsets that are no multiple of
                                           64, an empty batch item; r == 0, N == 0, N == 1; N = 2048 * 256 + 1 (the
                                           grid-stride loops take a second trip)
  bfs_cluster       csrc/cluster.hip       frontiers of 255 .. 513 points (one and two 256-thread chunks), children
                                           contested by several parents, a 2000-deep chain, interleaved and negative
                                           labels, sizes at threshold and threshold - 1, no kept cluster, 70,000 clusters,
                                           empty lists, N == 0, the host fallback at a 1000-entry list
  voxelization_idx  csrc/voxelize_idx.hip  one voxel, all distinct, voxels that differ in one column, extreme int64 values,
                                           the table at its highest load, probing that wraps past the last slot,
                                           N = 2048 * 256 + 1
  voxelization      csrc/core.hip          rows without points, INT32_MIN padding, a row of 300, points in no row, modes 4
                                           and 3, C in {1, 3, 6, 8}, M * C > 2048 * 256, transposed and bf16 input

Outputs the caller owns are pre-filled with a sentinel where the C ABI is called directly.  Integer results are compared
bit for bit; every case runs twice and the two runs must be identical."""
import numpy as np
import pytest
import torch

import point_ops_cases as P
import pointgroup_ops
import wsis_native as _n
from oracle import pg_ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -7
GUARD = 64


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)              # (a copy: the cases are read-only)


# ---------------------------------------------------------------- ball query
def _ballquery(scene):
    """wsis_ballquery_count / _fill on sentinel-filled outputs; idx has a guard tail that must stay untouched"""
    lib = _n.hip()
    xyz, bi, off = _dev(scene.xyz), _dev(scene.batch_idx), _dev(scene.batch_off)
    N, B = len(scene.xyz), len(scene.batch_off) - 1
    ws_bytes = lib.wsis_ballquery_workspace_bytes(N)
    assert ws_bytes > 0
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    sl = torch.full((N, 2), SENTINEL, dtype=torch.int32, device=DEV)
    total = torch.full((1,), SENTINEL, dtype=torch.int32, device=DEV)
    st = _n.stream_ptr()
    _n.check(lib.wsis_ballquery_count(_n.ptr(xyz), _n.ptr(bi), _n.ptr(off), N, B, float(scene.radius), _n.ptr(sl),
                                      _n.ptr(total), _n.ptr(ws), ws_bytes, st), "ballquery_count")
    n = int(total.item())
    assert n >= 0
    idx = torch.full((n + GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
    _n.check(lib.wsis_ballquery_fill(_n.ptr(xyz), _n.ptr(bi), _n.ptr(off), N, B, float(scene.radius), _n.ptr(sl),
                                     _n.ptr(idx), n, _n.ptr(ws), ws_bytes, st), "ballquery_fill")
    torch.cuda.synchronize()
    idx, sl = idx.cpu().numpy(), sl.cpu().numpy()
    assert (idx[n:] == SENTINEL).all(), "wrote past the end of idx"
    return idx[:n], sl


def _ballquery_twice(scene):
    idx, sl = _ballquery(scene)
    idx2, sl2 = _ballquery(scene)
    assert np.array_equal(idx, idx2) and np.array_equal(sl, sl2), "two runs differ"
    return idx, sl


def _pairs(idx, sl):
    return np.repeat(np.arange(len(sl), dtype=np.int64), sl[:, 1]) * len(sl) + idx


def _invariants(idx, sl, cap_reached):
    n = sl[:, 1].astype(np.int64)
    assert np.array_equal(sl[:, 0], np.concatenate([[0], np.cumsum(n)[:-1]]) if len(n) else n), "start = prefix sum"
    assert idx.size == n.sum() and (idx != SENTINEL).all() and n.max(initial=0) <= P.BQ_CAP
    inner = np.ones(idx.size, dtype=bool)
    inner[sl[n > 0, 0]] = False                          # the first entry of every list
    assert (np.diff(idx.astype(np.int64), prepend=0)[inner] > 0).all(), "lists ascend"
    if not cap_reached:
        assert (n < P.BQ_CAP).all()
        pq = np.sort(_pairs(idx, sl))
        qp = np.sort(idx.astype(np.int64) * len(sl) + np.repeat(np.arange(len(sl), dtype=np.int64), n))
        assert np.array_equal(pq, qp), "p lists q and q does not list p"


@pytest.mark.parametrize("name", sorted(P.SCENES))
def test_ballquery_is_exact(name):
    """a far_z / far_y failure with counts two or three times the reference is the unmasked cell key"""
    scene = P.SCENES[name]()
    want_idx, want_sl = P.oracle_flat(name)
    idx, sl = _ballquery_twice(scene)
    wrong = np.flatnonzero(sl[:, 1] != want_sl[:, 1])
    assert wrong.size == 0, (f"{wrong.size} of {len(sl)} counts differ; first: point {wrong[0]} has {sl[wrong[0], 1]}, "
                             f"reference {want_sl[wrong[0], 1]}; ratio got/want up to "
                             f"{(sl[wrong, 1] / np.maximum(want_sl[wrong, 1], 1)).max():.2f}")
    assert np.array_equal(sl, want_sl) and np.array_equal(idx, want_idx)
    _invariants(idx, sl, cap_reached=(name == "cap"))


def test_ballquery_second_trip_of_the_grid_stride_loops():
    scene, counts, lists = P.large_scene()
    idx, sl = _ballquery_twice(scene)
    assert np.array_equal(sl[:, 1], counts)
    _invariants(idx, sl, cap_reached=False)
    for p, want in lists.items():
        assert np.array_equal(idx[sl[p, 0]:sl[p, 0] + sl[p, 1]], want), p
    last = len(counts) - 1
    assert last in lists and last >= P.GRID_THREADS


@pytest.mark.parametrize("name", ["r0", "none"])
def test_ballquery_degenerate(name):
    scene = P.zero_radius_scene() if name == "r0" else P.no_point_scene()
    idx, sl = _ballquery_twice(scene)                     # count and fill both return OK
    assert idx.size == 0 and (sl == 0).all() and sl.shape == (len(scene.xyz), 2)
    got_idx, got_sl = pointgroup_ops.ballquery_batch_p(_dev(scene.xyz), _dev(scene.batch_idx), _dev(scene.batch_off),
                                                       scene.radius, 50)
    assert got_idx.numel() == 0 and not bool(got_sl.any())


# ---------------------------------------------------------------- bfs_cluster on the device
def _bfs_device(case, thr):
    ci, co = pointgroup_ops.bfs_cluster(_dev(case.sem), _dev(case.idx), _dev(case.start_len), thr)
    assert ci.is_cuda and co.is_cuda and ci.dtype == torch.int32 and co.dtype == torch.int32
    return ci.cpu().numpy().reshape(-1, 2), co.cpu().numpy()


@pytest.mark.parametrize("name", sorted(P.BFS_CASES))
def test_bfs_cluster_device_is_the_fifo_walk(name):
    case = P.bfs_case(name)
    for thr in case.thresholds:
        ri, ro = pg_ops.bfs_cluster(case.sem, case.idx, case.start_len, thr)
        hi, ho = pointgroup_ops.bfs_cluster(torch.from_numpy(np.array(case.sem)), torch.from_numpy(np.array(case.idx)),
                                            torch.from_numpy(np.array(case.start_len)), thr)
        di, do = _bfs_device(case, thr)
        assert np.array_equal(do, ro) and np.array_equal(di, ri.reshape(-1, 2)), (name, thr)
        assert np.array_equal(do, ho.numpy()) and np.array_equal(di, hi.numpy().reshape(-1, 2)), (name, thr)
        di2, do2 = _bfs_device(case, thr)
        assert np.array_equal(di, di2) and np.array_equal(do, do2), "two runs differ"


@pytest.mark.parametrize("name", sorted(P.BFS_CASES))
def test_cc_same_label_roots_and_sizes(name):
    case = P.bfs_case(name)
    N = len(case.sem)
    want_root, want_size = P.components(case)
    sem, idx, sl = _dev(case.sem), _dev(case.idx), _dev(case.start_len)
    runs = []
    for _ in range(2):
        parent, root, size = (torch.full((N,), SENTINEL, dtype=torch.int32, device=DEV) for _ in range(3))
        _n.check(_n.hip().wsis_cc_same_label(_n.ptr(sem), _n.ptr(idx), _n.ptr(sl), N, _n.ptr(parent), _n.ptr(root),
                                             _n.ptr(size), _n.stream_ptr()), "cc_same_label")
        torch.cuda.synchronize()
        runs.append((root.cpu().numpy(), size.cpu().numpy()))
    root, size = runs[0]
    assert np.array_equal(root, want_root), "root[i] = smallest index of i's component"
    assert np.array_equal(size[root], want_size), "size[root] = size of the component"
    assert np.array_equal(root, runs[1][0]) and np.array_equal(size, runs[1][1])


# ---------------------------------------------------------------- voxelization_idx on the device
def _vi_device(coords):
    out = pointgroup_ops.voxelization_idx(_dev(coords), 2, 4)
    assert all(t.is_cuda for t in out)
    return tuple(t.cpu().numpy() for t in out)


def _vi_check(coords):
    want = P.first_occurrence(coords)
    got = _vi_device(coords)
    host = tuple(t.numpy() for t in pointgroup_ops.voxelization_idx(torch.from_numpy(np.array(coords)), 2, 4))
    for g, w, h, what in zip(got, want, host, ("voxel_locs", "p2v", "v2p")):
        assert g.shape == w.shape and g.dtype == w.dtype and np.array_equal(g, w), what
        assert np.array_equal(g, h), what + " (host library)"
    if len(coords) <= P.VI_DICT_ORACLE_MAX:
        for g, w in zip(got, pg_ops.voxelization_idx(coords)):
            assert np.array_equal(g, w)
    for g, g2 in zip(got, _vi_device(coords)):
        assert np.array_equal(g, g2), "two runs differ"


@pytest.mark.parametrize("name", sorted(P.VI_CASES))
def test_voxelization_idx_device(name):
    _vi_check(P.vi_case(name))


def test_voxelization_idx_device_small_random_inputs_at_full_load():
    for seed in range(64):
        coords = P.vi_random_small(seed)
        got = _vi_device(coords)
        for g, w in zip(got, pg_ops.voxelization_idx(coords)):
            assert g.shape == w.shape and np.array_equal(g, w), seed


# ---------------------------------------------------------------- voxelization
def _vox_check(case, C, mode, seed):
    v2p = _dev(case.v2p)
    feats = P.vox_feats(case.n_points, C, seed)
    g = P.vox_feats(case.v2p.shape[0], C, seed + 1)
    runs = []
    for _ in range(2):
        f = _dev(feats).requires_grad_(True)
        out = pointgroup_ops.voxelization(f, v2p, mode)
        out.backward(_dev(g))
        runs.append((out.detach().cpu().numpy(), f.grad.cpu().numpy()))
    out, grad = runs[0]
    assert np.array_equal(out, runs[1][0]) and np.array_equal(grad, runs[1][1]), "two runs differ"
    n = case.v2p[:, 0]
    # the operator's contract: the sequential fp32 sum in list order, bit for bit
    assert np.array_equal(out, pg_ops.voxelization(feats, case.v2p, mode))
    assert np.array_equal(grad, pg_ops.voxelization_backward(g, case.v2p, case.n_points, mode))
    # and an fp64 mean / sum within the bound of n additions, a multiplication per term and a reciprocal
    ref, bound = P.vox_fp64(feats, case.v2p, mode)
    err = np.abs(out.astype(np.float64) - ref)
    print(f"C={C} mode={mode}: max err / bound = {(err / np.maximum(bound, 1e-300)).max():.3f}")
    assert (err <= bound).all()
    assert (out[n == 0] == 0).all() and not np.signbit(out[n == 0]).any(), "a row without points is exactly 0"
    dref, dbound = P.vox_bwd_fp64(g, case.v2p, case.n_points, mode)
    assert (np.abs(grad.astype(np.float64) - dref) <= dbound).all()
    unlisted = np.ones(case.n_points, dtype=bool)
    for m in np.flatnonzero(n > 0):
        unlisted[case.v2p[m, 1:1 + n[m]]] = False
    assert unlisted.sum() >= 61 and (grad[unlisted] == 0).all(), "a point in no voxel gets exactly 0"


@pytest.mark.parametrize("mode", [4, 3])
@pytest.mark.parametrize("C", P.VOX_CHANNELS)
def test_voxelization_handwritten_maps(C, mode):
    _vox_check(P.vox_small(), C, mode, 70 + C)


@pytest.mark.parametrize("mode", [4, 3])
def test_voxelization_second_trip_of_the_grid_stride_loop(mode):
    case = P.vox_large()
    assert case.v2p.shape[0] * P.VOX_LARGE_C > P.GRID_THREADS
    _vox_check(case, P.VOX_LARGE_C, mode, 80)


@pytest.mark.parametrize("mode", [4, 3])
def test_voxelization_takes_views_and_bf16(mode):
    case = P.vox_small()
    v2p = _dev(case.v2p)
    C = 6
    base = _dev(P.vox_feats(C, case.n_points, 90))                        # [C, N]: its transpose is a strided view
    view = base.t()
    assert not view.is_contiguous()
    assert torch.equal(pointgroup_ops.voxelization(view, v2p, mode),
                       pointgroup_ops.voxelization(view.contiguous().float(), v2p, mode))
    low = view.contiguous().bfloat16()
    got = pointgroup_ops.voxelization(low, v2p, mode)
    assert got.dtype == torch.float32
    assert torch.equal(got, pointgroup_ops.voxelization(low.contiguous().float(), v2p, mode))
    want = pg_ops.voxelization(low.float().cpu().numpy(), case.v2p, mode)
    assert np.array_equal(got.cpu().numpy(), want)
