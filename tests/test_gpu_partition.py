"""GPU: the partition front end (3d-wsis_amd/wsis_partition.py, csrc/partition.hip) against tests/partition_ref.py and
tests/golden/partition_golden.npz (what the reference's own ``compute_graph_nn_2`` and edge-weight expression computed).

1. prune: ids, positions, colours, histogram and counts bit-equal to the oracle at the edges of ply_c.cpp:293-392;
2. k nearest neighbours: ids and the bits of d2 equal to the oracle at every size and k where the kernel takes another
   path (one batch, two batches, one cell, the scan of every point, anisotropic ring growth, ties), and equal to the
   fixture's ``target2`` / ``target`` / ``distances``;
3. geometric features: covariance within one fp64 step per accumulated term ((k + 1) 2^-52 trace), eigenvalues within
   EV_TOL * trace,
   features within what partition_ref.feature_tolerances propagates plus one fp32 step, verticality where the smaller
   relative eigen-gap exceeds GAP_MIN (at most 1 % of the points left out);
4. assembly: the mean within one fp32 step of ``math.fsum``, everything else bit-equal to numpy's fp32 expressions
   evaluated with the device's mean, and the fixture's edge weights within what the two means' difference propagates
   through the fp32 expression (partition_ref.edge_weight_margin) plus one fp32 step;
5. the whole path, a second call, every refusal, and peak device memory.

Every figure is printed before it is asserted."""
import math

import numpy as np
import pytest
import torch

import partition_ref as ref
from test_partition_ref_host import Golden, K_ADJ, K_GEOF, TAGS

pytestmark = pytest.mark.gpu

_CACHE = {}


def wp():
    import wsis_partition
    return wsis_partition


def host(t):
    return None if t is None else t.cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype.itemsize == b.dtype.itemsize and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def report(name, err, tol):
    err, tol = np.asarray(err, np.float64), np.broadcast_to(np.asarray(tol, np.float64), np.shape(err))
    worst = float((err / np.maximum(tol, 1e-300)).max()) if err.size else 0.0
    print(f"{name}: largest error {float(err.max()) if err.size else 0.0:.3g}, largest error / tolerance {worst:.3g}")
    assert (err <= tol).all(), name


# ---- 1: prune ----------------------------------------------------------------------------------------------------------

def _sequential_and_pairwise_differ(x):
    seq = np.float32(0)
    for v in x:
        seq = seq + v
    return seq != np.sum(np.ascontiguousarray(x))


def prune_case(name):
    rng = np.random.default_rng(11)
    voxel = 0.03
    if name == "one_point":
        xyz = np.array([[1.5, -2.25, 0.125]], np.float32)
    elif name == "one_voxel":
        xyz = (np.array([3.0, 4.0, 5.0]) + rng.uniform(0, 0.029, (50, 3))).astype(np.float32)
        xyz[0] = (3.0, 4.0, 5.0)
    elif name == "single_and_300":
        # a voxel of one point, and one of 300 points ten metres out whose sequential and pairwise fp32 sums differ
        big = (np.array([10.0, 10.0, 10.0]) + rng.uniform(0.001, 0.029, (300, 3))).astype(np.float32)
        assert any(_sequential_and_pairwise_differ(big[:, a]) for a in range(3)), "the order of the sum must matter here"
        xyz = np.concatenate([big[:150], [[10.5, 10.01, 10.01]], big[150:], [[10.2, 10.01, 10.01]]]).astype(np.float32)
    elif name == "x_max_on_boundary":
        voxel = 0.25                                        # exact: (1.0 - 0.0) / 0.25 = 4 = n_bin, not clamped
        xyz = np.array([[0, 0, 0], [0.25, 0, 0], [0.5, 0.1, 0], [1.0, 0, 0], [1.0, 0.2, 0.75], [0.99, 0, 0]], np.float32)
    elif name == "negative":
        xyz = rng.uniform(-1.0, -0.2, (4000, 3)).astype(np.float32)
    elif name == "offset_10m":
        xyz = (np.array([10.0, -10.0, 10.0]) + rng.uniform(0, 0.6, (4000, 3))).astype(np.float32)
    elif name == "colours":
        xyz = np.zeros((7, 3), np.float32)
        xyz[2:, 0] = 1.0
    else:
        raise KeyError(name)
    rgb = rng.integers(0, 256, (len(xyz), 3)).astype(np.uint8)
    if name == "colours":                                 # means 1.5 and 254.6: truncation 1 / 254, rounding 2 / 255
        rgb[:2] = [[1, 1, 1], [2, 2, 2]]
        rgb[2:] = [[254, 254, 254], [255, 255, 255], [255, 255, 255], [254, 254, 254], [255, 255, 255]]
    labels = rng.integers(0, 14, len(xyz)).astype(np.uint8)
    return xyz, rgb, labels, voxel


@pytest.mark.parametrize("with_labels", (False, True))
@pytest.mark.parametrize("name", ("one_point", "one_voxel", "single_and_300", "x_max_on_boundary", "negative", "offset_10m",
                                  "colours"))
def test_prune_is_bit_equal_to_the_oracle(name, with_labels):
    xyz, rgb, labels, voxel = prune_case(name)
    want = ref.prune(xyz, voxel, rgb, labels if with_labels else None, 13 if with_labels else 0)
    got = wp().prune(xyz, voxel, rgb, labels if with_labels else None, 13 if with_labels else 0)
    V = len(want["xyz"])
    print(f"{name}: N {len(xyz)} V {V} largest voxel {int(want['count'].max())}")
    assert np.array_equal(host(got.p2v).astype(np.uint32), want["p2v"])
    assert np.array_equal(host(got.count).astype(np.uint32), want["count"])
    assert host(got.xyz).dtype == np.float32 and same_bits(host(got.xyz), want["xyz"])
    assert host(got.rgb).dtype == np.uint8 and np.array_equal(host(got.rgb), want["rgb"])
    if with_labels:
        assert np.array_equal(host(got.label_hist).view(np.uint32), want["label_hist"])
    else:
        assert got.label_hist is None
    if name == "x_max_on_boundary":
        b, _ = ref.bins(xyz, voxel)
        assert b[:, 0].max() == 4 == math.ceil((xyz[:, 0].max() - xyz[:, 0].min()) / voxel)
    if name == "colours":
        assert host(got.rgb).tolist() == [[1, 1, 1], [254, 254, 254]]
    if name == "single_and_300":
        assert sorted(want["count"].tolist()) == [1, 1, 300]


# ---- 2: k nearest neighbours -------------------------------------------------------------------------------------------

def cloud(name):
    if name in _CACHE:
        return _CACHE[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    if name.startswith("blob"):                           # blob<V>: a small cluttered volume
        xyz = rng.uniform(0, 1, (int(name[4:]), 3)).astype(np.float32)
    elif name == "room20000":
        raw, rgb = ref.make_room(5, n=52000)
        xyz = ref.prune(raw, 0.03, rgb)["xyz"][:20000]
        assert len(xyz) == 20000
    elif name == "one_cell":
        xyz = (np.array([2.0, 2.0, 2.0]) + rng.uniform(0, 1e-3, (200, 3))).astype(np.float32)
    elif name == "outlier":                               # one point 100 m away: its query scans every point
        xyz = rng.uniform(0, 1, (1000, 3)).astype(np.float32)
        xyz[417] = (100.0, 0.5, 0.5)
    elif name == "sheet":
        xyz = np.concatenate([rng.uniform(0, 2, (3000, 2)), np.zeros((3000, 1))], 1).astype(np.float32)
    elif name == "line":
        xyz = np.zeros((2000, 3), np.float32)
        xyz[:, 0] = rng.uniform(0, 5, 2000)
    elif name == "duplicates":                            # every point three times, and 70 at one place
        base = rng.uniform(0, 1, (300, 3)).astype(np.float32)
        xyz = np.concatenate([base, base, np.full((70, 3), 0.5, np.float32), base])
        xyz = xyz[rng.permutation(len(xyz))]
    else:
        raise KeyError(name)
    k_max = min(64, len(xyz) - 1)
    out = _CACHE[name] = (np.ascontiguousarray(xyz), ) + ref.knn(xyz, k_max)
    return out


def check_knn(name, k, cell=0.0):
    xyz, want_nbr, want_d2 = cloud(name)
    got, stats = wp().knn(xyz, k, cell=cell, stats=True)
    nbr, d2, stats = host(got.nbr), host(got.dist2), host(stats)
    print(f"{name} V {len(xyz)} k {k} cell {cell}: candidates per query {stats[:, 0].mean():.1f}, "
          f"share of queries that scanned every point {stats[:, 1].mean():.4f}; rows with a wrong id "
          f"{int((nbr != want_nbr[:, :k]).any(1).sum())}")
    assert nbr.dtype == np.int32 and d2.dtype == np.float64
    assert np.array_equal(nbr, want_nbr[:, :k])
    assert same_bits(d2, want_d2[:, :k])
    return stats


@pytest.mark.parametrize("k", (1, 10, 45, 64))
def test_knn_with_k_plus_one_points(k):
    check_knn(f"blob{k + 1}", k)


@pytest.mark.parametrize("name,k", [("blob64", 1), ("blob64", 10), ("blob64", 45), ("blob65", 1), ("blob65", 10),
                                    ("blob65", 45), ("blob65", 64), ("blob1000", 1), ("blob1000", 10), ("blob1000", 45),
                                    ("blob1000", 64), ("room20000", 1), ("room20000", 10), ("room20000", 45),
                                    ("room20000", 64)])
def test_knn_sizes(name, k):
    check_knn(name, k)


def test_knn_cell_edge_changes_nothing():
    for cell in (0.09, 0.02, 1.0):
        check_knn("room20000", 45, cell)


def test_knn_all_points_in_one_cell():
    stats = check_knn("one_cell", 45, cell=1.0)
    assert (stats[:, 1] == 0).all() and (stats[:, 0] == 200).all()
    check_knn("one_cell", 64)


def test_knn_far_point_scans_every_point():
    stats = check_knn("outlier", 45, cell=0.25)
    assert stats[417, 1] == 1 and stats[417, 0] >= 1000
    assert stats[:, 1].sum() < 50                         # the others stop after a few rings
    check_knn("outlier", 10)


@pytest.mark.parametrize("name", ("sheet", "line"))
def test_knn_anisotropic_clouds(name):
    check_knn(name, 45)
    check_knn(name, 10, cell=0.05)


def test_knn_ties_go_by_id():
    xyz, want_nbr, want_d2 = cloud("duplicates")
    assert (want_d2[:, 1] == 0).all()                     # every point has at least two twins
    check_knn("duplicates", 45)
    check_knn("duplicates", 64, cell=0.3)


@pytest.mark.parametrize("tag", TAGS)
def test_knn_reproduces_the_reference(tag):
    gold = Golden(tag)
    got = wp().knn(gold.xyz, K_GEOF, cell=0.09)
    nbr, d2 = host(got.nbr), host(got.dist2)
    assert np.array_equal(nbr.flatten().astype(np.uint32), gold.target2)
    assert np.array_equal(nbr[:, :K_ADJ].flatten().astype(np.uint32), gold.target)
    assert same_bits(np.sqrt(d2[:, :K_ADJ]).flatten().astype(np.float32), gold.distances)


# ---- 3: geometric features ---------------------------------------------------------------------------------------------

def check_geof(name, xyz, nbr, k):
    want = ref.geof(xyz, nbr)
    got = wp().geometric_features(xyz, nbr)
    geof, cov, ev = host(got.geof), host(got.cov), host(got.ev)
    assert geof.dtype == np.float32 and cov.dtype == ev.dtype == np.float64
    trace = want["trace"]
    report(f"{name} covariance", np.abs(cov - want["cov"]), (ref.cov_tol(k) * trace)[:, None])
    report(f"{name} eigenvalues", np.abs(ev - want["ev"]), (ref.EV_TOL * trace)[:, None])
    assert (ev >= 0).all() and (np.diff(ev, axis=1) <= 0).all()
    tol = ref.feature_tolerances(want["ev"], trace, want["gap"])
    for j, fname in enumerate(("linearity", "planarity", "scattering")):
        report(f"{name} {fname}", np.abs(geof[:, j].astype(np.float64) - want["geof64"][:, j]),
               tol[:, j] + ref.step32(want["geof64"][:, j]))
    keep = want["gap"] > ref.GAP_MIN
    print(f"{name}: GAP_MIN {ref.GAP_MIN:.3g}, smallest relative eigen-gap {float(want['gap'].min()):.3g}, "
          f"share left out of the verticality comparison {1 - keep.mean():.4f}")
    report(f"{name} verticality", np.abs(geof[keep, 3].astype(np.float64) - want["geof64"][keep, 3]),
           tol[keep, 3] + ref.step32(want["geof64"][keep, 3]))
    return keep, geof


@pytest.mark.parametrize("tag", TAGS)
def test_geof_on_the_fixture_rooms(tag):
    gold = Golden(tag)
    keep, geof = check_geof(tag, gold.xyz, gold.knn()[0], K_GEOF)
    assert 1 - keep.mean() <= 0.01
    assert np.isfinite(geof).all()


def test_geof_exactly_collinear_and_coplanar():
    i = np.arange(40, dtype=np.float32)
    line = np.stack([0.25 * i, 0.5 * i, 0.5 * i], 1) + np.float32(8.0)            # exact in fp32
    nbr, _ = ref.knn(line, 10)
    keep, geof = check_geof("collinear", line, nbr, 10)
    assert np.array_equal(geof[:, 0], np.ones(40, np.float32)) or np.abs(geof[:, 0] - 1).max() < 1e-6
    a, b = np.meshgrid(np.arange(12, dtype=np.float32), np.arange(9, dtype=np.float32), indexing="ij")
    plane = np.stack([0.25 * a.ravel() + 3, 0.375 * b.ravel() - 5, np.full(a.size, 1.5)], 1).astype(np.float32)
    nbr, _ = ref.knn(plane, 20)
    keep, geof = check_geof("coplanar", plane, nbr, 20)
    assert np.abs(geof[:, 2]).max() < 1e-6                # scattering
    # the plane is horizontal: the two eigenvectors that carry weight have no z component
    assert np.abs(geof[:, 3]).max() < 1e-6


def test_geof_of_coincident_points_is_nan():
    xyz = np.full((46, 3), 7.25, np.float32)
    nn = wp().knn(xyz, 45)
    nbr = host(nn.nbr)
    assert np.array_equal(nbr, ref.knn(xyz, 45)[0]) and (host(nn.dist2) == 0).all()
    got = wp().geometric_features(xyz, nn.nbr)
    want = ref.geof(xyz, nbr)
    assert np.isnan(want["geof"]).all()
    assert np.isnan(host(got.geof)).all()
    assert (host(got.ev) == 0).all() and (host(got.cov) == 0).all()


# ---- 4: assembly -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag", TAGS)
def test_assembly(tag):
    gold = Golden(tag)
    w = wp()
    nn = w.knn(gold.xyz, K_GEOF)
    gf = w.geometric_features(gold.xyz, nn.nbr)
    rgb = torch.from_numpy(gold.rgb).cuda()
    features, source, target, distances, weight, mean = w.edge_features(gf.geof, rgb, nn, K_ADJ, 1.)
    dist, mean = host(distances), host(mean)
    assert mean.dtype == np.float32 and mean.shape == (1, )
    exact = math.fsum(float(d) for d in dist) / len(dist)
    print(f"{tag}: device mean {float(mean[0]):.9g}, fsum mean {exact:.17g}, reference mean {float(gold.mean):.9g}, "
          f"difference in fp32 steps {abs(float(mean[0]) - exact) / float(ref.step32(exact)):.3g}")
    assert abs(float(mean[0]) - exact) <= float(ref.step32(exact))
    want = ref.assemble(host(gf.geof), gold.rgb, host(nn.nbr), host(nn.dist2), K_ADJ, 1., mean=mean[0])
    assert same_bits(host(features), want["features"])
    assert np.array_equal(host(source).view(np.uint32), want["source"])
    assert np.array_equal(host(target).view(np.uint32), want["target"])
    assert same_bits(dist, want["distances"])
    assert same_bits(host(weight), want["edge_weight"])
    # against what the reference computed
    assert np.array_equal(host(source).view(np.uint32), gold.source) and np.array_equal(host(target).view(np.uint32), gold.target)
    assert same_bits(dist, gold.distances)
    margin = ref.edge_weight_margin(gold.distances, mean[0], gold.mean)
    report(f"{tag} edge_weight against the reference", np.abs(host(weight).astype(np.float64) - gold.edge_weight), margin)


# ---- 5: the whole path -------------------------------------------------------------------------------------------------

def raw_room():
    if "raw" not in _CACHE:
        _CACHE["raw"] = ref.make_room(9, n=30000, size=(2.0, 1.5, 1.2))
    return _CACHE["raw"]


def components_solver(features, source, target, edge_weight, reg_strength):
    """stands in for libcp.cutpursuit: connected components of the graph thresholded on feature distance (host)"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    assert features.dtype == np.float32 and source.dtype == target.dtype == np.uint32 and edge_weight.dtype == np.float32
    assert features.shape[1] == 7 and len(source) == len(target) == len(edge_weight)
    V = len(features)
    near = np.linalg.norm(features[source] - features[target], axis=1) < 0.35
    g = coo_matrix((np.ones(int(near.sum())), (source[near], target[near])), shape=(V, V))
    n, ids = connected_components(g, directed=False)
    return [np.nonzero(ids == c)[0] for c in range(n)], ids.astype(np.uint32)


def test_partition_inputs_equals_the_stages_and_repeats():
    xyz, rgb = raw_room()
    w = wp()
    a = w.partition_inputs(xyz, rgb)
    pr = w.prune(xyz, 0.03, rgb)
    nn = w.knn(pr.xyz, 45)
    gf = w.geometric_features(pr.xyz, nn.nbr)
    features, source, target, distances, weight, mean = w.edge_features(gf.geof, pr.rgb, nn, 10, 1.)
    stages = (features, source, target, weight, distances, mean, nn.nbr, pr.p2v, pr.xyz, pr.rgb)
    print(f"N {len(xyz)} V {int(pr.xyz.shape[0])} E {int(source.numel())}")
    for name, x, y in zip(a._fields, a, stages):
        assert same_bits(host(x), host(y)), name
    b = w.partition_inputs(torch.from_numpy(xyz).cuda(), torch.from_numpy(rgb).cuda())
    for name, x, y in zip(a._fields, a, b):
        assert same_bits(host(x), host(y)), name
    want = ref.prune(xyz, 0.03, rgb)
    assert np.array_equal(host(a.p2v).astype(np.uint32), want["p2v"]) and same_bits(host(a.xyz), want["xyz"])
    args = a.solver_args(0.03)
    assert [x.dtype for x in args[:4]] == [np.float32, np.uint32, np.uint32, np.float32] and args[4] == 0.03


def test_generate_superpoints_with_a_stand_in_solver():
    xyz, rgb = raw_room()
    w = wp()
    ids = w.generate_superpoints(xyz, rgb, components_solver)
    inputs = w.partition_inputs(xyz, rgb)
    _, in_component = components_solver(*inputs.solver_args())
    print(f"N {len(xyz)} V {len(in_component)} superpoints {int(ids.max()) + 1}")
    assert ids.shape == (len(xyz), ) and len(np.unique(ids)) == int(ids.max()) + 1 > 1
    p2v = host(inputs.p2v)
    assert np.array_equal(ids, in_component[p2v]) and np.array_equal(inputs.to_points(in_component), ids)
    dev_ids = inputs.to_points(torch.from_numpy(in_component.astype(np.int64)).cuda())
    assert dev_ids.is_cuda and np.array_equal(host(dev_ids), ids)
    assert np.array_equal(w.generate_superpoints(xyz, rgb, components_solver), ids)


def test_every_refusal_raises():
    import wsis_native
    w = wp()
    xyz, rgb = raw_room()
    xyz, rgb = xyz[:500], rgb[:500]
    nan, inf = xyz.copy(), xyz.copy()
    nan[77, 1], inf[3, 2] = np.nan, np.inf
    bad = [lambda: w.prune(xyz.astype(np.float64), 0.03, rgb), lambda: w.prune(xyz, 0.03, rgb.astype(np.int16)),
           lambda: w.prune(xyz[:0], 0.03, rgb[:0]), lambda: w.prune(nan, 0.03, rgb), lambda: w.prune(inf, 0.03, rgb),
           lambda: w.prune(xyz, 0.03, rgb, np.full(500, 14, np.uint8), 13), lambda: w.prune(xyz, 0.0, rgb),
           lambda: w.knn(nan, 10), lambda: w.knn(inf, 10), lambda: w.knn(xyz, 65), lambda: w.knn(xyz[:45], 45),
           lambda: w.knn(xyz.astype(np.float64), 10), lambda: w.partition_inputs(xyz, rgb, k_nn_adj=46),
           lambda: w.partition_inputs(xyz, rgb, k_nn_geof=65), lambda: w.partition_inputs(nan, rgb),
           lambda: w.partition_inputs(xyz[:20], rgb[:20]), lambda: w.prune(torch.from_numpy(xyz), 0.03, rgb, device="cpu"),
           lambda: w.geometric_features(xyz, np.zeros((500, 65), np.int32)),
           lambda: w.generate_superpoints(xyz.astype(np.float64), rgb, components_solver)]
    for i, f in enumerate(bad):
        with pytest.raises(wsis_native.WsisError):
            f()
            print("not refused:", i)
    # the library itself refuses what the Python layer checks first
    lib = wsis_native.hip()
    x = torch.from_numpy(xyz).cuda()
    assert lib.wsis_pt_knn_workspace_bytes(0) < 0
    ws = torch.empty(lib.wsis_pt_knn_workspace_bytes(500), dtype=torch.uint8, device="cuda")
    nbr = torch.empty((500, 64), dtype=torch.int32, device="cuda")
    d2 = torch.empty((500, 64), dtype=torch.float64, device="cuda")
    for V, k in ((500, 65), (500, 0), (45, 45)):
        assert lib.wsis_pt_knn(x.data_ptr(), V, k, 0.0, nbr.data_ptr(), d2.data_ptr(), None, ws.data_ptr(), ws.numel(),
                               wsis_native.stream_ptr()) != 0
    assert lib.wsis_pt_knn(x.data_ptr(), 500, 10, 0.0, nbr.data_ptr(), d2.data_ptr(), None, ws.data_ptr(), 1024,
                           wsis_native.stream_ptr()) != 0


def test_peak_memory_is_linear_in_the_points():
    """c = the bytes per point of everything partition_inputs allocates, with no credit for reuse and V <= N: inputs 15,
    bin rows 32, p2v 4 + 8 (its int64 copy), point CSR 8, pruned cloud 19, neighbour lists 45 * 12 = 540, features and
    moments 16 + 48 + 24 = 88, assembly 28 + 4 * 40 = 188 -> 902, plus the four workspaces over N.  The
    bound linear in N is the check: anything of order V^2 (8 V^2 = 94 GB here) would break it."""
    import wsis_native
    N = 200000
    xyz, rgb = ref.make_room(21, n=N, size=(6.0, 5.0, 3.0))
    lib = wsis_native.hip()
    ws = (lib.wsis_voxelize_idx_workspace_bytes(N) + lib.wsis_segment_csr_workspace_bytes(N, N) +
          lib.wsis_pt_knn_workspace_bytes(N) + lib.wsis_pt_edge_features_workspace_bytes(N, 10))
    c = 902 + ws / N
    x, col = torch.from_numpy(xyz).cuda(), torch.from_numpy(rgb).cuda()
    wp().partition_inputs(x[:1000], col[:1000])          # library handles, allocator pools
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = wp().partition_inputs(x, col)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    V = int(out.xyz.shape[0])
    print(f"N {N} V {V}: c = {c:.1f} bytes per point (workspaces {ws / N:.1f}); peak {peak} bytes = {peak / N:.1f} per point; "
          f"bound {c * N + (16 << 20):.0f}")
    assert peak <= c * N + (16 << 20)                       # the check: linear in N, so nothing of order V^2 (8 V^2 = 94 GB)
