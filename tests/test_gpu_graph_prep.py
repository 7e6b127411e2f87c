"""GPU: the superpoint-graph preparation (3d-wsis_amd/wsis_graph_prep.py, csrc/graphprep.hip) against

1. what the reference's builders computed (tests/golden/graph_prep_golden.npz): edges, vertex ids, labels, is1ins and
   counts equal; centroids within gap_c and offset vectors within 2 gap_c (the reference's centres are sequential
   float32 means; gap_c, stored with the fixture, bounds that of a superpoint's points); features within what
   tests/graph_prep_ref.py propagates from gap_c and EV_TOL through each expression, plus one float32 step; standardised
   columns within that tolerance over the column scale, plus two float32 steps;
2. the numpy oracle evaluated in float64, kernel by kernel at the kernels' own edges: centroid within one float32 step,
   mean and std of the deltas within two, eigenvalues within EV_TOL * trace, everything discrete equal;
3. conditions: a second call is bit-identical, bad input raises, no call allocates anything of order S*N or S^2, and the
   graph feeds DeviceScenePrep.upload and clustering_in_graph unchanged.

Every figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

import graph_prep_ref as ref
from test_graph_prep_host import Golden, TAGS

pytestmark = pytest.mark.gpu

ROW_LENGTHS = (1, 2, 3, 63, 64, 65, 129, 5000)


def gp():
    import wsis_graph_prep
    return wsis_graph_prep


def steps32(got, want):
    """|got - want| in float32 steps at |want|"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return np.abs(got - want) / ref.step32(want)


def report(name, err, tol):
    err, tol = np.asarray(err, np.float64), np.broadcast_to(np.asarray(tol, np.float64), np.shape(err))
    worst = float((err / np.maximum(tol, 1e-300)).max()) if err.size else 0.0
    print(f"{name}: largest error {float(err.max()) if err.size else 0.0:.3g}, largest error / tolerance {worst:.3g}")
    assert (err <= tol).all(), name


# ---- 1: the reference's graphs ---------------------------------------------------------------------------------------

def _build(gold, **kw):
    rng = np.random.RandomState(gold.seed)
    if gold.kind == "s3dis":
        return gp().build_graph_s3dis(gold.xyz, gold.superpoint, gold.sem, gold.ins, rng, **kw)
    return gp().build_graph_scannet(gold.xyz, gold.faces.astype(np.int64), gold.superpoint, gold.sem, gold.ins, rng, **kw)


@pytest.mark.parametrize("tag", TAGS)
def test_builder_reproduces_the_reference(tag):
    gold = Golden(tag)
    o = gold.oracle()
    g = _build(gold)
    gold.check_discrete(g.edges, g.is1ins, g.vs)
    assert set(g.vs) == {"v", "semantic_label", "instance_label", "superpoint_feature", "superpoint_offset_vector"}
    spf, want = g.vs["superpoint_feature"], gold.vs_superpoint_feature
    assert spf.dtype == np.float64 and spf.shape == want.shape
    report("centroid", np.abs(spf[:, :3] - want[:, :3]), gold.gap_c)
    off = g.vs["superpoint_offset_vector"]
    assert off.dtype == np.float64
    report("offset vector", np.abs(off - gold.vs_superpoint_offset_vector), 2 * gold.gap_c)
    ft = o["features"]
    ftol = ref.feature_tolerances(ft, gold.gap_c)
    for j, name in ((3, "length"), (4, "surface"), (5, "volume")):
        report(name, np.abs(spf[:, j] - want[:, j]), ftol[name] + ref.step32(want[:, j]))
    assert g.f.dtype == np.float32 and g.f.shape == gold.f.shape
    if gold.kind == "s3dis":
        tol = ref.edge_tolerances(ft, gold.edges, gold.f, gold.gap_c)
    else:
        tol = ref.edge_tolerances(ft, gold.edges, o["f_raw"], gold.gap_c) / o["f_scale"] + 2 * ref.step32(gold.f)
    for c in range(13):
        report(f"f[:, {c}]", np.abs(g.f[:, c].astype(np.float64) - gold.f[:, c]), tol[:, c])


def test_scannet_raw_features_before_the_standardisation():
    gold = Golden("scannet_a")
    o = gold.oracle()
    g = _build(gold, standardize=False)
    tol = ref.edge_tolerances(o["features"], gold.edges, o["f_raw"], gold.gap_c)
    report("raw f", np.abs(g.f.astype(np.float64) - o["f_raw"]), tol)


# ---- 2: kernel by kernel against the oracle in float64 ---------------------------------------------------------------

def _rows_scene(seed=3):
    """superpoints of the ROW_LENGTHS, then a collinear, a coplanar and an all-equal one and one 100 m from the origin"""
    rng = np.random.default_rng(seed)
    pts, sp = [], []
    for n in ROW_LENGTHS:
        pts.append(rng.uniform(-2, 2, 3) + rng.standard_normal((n, 3)) * [0.2, 0.1, 0.03])
    t = np.linspace(-1, 1, 70)[:, None]
    pts.append(np.asarray([0.5, -0.3, 1.0]) + t * np.asarray([[0.3, -0.2, 0.5]]))                          # collinear
    pts.append(rng.standard_normal((90, 2)) @ np.asarray([[0.2, 0.1, 0.0], [0.0, 0.1, 0.3]]) + 1.0)        # coplanar
    pts.append(np.full((9, 3), 100.1))                                                                      # all equal
    pts.append(100.0 + rng.standard_normal((300, 3)) * [0.2, 0.05, 0.01])                                   # far away
    for s, p in enumerate(pts):
        sp.append(np.full(len(p), s))
    xyz, sp = np.concatenate(pts).astype(np.float32), np.concatenate(sp)
    perm = rng.permutation(len(xyz))
    return xyz[perm], sp[perm].astype(np.int64)


def test_moments_at_every_row_length_and_degenerate_shape():
    xyz, sp = _rows_scene()
    o = ref.superpoint_features(xyz, sp, wide=True)
    scene = gp().GraphScene(xyz, sp)
    ft = gp().superpoint_features(scene)
    ft2 = gp().superpoint_features(scene)
    for a, b in zip(ft, ft2):
        assert torch.equal(a, b)
    assert ft.count.dtype == torch.int64 and np.array_equal(ft.count.cpu().numpy(), o["count"].astype(np.int64))
    assert np.array_equal(o["count"][:len(ROW_LENGTHS)], ROW_LENGTHS)
    s = steps32(ft.centroid.cpu().numpy(), o["centroid"])
    print("centroid: largest difference in float32 steps", s.max())
    assert s.max() <= 1
    one = np.nonzero(o["count"] == 1)[0][0]
    assert np.array_equal(ft.centroid.cpu().numpy()[one], xyz[sp == one][0])
    trace = o["cov"][:, :3].sum(1)
    big = o["count"] >= 3
    report("eigenvalues", np.abs(ft.ev.cpu().numpy() - o["ev"])[big], (ref.EV_TOL * trace)[big, None])
    report("covariance", np.abs(ft.cov.cpu().numpy() - o["cov"]), (ref.EV_TOL * trace)[:, None])
    tol = ref.feature_tolerances(o, 0.0)
    for name in ("length", "surface", "volume"):
        got, want = getattr(ft, name).cpu().numpy().astype(np.float64), o[name].astype(np.float64)
        report(name, np.abs(got - want), np.where(o["count"] == 2, 0.0, tol[name]) + ref.step32(want))
    flat = len(ROW_LENGTHS) + 2                       # all equal: exactly zero
    assert o["count"][flat] == 9 and not ft.ev.cpu().numpy()[flat].any() and float(ft.length[flat]) == 0.0
    arr = ft.as_array()
    assert arr.dtype == np.float64 and arr.shape == (len(trace), 7) and np.array_equal(arr[:, 6], o["count"])


def test_label_mode_ties_and_many_labels():
    rng = np.random.default_rng(5)
    labels, sp = [], []

    def row(values):
        sp.append(np.full(len(values), len(labels)))
        labels.append(np.asarray(values))
    for n in ROW_LENGTHS:
        row(rng.choice([-100, 2, 7, 11], n))
    row([5] * 20 + [3] * 20 + [9] * 5)                        # a tie: the smaller value
    row([7] * 33 + [-100] * 33 + [1] * 10)                    # a tie with -100: -100 is the smaller value
    row([-100] * 40 + [4] * 30)                               # a -100 majority
    row(np.arange(130) * 3 - 100)                             # 130 distinct labels: the first (smallest) one
    row([8] * 64 + [6] * 65)                                  # 64 against 65: more than one ballot per count
    labels, sp = np.concatenate(labels).astype(np.int64), np.concatenate(sp).astype(np.int64)
    perm = rng.permutation(len(sp))
    labels, sp = labels[perm], sp[perm]
    xyz = rng.uniform(-1, 1, (len(sp), 3)).astype(np.float32)
    sem = np.where(labels == -100, -100, labels % 5).astype(np.float64)
    want = ref.superpoint_labels(xyz, sp, sem, labels, wide=True)
    scene = gp().GraphScene(xyz, sp)
    got = gp().superpoint_labels(scene, sem, labels)
    assert got.sp_semantic.dtype == got.sp_instance.dtype == np.float64
    assert np.array_equal(got.sp_instance, want[1]) and np.array_equal(got.sp_semantic, want[0])
    base = len(ROW_LENGTHS)
    assert list(got.sp_instance[base:base + 5]) == [3, -100, -100, -100, 6]
    n_max = max(np.bincount(sp).max(), np.unique(labels, return_counts=True)[1].max())
    report("offset vector", np.abs(got.sp_offset_vector - want[2]), 2 * ref.gap_c(xyz, int(n_max)))
    again = gp().superpoint_labels(scene, sem, labels)
    assert all(np.array_equal(a, b) for a, b in zip(got, again))
    none = gp().superpoint_labels(scene, None, None)
    assert (none.sp_semantic == -100).all() and (none.sp_instance == -100).all() and not none.sp_offset_vector.any()


def _clear_centres(make, ks=(), radius=None):
    """the first seed whose centres keep every neighbour decision clear of ``gap`` = gap_c with n_max = 0, the rounding
    of a centre that is stored in float32: every centre distance and the cut after the k-th neighbour above
    4 sqrt(3) gap for each k of ``ks``; no distance within 2 sqrt(3) gap of ``radius`` and consecutive candidate
    distances inside it more than 4 sqrt(3) gap apart"""
    for seed in range(400):
        centres = make(np.random.default_rng(seed)).astype(np.float32)
        gap = ref.gap_c(centres, 0)
        if all(ref.neighbours_clear(centres, k=k, gap=gap) for k in ks) and \
                (radius is None or ref.neighbours_clear(centres, radius=radius, gap=gap)):
            return centres, gap
    raise AssertionError("no seed clear of rounding")


def _same_lists(centres, k, radius, gap):
    """``gap`` None: duplicate centres, whose ties are exact on both sides and go by id"""
    want = ref.neighbor_lists(centres, k, radius)
    if gap is not None:
        assert gap > 0 and ref.neighbours_clear(centres, k=k if np.isinf(radius) else None,
                                                radius=None if np.isinf(radius) else radius, gap=gap)
    got = gp().neighbor_lists(centres, k, radius)
    again = gp().neighbor_lists(centres, k, radius)
    for a, b, w in zip(got, again, want):
        assert torch.equal(a, b)
        assert a.cpu().numpy().dtype == w.dtype and np.array_equal(a.cpu().numpy(), w)
    return want


@pytest.mark.parametrize("S", [1, 2, 11, 12, 63, 64, 65, 700])
def test_neighbours_at_every_size(S):
    radius = 0.3 if S == 700 else 0.5
    centres, gap = _clear_centres(lambda rng: rng.uniform(0, 1, (S, 3)) * [3.0, 2.0, 1.0], (1, 10, 128), radius)
    for k in (1, 10, 128):
        nbr, _, count = _same_lists(centres, k, np.inf, gap)
        assert (count == S - 1).all() and ((nbr >= 0).sum(1) == min(k, S - 1)).all()
    nbr, _, count = _same_lists(centres, 10, radius, gap)
    if S == 700:
        assert count.max() > 10 and (nbr[count > 10] >= 0).all()          # a radius with count > k


def test_neighbours_duplicates_empty_radius_and_crowded_radius():
    base, gap = _clear_centres(lambda rng: rng.uniform(0, 1, (40, 3)) * 2, (1, 10), 1e-4)
    centres = np.concatenate([base, base[:25], base[:5]])                 # duplicates: distance 0, ties by id
    for k in (1, 10, 128):
        nbr, dist2, _ = _same_lists(centres, k, np.inf, None)
    assert nbr[0, 0] == 40 and nbr[0, 1] == 65 and dist2[0, 0] == 0 and dist2[0, 1] == 0
    nbr, dist2, count = _same_lists(base, 10, 1e-4, gap)                  # a radius with no candidate
    assert (count == 0).all() and (nbr == -1).all() and np.isinf(dist2).all()
    tight, gap = _clear_centres(lambda rng: rng.uniform(0, 1, (60, 3)) * 0.2, (10,), 0.5)   # everything within the radius
    nbr, _, count = _same_lists(tight, 10, 0.5, gap)
    assert (count == 59).all() and (nbr >= 0).all()


def test_edge_features_at_every_pair_count():
    rng = np.random.default_rng(9)
    sizes = [1, 2, 63, 64, 65, 1000, 1000, 64, 1500, 3, 130]
    pts, sp = [], []
    for s, n in enumerate(sizes):
        pts.append(rng.uniform(-2, 2, 3) + rng.standard_normal((n, 3)) * [0.2, 0.1, 0.03])
        sp.append(np.full(n, s))
    xyz, sp = np.concatenate(pts).astype(np.float32), np.concatenate(sp).astype(np.int64)
    perm = rng.permutation(len(xyz))
    xyz, sp = xyz[perm], sp[perm]
    # 1, 2, 63, 64, 65 and 1000 pairs, each with the source larger and with the target larger (both directions of an
    # edge), and equal rows of 64 and of 1000 points, where nothing is sampled
    edges = np.asarray(sorted([(0, 8), (8, 0), (1, 8), (8, 1), (2, 10), (10, 2), (3, 4), (4, 3), (4, 10), (10, 4), (5, 8),
                               (8, 5), (3, 7), (7, 3), (5, 6), (6, 5), (0, 1), (1, 0), (9, 1), (1, 9)]), dtype=np.int64)
    scene = gp().GraphScene(xyz, sp)
    ft = gp().superpoint_features(scene)
    counts = ft.count.cpu().numpy()
    samples = gp().draw_samples(counts, edges, np.random.RandomState(4))
    assert np.array_equal(samples[0], ref.draw_samples(counts, edges, np.random.RandomState(4))[0])
    pairs = sorted(set(np.minimum(counts[edges[:, 0]], counts[edges[:, 1]]).tolist()))
    assert pairs == [1, 2, 63, 64, 65, 1000]
    got = gp().edge_features(scene, ft, edges, None, samples=samples)
    again = gp().edge_features(scene, ft, edges, np.random.RandomState(4))
    assert torch.equal(got, again) and got.dtype == torch.float32 and tuple(got.shape) == (len(edges), 13)
    got = got.cpu().numpy()
    o = ref.superpoint_features(xyz, sp, wide=True)
    want = ref.edge_features(xyz, sp, o, edges, samples, wide=True)
    s = steps32(got[:, :6], want[:, :6])
    single = np.minimum(counts[edges[:, 0]], counts[edges[:, 1]]) == 1
    print("delta mean / std: largest difference in float32 steps", s.max())
    assert s.max() <= 2 and np.array_equal(got[single, :6], want[single, :6]) and not got[single, 3:6].any()
    # columns 6-12 are float32 expressions of the device's own features: evaluated in numpy, they are the same bits
    own = {k: getattr(ft, k).cpu().numpy() for k in ("centroid", "length", "surface", "volume")}
    own["count"] = counts.astype(np.uint64)
    assert np.array_equal(got[:, 6:], ref.edge_features(xyz, sp, own, edges, samples, wide=True)[:, 6:])


# ---- 3: conditions ---------------------------------------------------------------------------------------------------

def test_a_second_call_is_bit_identical():
    for tag in ("s3dis_a", "scannet_a"):
        a, b = _build(Golden(tag)), _build(Golden(tag))
        assert a.f.tobytes() == b.f.tobytes() and np.array_equal(a.edges, b.edges) and np.array_equal(a.is1ins, b.is1ins)
        for k in a.vs:
            assert np.asarray(a.vs[k]).tobytes() == np.asarray(b.vs[k]).tobytes(), k


def test_bad_input_raises():
    import wsis_native
    gold = Golden("s3dis_a")
    m = gp()
    for bad in (-1, len(gold.xyz)):                            # a face vertex outside the points: refused on the host
        with pytest.raises(ValueError):
            m.face_edges(np.asarray([[0, 1, 2], [3, bad, 4]]), gold.superpoint)
    sp = gold.superpoint.copy()
    sp[sp == 17] = 18                                          # superpoint 17 has no points
    with pytest.raises(wsis_native.WsisError):
        m.GraphScene(gold.xyz, sp)
    with pytest.raises(wsis_native.WsisError):
        m.GraphScene(gold.xyz.astype(np.float64), gold.superpoint)
    with pytest.raises(wsis_native.WsisError):
        m.neighbor_lists(gold.xyz[:200], 129)
    with pytest.raises(wsis_native.WsisError):
        m.GraphScene(gold.xyz, gold.superpoint, device="cpu")
    with pytest.raises(wsis_native.WsisError):
        m.build_graph_s3dis(gold.xyz, gold.superpoint, gold.sem, gold.ins, np.random.RandomState(0), k=129)


def test_no_call_allocates_anything_like_s_times_n_or_s_squared():
    """N = 200,000 points, S = 3,000 superpoints: the peak device allocation above what is allocated when a call starts
    stays below 100 N bytes + 16 MiB (one S x N byte mask would be 600 MB, one S x S fp64 table 72 MB)"""
    m = gp()
    N, S = 200000, 3000
    rng = np.random.default_rng(11)
    centres = rng.uniform(0, 1, (S, 3)) * [12.0, 10.0, 3.0]
    sp = rng.integers(0, S, N)
    sp[:S] = np.arange(S)
    xyz = (centres[sp] + rng.standard_normal((N, 3)) * 0.05).astype(np.float32)
    ins = (sp % 40).astype(np.int64)
    sem = ins % 13
    faces = rng.integers(0, N, (5000, 3))
    limit = 100 * N + (16 << 20)
    peaks = {}

    def measured(name, fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        peaks[name] = torch.cuda.max_memory_allocated() - base
        return out

    scene = measured("scene", lambda: m.GraphScene(xyz, sp))
    ft = measured("features", lambda: m.superpoint_features(scene))
    measured("labels", lambda: m.superpoint_labels(scene, sem, ins, ft))
    nl = measured("neighbours", lambda: m.neighbor_lists(ft.centroid, 10))
    measured("neighbours, radius", lambda: m.neighbor_lists(ft.centroid, 128, 0.3))
    measured("face edges", lambda: m.face_edges(faces, scene.superpoint))
    s = torch.arange(S, device="cuda")[:, None].expand(S, 10)
    edges = m._symmetric_edges(s.reshape(-1), nl.nbr.long().reshape(-1), S)
    f = measured("edge features", lambda: m.edge_features(scene, ft, edges, np.random.RandomState(0)))
    measured("standardise", lambda: m.standardize_features(f))
    del scene, ft, nl, f, edges, s
    g = measured("s3dis", lambda: m.build_graph_s3dis(xyz, sp, sem, ins, np.random.RandomState(0)))
    measured("scannet", lambda: m.build_graph_scannet(xyz, faces, sp, sem, ins, np.random.RandomState(0)))
    print("peak bytes above the start of the call:", peaks, "limit", limit)
    assert max(peaks.values()) < limit, peaks
    assert g.vcount == S and len(g.edges) >= 10 * S and np.isfinite(g.f).all()


def test_scannet_graph_feeds_scene_prep_and_grouping_unchanged(tmp_path):
    import harness
    import inference
    import wsis_datasets as datasets
    sc = harness.make_scene(5, room=(1.6, 1.3, 1.1), n_box=4)
    tup, _ = datasets.synthetic_scene_to_reference_format(sc)
    xyz, _, sem, ins, sp, _ = tup
    rng = np.random.default_rng(1)
    from scipy.spatial import cKDTree
    pick = rng.choice(len(xyz), 3000, replace=False)
    near = cKDTree(xyz).query(xyz[pick], k=8)[1]
    faces = np.stack([pick, near[:, 3], near[:, 7]], 1)
    graph = gp().build_graph_scannet(xyz, faces, sp, sem, ins, np.random.RandomState(3))
    S = sc["S"]
    assert graph.vcount == S and graph.f.shape == (len(graph.edges), 13) and np.isfinite(graph.f).all()
    assert np.array_equal(graph.edges, np.asarray(sorted(set(map(tuple, graph.edges.tolist())))))
    assert np.array_equal(graph.edges[np.lexsort((graph.edges[:, 0], graph.edges[:, 1]))][:, ::-1], graph.edges)   # symmetric
    graph.save(tmp_path / "g.npz")
    back = datasets.PlainGraph.load(tmp_path / "g.npz")
    assert np.array_equal(back.f, graph.f) and np.array_equal(back.is1ins, graph.is1ins)
    prep = datasets.DeviceScenePrep(max_npoint=250000, aug=False, test_mode=True, seed=0, device="cuda")
    item = prep(prep.upload(tup, graph)).to_host()
    assert item[8].vcount == S and np.array_equal(item[8].edges, graph.edges) and np.array_equal(item[8].f, graph.f)
    import wsis_weak_labels
    scene = wsis_weak_labels.WeakLabelScene(xyz, sp)
    assert np.abs(scene.centre.cpu().numpy() - graph.vs["superpoint_feature"][:, :3]).max() < 1e-4
    sem_pred, off, occ, size = harness.synthetic_predictions(sc, 5)
    conf, label_id, masks = inference.clustering_in_graph("s", xyz, sp, (graph.edges[:, 0], graph.edges[:, 1]), sem_pred,
                                                          off, occ, size)
    assert len(conf) == len(label_id) == len(masks) > 0 and masks.shape[1] == len(xyz)
