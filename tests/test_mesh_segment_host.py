"""CPU: the two sweeps of the mesh segmentation.

1. tests/mesh_segment_ref.py against itself: the sequential sweeps and the round formulation, two constructions that
   share no code, give the same segments;
2. ``wsis_host_mesh_merge`` (csrc/host_ops.cpp, through ``wsis_graph_prep.mesh_merge``) against the sequential
   restatement: ids equal, on the same inputs and on hand cases built so that each rule decides the outcome.

Every comparison is equality of integers.  No device is touched."""
import numpy as np
import pytest

import mesh_segment_ref as ref

F32 = np.float32
KT = F32(ref.K_THRESH)


def merge(a, b, w, V, k_thresh=ref.K_THRESH, seg_min_verts=ref.SEG_MIN_VERTS):
    import wsis_graph_prep
    return wsis_graph_prep.mesh_merge(a, b, w, V, k_thresh, seg_min_verts)


def random_graph(V, seed):
    """E = 5 V edges (self loops and repeats as they fall), weights from 64 distinct fp32 values: ties occur"""
    rng = np.random.RandomState(seed)
    E = 5 * V
    a, b = rng.randint(0, V, E).astype(np.int32), rng.randint(0, V, E).astype(np.int32)
    values = (rng.rand(64) * 0.03).astype(F32)
    return ref.sort_edges(a, b, values[rng.randint(0, 64, E)]) + (V,)


def heightfield_graph():
    xyz, faces = ref.heightfield(60, seed=5)
    vn = ref.vertex_normals(len(xyz), faces, ref.face_normals(xyz, faces))
    a, b = ref.edges_of_faces(faces)
    return ref.sort_edges(a, b, ref.edge_weights(xyz, vn, a, b)) + (len(xyz),)


_GRAPHS = {}


def graph(name):
    if name not in _GRAPHS:
        _GRAPHS[name] = {"random300": lambda: random_graph(300, 1), "random2000": lambda: random_graph(2000, 2),
                         "heightfield60": heightfield_graph}[name]()
    return _GRAPHS[name]


GRAPHS = ("random300", "random2000", "heightfield60")
SETTINGS = ((ref.K_THRESH, ref.SEG_MIN_VERTS), (0.001, 1), (0.02, 50))


@pytest.mark.parametrize("k_thresh,seg_min_verts", SETTINGS)
@pytest.mark.parametrize("name", GRAPHS)
def test_the_round_formulation_gives_the_sequential_segments(name, k_thresh, seg_min_verts):
    a, b, w, V = graph(name)
    ids, S = ref.sweeps(a, b, w, V, k_thresh, seg_min_verts)
    ids_r, S_r, rounds1, rounds2 = ref.sweeps_by_rounds(a, b, w, V, k_thresh, seg_min_verts)
    print(f"{name}: {V} vertices, {len(w)} edges, {S} segments, rounds {rounds1} + {rounds2}")
    assert S == S_r and np.array_equal(ids, ids_r)
    assert 1 <= S < V and ids.min() == 0 and ids.max() == S - 1


@pytest.mark.parametrize("k_thresh,seg_min_verts", SETTINGS)
@pytest.mark.parametrize("name", GRAPHS)
def test_host_merge_equals_the_restatement(name, k_thresh, seg_min_verts):
    a, b, w, V = graph(name)
    ids, S = ref.sweeps(a, b, w, V, k_thresh, seg_min_verts)
    got, n_seg = merge(a, b, w, V, k_thresh, seg_min_verts)
    assert got.dtype == np.int64 and got.shape == (V,) and n_seg == S
    assert np.array_equal(got, ids)


def both(a, b, w, V, seg_min_verts=1, k_thresh=ref.K_THRESH):
    """the hand cases: host op = restatement = rounds -> ids as a list"""
    a, b, w = np.asarray(a, np.int32), np.asarray(b, np.int32), np.asarray(w, F32)
    assert (np.diff(w) >= 0).all()
    want, S = ref.sweeps(a, b, w, V, k_thresh, seg_min_verts)
    got, n_seg = merge(a, b, w, V, k_thresh, seg_min_verts)
    assert np.array_equal(got, want) and n_seg == S
    assert np.array_equal(ref.sweeps_by_rounds(a, b, w, V, k_thresh, seg_min_verts)[0], want)
    return got.tolist()


def test_no_edges_and_no_vertices():
    assert both([], [], [], 5) == [0, 1, 2, 3, 4]
    assert both([], [], [], 5, seg_min_verts=20) == [0, 1, 2, 3, 4]
    got, n_seg = merge([], [], [], 0)
    assert got.shape == (0,) and n_seg == 0


def test_an_edge_at_the_threshold_is_accepted():
    """the test is w <= thr: w == kThresh joins, the next fp32 above it does not"""
    assert both([0], [1], [KT], 2) == [0, 0]
    assert both([0], [1], [np.nextafter(KT, F32(1))], 2) == [0, 1]


def test_a_shrinking_threshold_rejects_a_heavier_edge():
    """a chain 0-1-2-3 joined at w = 0 has thr = kThresh / 4 = 0.0025: the edge to vertex 4 at 0.003 is refused though
    it is far below kThresh; a component of two (thr = 0.005) accepts the same weight"""
    assert both([0, 1, 2, 3], [1, 2, 3, 4], [0, 0, 0, 0.003], 5) == [0, 0, 0, 0, 1]
    assert both([0, 1], [1, 2], [0, 0.003], 3) == [0, 0, 0]


def test_sweep_two_absorbs_below_the_minimum_only():
    """two chains joined at w = 0, of segMinVerts - 1 and of exactly segMinVerts vertices, each hanging on a big one by
    an edge far above every threshold: the smaller is absorbed, the other left alone"""
    m = ref.SEG_MIN_VERTS
    big = list(range(0, 30))
    small = list(range(30, 30 + m - 1))
    exact = list(range(30 + m - 1, 30 + 2 * m - 1))
    a, b, w = [], [], []
    for group in (big, small, exact):
        a += group[:-1]
        b += group[1:]
        w += [0.0] * (len(group) - 1)
    a += [small[0], exact[0]]
    b += [big[3], big[4]]
    w += [0.5, 0.5]
    ids = both(a, b, w, 30 + 2 * m - 1, seg_min_verts=m)
    assert ids == [0] * 30 + [0] * (m - 1) + [1] * m
    assert both(a, b, w, 30 + 2 * m - 1, seg_min_verts=1) == [0] * 30 + [1] * (m - 1) + [2] * m


def test_sweep_two_takes_the_first_edge_in_order():
    """a lone vertex between two segments joins across the lighter of its two edges"""
    a, b, w = [0, 3, 2, 2], [1, 4, 1, 3], [0, 0, 0.3, 0.4]
    assert both(a, b, w, 5, seg_min_verts=2) == [0, 0, 0, 1, 1]
    a, b, w = [0, 3, 2, 2], [1, 4, 3, 1], [0, 0, 0.3, 0.4]
    assert both(a, b, w, 5, seg_min_verts=2) == [0, 0, 1, 1, 1]


def test_a_repeated_edge_is_accepted_after_the_threshold_rose():
    """(0,1) twice at w = 0.012 > kThresh.  Alone, both copies are refused.  After 1 joined 2 and 0 joined 3 at 0.009 the
    thresholds stand at 0.009 + kThresh / 2 = 0.014 on both sides: a copy joins the two pairs and the other copy finds
    one component.

    A copy that was itself refused cannot be accepted later, whatever happens in between: a refusal means w > thr[c]
    for one of its components c, every later edge is at least as heavy, so c never joins anything again in sweep 1 and
    its threshold never changes.  The second part pins that: both copies and an edge between them in the order are
    refused at 0.0145 > 0.014."""
    assert both([0, 0], [1, 1], [0.012, 0.012], 4) == [0, 1, 2, 3]
    assert both([1, 0, 0, 0], [2, 3, 1, 1], [0.009, 0.009, 0.012, 0.012], 4) == [0, 0, 0, 0]
    assert both([1, 0, 0, 1, 1], [2, 3, 1, 4, 0], [0.009, 0.009, 0.0145, 0.0145, 0.0145], 5) == [0, 1, 1, 0, 2]


def test_isolated_vertices_keep_their_own_segment():
    assert both([1, 2], [2, 4], [0, 0], 7) == [0, 1, 1, 2, 1, 3, 4]
    assert both([1, 2], [2, 4], [0, 0], 7, seg_min_verts=20) == [0, 1, 1, 2, 1, 3, 4]


def test_ids_are_numbered_by_the_smallest_member():
    """whatever root the union keeps: 5 joins 2 with 5 named first, 4 joins 0 likewise, 3 stays alone"""
    assert both([5, 4], [2, 0], [0, 0], 6) == [0, 1, 2, 3, 0, 2]
    assert both([4, 5, 2], [0, 2, 1], [0, 0, 0], 6) == [0, 1, 1, 2, 0, 1]


def test_self_loops_change_nothing():
    assert both([0, 1, 1], [0, 1, 2], [0, 0, 0], 3) == [0, 1, 1]


def test_bad_input_is_refused():
    import wsis_native
    with pytest.raises(wsis_native.WsisError):
        merge([0], [3], [0.0], 3)
    with pytest.raises(wsis_native.WsisError):
        merge([-1], [0], [0.0], 3)
    with pytest.raises(wsis_native.WsisError):
        merge([0, 1], [1, 2], [0.5, 0.25], 3)
    with pytest.raises(ValueError):
        merge([0, 1], [1], [0.5], 3)
