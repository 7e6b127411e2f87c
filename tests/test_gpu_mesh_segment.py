"""GPU: the ScanNet mesh superpoints (``wsis_graph_prep.segment_mesh``, csrc/meshseg.hip, ``wsis_host_mesh_merge``;
DESIGN.md 4.17) against tests/mesh_segment_ref.py, the numpy restatement of the definition.

1. the kernels, bit for bit: face normals, vertex normals and (a, b, w) on a stepped noisy heightfield and on meshes
   built around what can go wrong -- a fan vertex of valence 70, a vertex of valence 1, an unused vertex, a zero-area
   face, a face naming a vertex twice, zero-length edges, V around the wave size, F = 0, faces as int32 and int64;
2. the whole function: ids equal to the restatement, a planted right angle, identical bytes from two calls, the type
   of the result following the type of the input;
3. the refusals;
4. ``prepare_scannet_scene``.

No tolerance appears: every comparison is equality of fp32 bits or of integers.  The restatement of a mesh is computed
once and shared."""
import numpy as np
import pytest
import torch

import mesh_segment_ref as ref

pytestmark = pytest.mark.gpu

F32 = np.float32


def gp():
    import wsis_graph_prep
    return wsis_graph_prep


# ---- the meshes --------------------------------------------------------------------------------------------------

def oddities():
    """one mesh with: vertex 0 the centre of a closed fan of 70 faces; vertex 71 in one face only; vertex 72 in none;
    the collinear face (73, 74, 75) of area 0; the face (5, 5, 6) naming a vertex twice (area 0, the edge (5, 5) of length
    0); vertex 76 at the position of vertex 10, so that the edge (76, 10) between two vertices has length 0"""
    rng = np.random.RandomState(11)
    ang = np.arange(70) * (2 * np.pi / 70)
    ring = np.stack([np.cos(ang), np.sin(ang), 0.1 * rng.randn(70)], 1)
    xyz = np.concatenate([[[0.0, 0.0, 0.3]], ring, [[1.5, 0.2, 0.4]], [[9.0, 9.0, 9.0]],
                          [[2.0, 0.0, 0.0], [3.0, 0.0, 0.0], [4.0, 0.0, 0.0]], [ring[9]]]).astype(F32)
    fan = [(0, 1 + i, 1 + (i + 1) % 70) for i in range(70)]
    faces = np.asarray(fan + [(71, 1, 2), (73, 74, 75), (5, 5, 6), (76, 10, 11)], dtype=np.int64)
    return xyz, faces


def strip(V):
    """V random vertices, the faces (i, i + 1, i + 2); a single vertex gets the one face (0, 0, 0)"""
    rng = np.random.RandomState(100 + V)
    xyz = rng.rand(V, 3).astype(F32)
    faces = np.stack([np.arange(V - 2), np.arange(1, V - 1), np.arange(2, V)], 1) if V > 2 else np.zeros((1, 3))
    return xyz, faces.astype(np.int64)


def right_angle(cell=0.05):
    """two flat 15 x 15 patches of 225 vertices each: a floor (columns 0..14 of a 30 x 15 grid) and a wall dropping from
    its last column (columns 15..29), joined by the strip of faces between columns 14 and 15, which lies in the wall's
    plane, less the strip's last cell.  The wall's vertices all have the wall's normal; the floor's last column has
    mixed normals, each vertex a segment of its own after sweep 1, which sweep 2 gives back to the floor."""
    s, t = np.meshgrid(np.arange(30), np.arange(15))
    xyz = (np.stack([np.minimum(s, 14), t, -np.maximum(s - 14, 0)], -1).reshape(-1, 3) * cell).astype(F32)
    faces = ref.grid_faces(30, 15)
    v = 13 * 30 + 14
    last_cell = (faces == [v, v + 1, v + 30]).all(1) | (faces == [v + 1, v + 31, v + 30]).all(1)
    return xyz, faces[~last_cell]


MESHES = {"heightfield": lambda: ref.heightfield(40, seed=3), "oddities": oddities, "no_faces": lambda: strip(5)[:1] +
          (np.zeros((0, 3), np.int64),), "right_angle": right_angle}
MESHES.update({f"strip{V}": (lambda V=V: strip(V)) for V in (1, 63, 64, 65)})
KERNEL_MESHES = ("heightfield", "oddities", "no_faces", "strip1", "strip63", "strip64", "strip65")
_CACHE = {}


def mesh(name):
    """-> (vertices, faces, the restatement's stages); computed once, the stages read-only"""
    if name not in _CACHE:
        xyz, faces = MESHES[name]()
        fn = ref.face_normals(xyz, faces)
        vn = ref.vertex_normals(len(xyz), faces, fn)
        a, b = ref.edges_of_faces(faces)
        want = {"fn": fn, "vn": vn, "a": a, "b": b, "w": ref.edge_weights(xyz, vn, a, b)}
        for arr in want.values():
            arr.setflags(write=False)
        _CACHE[name] = (xyz, faces, want)
    return _CACHE[name]


def ref_ids(name, k_thresh=ref.K_THRESH, seg_min_verts=ref.SEG_MIN_VERTS):
    key = (name, k_thresh, seg_min_verts)
    if key not in _CACHE:
        xyz, faces, want = mesh(name)
        order = ref.sort_edges(want["a"], want["b"], want["w"])
        _CACHE[key] = ref.sweeps(*order, len(xyz), k_thresh, seg_min_verts)[0]
        _CACHE[key].setflags(write=False)
    return _CACHE[key]


def same_bits(got, want, name):
    got = got.cpu().numpy()
    assert got.dtype == want.dtype and got.shape == want.shape, name
    g, w = got.view(np.uint32).reshape(-1), want.view(np.uint32).reshape(-1)
    differ = np.nonzero(g != w)[0]
    print(f"{name}: {len(differ)} of {len(w)} words differ")
    assert len(differ) == 0, f"{name}: first at {differ[:5]}: {got.reshape(-1)[differ[:5]]} != {want.reshape(-1)[differ[:5]]}"


# ---- 1: the kernels --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("index_dtype", (np.int64, np.int32))
@pytest.mark.parametrize("name", KERNEL_MESHES)
def test_normals_and_weights_equal_the_restatement_bit_for_bit(name, index_dtype):
    xyz, faces, want = mesh(name)
    faces = faces.astype(index_dtype)
    fn, vn = gp().mesh_normals(xyz, faces)
    a, b, w, vn2 = gp().mesh_edge_weights(torch.from_numpy(xyz).cuda(), torch.from_numpy(faces).cuda())
    assert fn.is_cuda and vn.is_cuda and a.is_cuda and b.is_cuda and w.is_cuda
    same_bits(fn, want["fn"], "face normals")
    same_bits(vn, want["vn"], "vertex normals")
    same_bits(vn2, want["vn"], "vertex normals (second call)")
    assert a.dtype == torch.int32 and np.array_equal(a.cpu().numpy(), want["a"])
    assert b.dtype == torch.int32 and np.array_equal(b.cpu().numpy(), want["b"])
    same_bits(w, want["w"], "edge weights")


def test_the_oddities_are_what_they_claim():
    """the restatement itself on the mesh of special cases: the cases are there"""
    xyz, faces, want = mesh("oddities")
    valence = np.bincount(faces.reshape(-1), minlength=len(xyz))
    assert valence[0] == 70 and valence[71] == 1 and valence[72] == 0
    assert not want["vn"][72].any() and want["vn"][0].any()
    zero_area = [i for i, n in enumerate(want["fn"]) if not n.any()]
    assert zero_area == [71, 72, 73]                # (76, 10, 11) has two vertices in one place
    assert np.array_equal(xyz[76], xyz[10]) and (want["a"][3 * 73], want["b"][3 * 73]) == (76, 10)
    assert (want["a"][3 * 72], want["b"][3 * 72]) == (5, 5)
    assert np.isfinite(want["w"]).all()


# ---- 2: the whole function -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k_thresh,seg_min_verts", ((ref.K_THRESH, ref.SEG_MIN_VERTS), (0.001, 1)))
def test_ids_equal_the_restatement_on_the_heightfield(k_thresh, seg_min_verts):
    xyz, faces, _ = mesh("heightfield")
    assert len(faces) == 3042
    want = ref_ids("heightfield", k_thresh, seg_min_verts)
    got = gp().segment_mesh(xyz, faces, k_thresh, seg_min_verts)
    print(f"{want.max() + 1} segments")
    assert isinstance(got, np.ndarray) and got.dtype == np.int64 and np.array_equal(got, want)
    assert 1 < want.max() + 1 < len(xyz)


@pytest.mark.parametrize("name", ("oddities", "no_faces", "strip1", "strip65"))
def test_ids_equal_the_restatement_on_the_small_meshes(name):
    xyz, faces, _ = mesh(name)
    got = gp().segment_mesh(xyz, faces.astype(np.int32))
    assert np.array_equal(got, ref_ids(name))
    if name == "no_faces":
        assert np.array_equal(got, np.arange(len(xyz)))


def test_no_vertices():
    got = gp().segment_mesh(np.zeros((0, 3), F32), np.zeros((0, 3), np.int64))
    assert got.dtype == np.int64 and got.shape == (0,)


def test_a_planted_right_angle_gives_its_two_patches():
    """exactly the two patches while segMinVerts <= 225 (from the default on: below it the floor's last column, whose
    normals are mixed, stays apart), one segment when segMinVerts exceeds the vertex count"""
    xyz, faces, _ = mesh("right_angle")
    patches = (np.arange(450) % 30 >= 15).astype(np.int64)
    for seg_min_verts in (ref.SEG_MIN_VERTS, 225):
        got = gp().segment_mesh(xyz, faces, segMinVerts=seg_min_verts)
        assert np.array_equal(got, ref_ids("right_angle", ref.K_THRESH, seg_min_verts))
        assert got.max() + 1 == 2 and np.array_equal(got, patches)
    got = gp().segment_mesh(xyz, faces, segMinVerts=451)
    assert np.array_equal(got, ref_ids("right_angle", ref.K_THRESH, 451)) and not got.any()


def test_two_calls_give_the_same_bytes_and_the_result_follows_the_input_type():
    xyz, faces, _ = mesh("heightfield")
    first = gp().segment_mesh(xyz, faces)
    second = gp().segment_mesh(xyz, faces)
    assert isinstance(first, np.ndarray) and first.tobytes() == second.tobytes()
    t = gp().segment_mesh(torch.from_numpy(xyz).cuda(), torch.from_numpy(faces).cuda())
    assert torch.is_tensor(t) and t.is_cuda and t.dtype == torch.int64 and t.cpu().numpy().tobytes() == first.tobytes()
    stages = [gp().mesh_edge_weights(xyz, faces) for _ in range(2)]
    for x, y in zip(*stages):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()


# ---- 3: the refusals -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("what", ("nan", "inf_in_an_unused_vertex", "index_V", "index_negative", "faces_without_vertices"))
def test_bad_meshes_are_refused(what):
    xyz, faces, _ = mesh("oddities")
    xyz, faces = xyz.copy(), faces.copy()
    if what == "nan":
        xyz[3, 1] = np.nan
    elif what == "inf_in_an_unused_vertex":
        xyz[72, 2] = np.inf
    elif what == "index_V":
        faces[40, 2] = len(xyz)
    elif what == "index_negative":
        faces[0, 0] = -1
    else:
        xyz = xyz[:0]
    for call in (gp().segment_mesh, gp().mesh_edge_weights, gp().mesh_normals):
        with pytest.raises(ValueError):
            call(xyz, faces)


def test_sizes_beyond_int32_are_refused_before_anything_is_allocated():
    one, tri = np.zeros((1, 3), F32), np.zeros((1, 3), np.int64)
    with pytest.raises(ValueError):
        gp().segment_mesh(np.broadcast_to(one, (1 << 31, 3)), tri)
    with pytest.raises(ValueError):
        gp().segment_mesh(one, np.broadcast_to(tri, ((1 << 31) // 3 + 1, 3)))


def test_wrong_types_and_devices_are_refused():
    import wsis_native
    xyz, faces, _ = mesh("strip63")
    with pytest.raises(wsis_native.WsisError):
        gp().segment_mesh(xyz, faces, device="cpu")
    with pytest.raises(wsis_native.WsisError):
        gp().segment_mesh(xyz.astype(np.float64), faces)
    with pytest.raises(wsis_native.WsisError):
        gp().segment_mesh(xyz, faces.astype(np.float32))
    with pytest.raises(ValueError):
        gp().segment_mesh(xyz.reshape(-1), faces)


# ---- 4: the scene --------------------------------------------------------------------------------------------------

def test_prepare_scannet_scene_is_the_reference_s_array_part():
    import wsis_datasets
    xyz, faces, _ = mesh("heightfield")
    rng = np.random.RandomState(9)
    points = np.concatenate([xyz.astype(np.float64), rng.randint(0, 256, (len(xyz), 3)).astype(np.float64)], 1)
    sem = (xyz[:, 0] > 1.0).astype(np.float64)
    ins = np.where(xyz[:, 1] > 1.0, 1.0, -100.0)
    tup, graph = gp().prepare_scannet_scene(points, faces, sem, ins, np.random.RandomState(4), scene="scene0000_00")
    coords, colors, sem_out, ins_out, superpoint, scene = tup
    assert scene == "scene0000_00" and sem_out is sem and ins_out is ins
    assert np.array_equal(superpoint, gp().segment_mesh(xyz, faces)) and np.array_equal(superpoint, ref_ids("heightfield"))
    assert np.array_equal(coords, points[:, :3] - points[:, :3].mean(0)) and coords.flags.c_contiguous
    assert np.array_equal(colors, points[:, 3:6] / 127.5 - 1)
    want = gp().build_graph_scannet(xyz, faces, superpoint, sem, ins, np.random.RandomState(4))
    assert graph.vcount == want.vcount == superpoint.max() + 1
    assert np.array_equal(graph.edges, want.edges) and np.array_equal(graph.is1ins, want.is1ins)
    assert graph.f.tobytes() == want.f.tobytes()
    assert set(graph.vs) == set(want.vs) and all(np.array_equal(graph.vs[k], want.vs[k]) for k in want.vs)
    prep = wsis_datasets.DeviceScenePrep(max_npoint=250000, aug=False, test_mode=True, seed=0, device="cuda")
    resident = prep.upload(tup, graph)
    assert resident.N == len(xyz) and resident.S == graph.vcount
    # no labels: zeros for both, as the reference's test split
    tup0, graph0 = gp().prepare_scannet_scene(points, faces, rng=np.random.RandomState(4))
    assert not tup0[2].any() and not tup0[3].any() and tup0[2].shape == (len(xyz),)
    assert np.array_equal(tup0[4], superpoint) and np.array_equal(graph0.edges, graph.edges)
