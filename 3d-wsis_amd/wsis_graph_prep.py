"""The superpoint graph of a scene, built on the device: what ``data/ScanNetV2/prepare_data_inst_ScanNetV2.py``
(``build_weak_label_graph`` :172-285, ``compute_edges_feature`` :340-433) and ``data/S3DIS/prepare_S3DIS_inst_data.py``
(``build_graph_10NBR`` :101-224, ``compute_edges_feature`` :268-358) of the reference write into ``*_spg.dat``.

    scene = GraphScene(xyz, superpoint)                            once per scene: upload, point CSR of the superpoints
    superpoint_features(scene)                                     centroid, length, surface, volume, count
    superpoint_labels(scene, semantic_labels, instance_labels)     stats.mode per superpoint, offset to the instance centre
    neighbor_lists(centres, k, radius)                             KDTree.query / query_radius, ordered by (d2, id)
    face_edges(faces, superpoint)                                  the mesh-face edges of ScanNet :193-202
    edge_features(scene, features, edges, rng)                     the 13 edge features
    build_graph_s3dis(...) / build_graph_scannet(...)              -> wsis_datasets.PlainGraph
    segment_mesh(vertices, faces)                                  the ScanNet superpoints of a mesh (:77)
    prepare_scannet_scene(points, faces, ...)                      the array part of :64-91 -> (scene tuple, PlainGraph)

Both builders return what ``PlainGraph.from_igraph`` gives for the reference's graph: vertex attributes ``v``,
``semantic_label``, ``instance_label``, ``superpoint_feature``, ``superpoint_offset_vector``, edges in ``sorted(set)``
order, ``f`` and ``is1ins``.  The reference forms one ``np.where(superpoint == spID)`` mask per superpoint and use
(O(S*N)); here the per-point work is one pass per stage over the point CSR (``csrc/graphprep.hip``).

Randomness: the sampling of ``compute_edges_feature`` (:409-412) is drawn on the host from a
``numpy.random.RandomState``, one ``choice(n_big, n_small, replace=False)`` per edge with rows of different length, in
edge order; ``RandomState(seed)`` reproduces the reference after ``np.random.seed(seed)``.

There is no CPU fallback: a CPU device raises ``WsisError``.  Declared differences from the reference:
neighbour order = ascending (d2, id) with self excluded by id; S <= k gives every other superpoint; a superpoint id
without points, non-fp32 ``xyz`` and k > 128 are refused.
"""
import collections

import numpy as np
import torch

import wsis_native as _n
from torch_scatter import segment_csr
from wsis_datasets import PlainGraph

NONE = -100
K_MAX = 128                      # GP_K_MAX of csrc/graphprep.hip
SAMPLE_CHUNK = 1 << 20           # sample indices uploaded per wsis_gp_edge_features call

_SuperpointFeatures = collections.namedtuple("SuperpointFeatures", "centroid length surface volume count cov ev")
SuperpointLabels = collections.namedtuple("SuperpointLabels", "sp_semantic sp_instance sp_offset_vector")
NeighborLists = collections.namedtuple("NeighborLists", "nbr dist2 count")


class SuperpointFeatures(_SuperpointFeatures):
    """device tensors: ``centroid`` fp32 [S,3], ``length`` / ``surface`` / ``volume`` fp32 [S], ``count`` int64 [S], and
    for the tests the fp64 covariance ``cov`` [S,6] = (xx, yy, zz, xy, xz, yz) and eigenvalues ``ev`` [S,3]"""
    __slots__ = ()

    def as_array(self):
        """the reference's ``superpoints_features``: float64 [S,7] (what np.concatenate makes of float32 and uint64)"""
        cols = [self.centroid.double(), self.length.double()[:, None], self.surface.double()[:, None],
                self.volume.double()[:, None], self.count.double()[:, None]]
        return torch.cat(cols, 1).cpu().numpy()


def _cuda_device(device, what):
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _n.WsisError(f"{what} runs on the MI355X (there is no CPU fallback)")
    return dev


def _to_device(a, dev, dtype=None):
    t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
    t = t.to(dev)
    return (t if dtype is None else t.to(dtype)).contiguous()


class GraphScene(object):
    """What the graph stages need of one scene, uploaded once: ``xyz`` fp32 [N,3] (any other dtype is refused: the
    reference's arithmetic on the coordinates is float32 arithmetic), ``superpoint`` int64 [N] with dense ids 0..S-1, and
    the point CSR of the superpoints.  An id without points raises ``WsisError``."""

    def __init__(self, xyz, superpoint, device="cuda"):
        dev = _cuda_device(device, "GraphScene")
        if (xyz.dtype != torch.float32) if torch.is_tensor(xyz) else (np.asarray(xyz).dtype != np.float32):
            raise _n.WsisError(f"GraphScene: xyz must be float32, got {xyz.dtype if hasattr(xyz, 'dtype') else type(xyz)}")
        with torch.cuda.device(dev):
            self.xyz = _to_device(xyz, dev).reshape(-1, 3)
            self.superpoint = _to_device(superpoint, dev, torch.int64).reshape(-1)
            self.N = int(self.superpoint.numel())
            if self.xyz.shape[0] != self.N:
                raise ValueError(f"{self.xyz.shape[0]} points but {self.N} superpoint ids")
            if self.N == 0:
                raise _n.WsisError("GraphScene: a scene without points")
            lo, hi = int(self.superpoint.min()), int(self.superpoint.max())
            if lo < 0:
                raise ValueError("negative superpoint id")
            self.device, self.S = dev, hi + 1
            self.csr = segment_csr(self.superpoint, self.S)
            counts = self.csr.offsets[1:] - self.csr.offsets[:-1]
            n_empty = int((counts == 0).sum())
            if n_empty:
                first = int(torch.nonzero(counts == 0)[0])
                raise _n.WsisError(f"superpoint {first} has no points ({n_empty} such ids of {self.S})")


def superpoint_features(scene):
    """The superpoint half of ``compute_edges_feature`` (ScanNet :359-394): one wave per superpoint"""
    S, dev = scene.S, scene.device
    with torch.cuda.device(dev):
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)      # noqa: E731
        out = SuperpointFeatures(f32(S, 3), f32(S), f32(S), f32(S), torch.empty(S, dtype=torch.int64, device=dev),
                                 torch.empty((S, 6), dtype=torch.float64, device=dev),
                                 torch.empty((S, 3), dtype=torch.float64, device=dev))
        _n.check(_n.hip().wsis_gp_sp_moments(_n.ptr(scene.xyz), _n.ptr(scene.csr.perm), _n.ptr(scene.csr.offsets), scene.N, S,
                                             _n.ptr(out.count), _n.ptr(out.centroid), _n.ptr(out.length), _n.ptr(out.surface),
                                             _n.ptr(out.volume), _n.ptr(out.cov), _n.ptr(out.ev), _n.stream_ptr()),
                 "gp_sp_moments")
    return out


def _label_mode(scene, labels):
    """-> (distinct label values ascending [R], rank of every point int32 [N], mode rank per superpoint int64 [S])"""
    dev = scene.device
    lab = _to_device(labels, dev).reshape(-1)
    if int(lab.numel()) != scene.N:
        raise ValueError(f"{int(lab.numel())} labels for {scene.N} points")
    values, inverse = torch.unique(lab, return_inverse=True)
    rank = inverse.to(torch.int32).contiguous()
    del inverse
    mode = torch.empty(scene.S, dtype=torch.int32, device=dev)
    mode_count = torch.empty(scene.S, dtype=torch.int32, device=dev)
    _n.check(_n.hip().wsis_gp_label_mode(_n.ptr(rank), _n.ptr(scene.csr.perm), _n.ptr(scene.csr.offsets), scene.N, scene.S,
                                         _n.ptr(mode), _n.ptr(mode_count), _n.stream_ptr()), "gp_label_mode")
    return values, rank, mode.long()


def superpoint_labels(scene, semantic_labels, instance_labels, features=None):
    """``stats.mode`` of the two labels per superpoint (the smallest value wins a tie; -100 is a value like any other)
    and ``instance_center[label] - superpoint centre`` (ScanNet :186-189, :238-255): float64 ``sp_semantic`` [S],
    ``sp_instance`` [S], ``sp_offset_vector`` [S,3] (host arrays).  Both label arguments ``None``: -100 / -100 / zeros.
    The instance centres are ``wsis_wl_sp_stats`` over a CSR of the instance ranks."""
    S, dev = scene.S, scene.device
    if semantic_labels is None and instance_labels is None:
        return SuperpointLabels(np.full(S, float(NONE)), np.full(S, float(NONE)), np.zeros((S, 3)))
    if semantic_labels is None or instance_labels is None:
        raise ValueError("give both label arrays or neither")
    with torch.cuda.device(dev):
        if features is None:
            features = superpoint_features(scene)
        sem_values, _, sem_mode = _label_mode(scene, semantic_labels)
        ins_values, ins_rank, ins_mode = _label_mode(scene, instance_labels)
        R = int(ins_values.numel())
        csr = segment_csr(ins_rank.long(), R)
        total = torch.empty((R, 3), dtype=torch.float32, device=dev)
        count = torch.empty(R, dtype=torch.int32, device=dev)
        centre = torch.empty((R, 3), dtype=torch.float32, device=dev)
        _n.check(_n.hip().wsis_wl_sp_stats(_n.ptr(scene.xyz), _n.ptr(csr.perm), _n.ptr(csr.offsets), scene.N, R, _n.ptr(total),
                                           _n.ptr(count), _n.ptr(centre), _n.stream_ptr()), "wl_sp_stats")
        offset = (centre[ins_mode] - features.centroid).double()          # an fp32 difference, as the reference's
        return SuperpointLabels(sem_values[sem_mode].double().cpu().numpy(), ins_values[ins_mode].double().cpu().numpy(),
                                offset.cpu().numpy())


def neighbor_lists(centres, k, radius=float("inf"), device="cuda"):
    """Row s of ``nbr`` int32 [S,k] / ``dist2`` float64 [S,k]: the other superpoints within ``radius`` of s, nearest
    first, ties by id, padded with -1 / inf; ``count`` int32 [S]: how many lie within ``radius`` (may exceed k).
    Device tensors.  ``centres``: fp32 [S,3], numpy or device tensor."""
    k = int(k)
    if not 1 <= k <= K_MAX:
        raise _n.WsisError(f"neighbor_lists: k = {k} outside 1..{K_MAX}")
    dev = centres.device if torch.is_tensor(centres) and centres.is_cuda else _cuda_device(device, "neighbor_lists")
    with torch.cuda.device(dev):
        c = _to_device(centres, dev, torch.float32).reshape(-1, 3)
        S = int(c.shape[0])
        out = NeighborLists(torch.empty((S, k), dtype=torch.int32, device=dev),
                            torch.empty((S, k), dtype=torch.float64, device=dev),
                            torch.empty(S, dtype=torch.int32, device=dev))
        _n.check(_n.hip().wsis_gp_neighbors(_n.ptr(c), S, k, float(radius), _n.ptr(out.nbr), _n.ptr(out.dist2),
                                            _n.ptr(out.count), _n.stream_ptr()), "gp_neighbors")
    return out


def _unique_edges(keys, S):
    """sorted(set(edges)) from the keys a * S + b -> int64 [E,2] (device)"""
    u = torch.unique(keys)
    return torch.stack([torch.div(u, S, rounding_mode="floor"), u % S], 1)


def face_edges(faces, superpoint, device="cuda"):
    """Directed pairs (a, b), (b, a) for every mesh face whose vertices lie in more than one superpoint (ScanNet
    :193-202), each pair once, sorted: int64 [M,2] on the device"""
    dev = superpoint.device if torch.is_tensor(superpoint) and superpoint.is_cuda else _cuda_device(device, "face_edges")
    with torch.cuda.device(dev):
        sp = _to_device(superpoint, dev, torch.int64).reshape(-1)
        fc = _to_device(faces, dev, torch.int64).reshape(-1, 3)
        if int(fc.numel()) == 0:
            return torch.empty((0, 2), dtype=torch.int64, device=dev)
        if int(sp.numel()) == 0:
            raise ValueError("faces but no points")
        f_lo, f_hi, s_lo, s_hi = torch.stack([fc.min(), fc.max(), sp.min(), sp.max()]).tolist()      # one read-back
        if f_lo < 0 or f_hi >= int(sp.numel()):
            raise ValueError(f"face vertex index outside [0, {int(sp.numel())})")
        if s_lo < 0:
            raise ValueError("negative superpoint id")
        S = s_hi + 1
        ids = sp[fc]
        a = torch.cat([ids[:, 0], ids[:, 0], ids[:, 1]])
        b = torch.cat([ids[:, 1], ids[:, 2], ids[:, 2]])
        keep = a != b
        a, b = a[keep], b[keep]
        return _unique_edges(torch.cat([a * S + b, b * S + a]), S)


def _symmetric_edges(s, t, S, more=None):
    keys = torch.cat([s * S + t, t * S + s] + ([] if more is None else [more[:, 0] * S + more[:, 1]]))
    return _unique_edges(keys, S)


def draw_samples(counts, edges, rng):
    """The draws of :409-412 in edge order -> (offsets int64 [E+1], indices int32): for an edge whose rows differ in
    length, ``rng.choice(n_big, n_small, replace=False)``; no draw and an empty list otherwise"""
    counts = np.asarray(counts, dtype=np.int64)
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    ns, nt = counts[edges[:, 0]], counts[edges[:, 1]]
    size = np.where(ns != nt, np.minimum(ns, nt), 0)
    off = np.zeros(len(edges) + 1, dtype=np.int64)
    np.cumsum(size, out=off[1:])
    idx = np.empty(int(off[-1]), dtype=np.int32)
    big = np.maximum(ns, nt)
    for e in np.nonzero(size)[0]:
        idx[off[e]:off[e + 1]] = rng.choice(int(big[e]), int(size[e]), replace=False)
    return off, idx


def edge_features(scene, features, edges, rng, samples=None):
    """The edge half of ``compute_edges_feature`` (ScanNet :398-426) -> fp32 [E,13] on the device, columns ``delta_mean``
    3, ``delta_std`` 3, ``delta_centroid`` 3, length / surface / volume / point-count ratios.  ``edges``: [E,2] in the
    order the draws are made (the builders pass ``sorted(set)`` order).  ``samples``: the ``(offsets, indices)`` of
    ``draw_samples`` if they were drawn elsewhere (then ``rng`` is not used)."""
    dev, S = scene.device, scene.S
    with torch.cuda.device(dev):
        edges_h = (edges.cpu().numpy() if torch.is_tensor(edges) else np.asarray(edges)).astype(np.int64).reshape(-1, 2)
        E = len(edges_h)
        if E and (edges_h.min() < 0 or edges_h.max() >= S):
            raise ValueError("edge endpoint outside the graph")
        counts_h = features.count.cpu().numpy()
        off, idx = draw_samples(counts_h, edges_h, rng) if samples is None else samples
        off, idx = np.asarray(off, dtype=np.int64), np.asarray(idx, dtype=np.int32)
        ns, nt = counts_h[edges_h[:, 0]], counts_h[edges_h[:, 1]]
        if len(off) != E + 1 or not np.array_equal(np.diff(off), np.where(ns != nt, np.minimum(ns, nt), 0)):
            raise ValueError("sample lists do not match the edges")
        if len(idx) != off[-1] or (len(idx) and (idx.min() < 0 or (idx >= np.repeat(np.maximum(ns, nt), np.diff(off))).any())):
            raise ValueError("sample index outside its row")
        out = torch.empty((E, 13), dtype=torch.float32, device=dev)
        edges_d = torch.from_numpy(edges_h).to(dev)
        e0 = 0
        while e0 < E:                  # bounded uploads: at most SAMPLE_CHUNK indices (or one edge) per call
            e1 = int(np.searchsorted(off, off[e0] + SAMPLE_CHUNK, side="right")) - 1
            e1 = min(max(e1, e0 + 1), E)
            off_d = torch.from_numpy(off[e0:e1 + 1] - off[e0]).to(dev)
            idx_d = torch.from_numpy(idx[off[e0]:off[e1]]).to(dev) if off[e1] > off[e0] else None
            _n.check(_n.hip().wsis_gp_edge_features(
                _n.ptr(scene.xyz), _n.ptr(scene.csr.perm), _n.ptr(scene.csr.offsets), scene.N, S, _n.ptr(edges_d[e0:]),
                e1 - e0, _n.ptr(off_d), _n.ptr(idx_d), _n.ptr(features.centroid), _n.ptr(features.length),
                _n.ptr(features.surface), _n.ptr(features.volume), _n.ptr(out[e0:]), _n.stream_ptr()), "gp_edge_features")
            e0 = e1
        return out


def standardize_features(f):
    """``StandardScaler().fit(f)`` and ``transform(f, copy=False)`` on fp32 [E,13]: fp64 column mean and population
    variance, zero variance -> scale 1, ``(float64(x) - mean)`` rounded to fp32, then divided by the scale in fp64 and
    rounded again, as the in-place transform does"""
    if int(f.shape[0]) == 0:
        return f
    d = f.double()
    mean = d.mean(0)
    var = (d - mean).square().mean(0)
    scale = torch.where(var == 0, torch.ones_like(var), var.sqrt())
    return ((d - mean).float().double() / scale).float()


def cap_rule_edges(nbr, count, start_edges, cap=5):
    """The sequential edge loop of ScanNet :217-225 on the candidate lists (host arrays): for s ascending, up to ``cap``
    candidates of ``nbr[s]`` (in order) that are not yet edges become edges in both directions; an edge added from s
    does not count towards t's ``cap``.  ``start_edges``: [M,2], the directed edges that exist before (the face edges).
    -> int64 [P,2], the picks (s, t) in the order they were made, or ``None`` if some list ran out before ``cap`` picks
    while ``count[s]`` says more candidates exist than the list holds (call again with a larger k)."""
    nbr, count = np.asarray(nbr), np.asarray(count)
    k = nbr.shape[1] if nbr.ndim == 2 else 0
    edges = set(map(tuple, np.asarray(start_edges, dtype=np.int64).reshape(-1, 2).tolist()))
    picks = []
    for s in range(len(nbr)):
        cnt = 0
        for t in nbr[s].tolist():
            if cnt >= cap or t < 0:
                break
            if (s, t) not in edges:
                edges.add((s, t))
                edges.add((t, s))
                picks.append((s, t))
                cnt += 1
        if cnt < cap and count[s] > k:
            return None
    return np.asarray(picks, dtype=np.int64).reshape(-1, 2)


def _graph(S, labels, features, edges, f, is1ins):
    return PlainGraph({"v": np.arange(S), "semantic_label": labels.sp_semantic, "instance_label": labels.sp_instance,
                       "superpoint_feature": features.as_array(), "superpoint_offset_vector": labels.sp_offset_vector},
                      edges.cpu().numpy(), f.cpu().numpy(), is1ins)


def build_graph_s3dis(xyz, superpoint, semantic_labels, instance_labels, rng, k=10, device="cuda"):
    """``build_graph_10NBR`` (S3DIS :101-224): the k nearest superpoint centres of every superpoint, both directions;
    ``is1ins`` = the two instance labels equal, or the two semantic labels where both instances are -100 (:191-200);
    features not standardised.  -> PlainGraph"""
    scene = GraphScene(xyz, superpoint, device)
    S, dev = scene.S, scene.device
    with torch.cuda.device(dev):
        feats = superpoint_features(scene)
        labels = superpoint_labels(scene, semantic_labels, instance_labels, feats)
        nl = neighbor_lists(feats.centroid, k)
        s = torch.arange(S, device=dev)[:, None].expand(S, int(k))
        ok = nl.nbr >= 0
        edges = _symmetric_edges(s[ok], nl.nbr[ok].long(), S)
        f = edge_features(scene, feats, edges, rng)
        eh = edges.cpu().numpy()
        si, ti = labels.sp_instance[eh[:, 0]], labels.sp_instance[eh[:, 1]]
        ss, ts = labels.sp_semantic[eh[:, 0]], labels.sp_semantic[eh[:, 1]]
        is1ins = np.where((si == NONE) & (ti == NONE), ss == ts, si == ti)
        return _graph(S, labels, feats, edges, f, is1ins)


def build_graph_scannet(xyz, faces, superpoint, semantic_labels=None, instance_labels=None, rng=None, radius=0.3, cap=5,
                        standardize=True, device="cuda"):
    """``build_weak_label_graph`` (ScanNet :172-285): mesh-face edges, then for s ascending up to ``cap`` new edges to
    the nearest centres within ``radius`` (the sequential rule of :217-225, on the host over the candidate lists);
    ``is1ins`` = 0 if either instance label is -100, -1 if they are equal, 1 otherwise (:273-282); features
    standardised.  ``rng=None`` draws from numpy's global stream, as the reference does.  -> PlainGraph"""
    if rng is None:
        rng = np.random.mtrand._rand
    scene = GraphScene(xyz, superpoint, device)
    S, dev = scene.S, scene.device
    with torch.cuda.device(dev):
        feats = superpoint_features(scene)
        labels = superpoint_labels(scene, semantic_labels, instance_labels, feats)
        fe = face_edges(faces, scene.superpoint)
        fe_h = fe.cpu().numpy()
        k, picks = 16, None
        while picks is None:
            if k > K_MAX:
                raise _n.WsisError(f"build_graph_scannet: a superpoint needs more than {K_MAX} candidates within {radius}")
            nl = neighbor_lists(feats.centroid, k, radius)
            picks = cap_rule_edges(nl.nbr.cpu().numpy(), nl.count.cpu().numpy(), fe_h, cap)
            k *= 2
        picks = torch.from_numpy(picks).to(dev)
        edges = _symmetric_edges(picks[:, 0], picks[:, 1], S, more=fe)
        eh = edges.cpu().numpy()
        f = edge_features(scene, feats, edges, rng)
        if standardize:
            f = standardize_features(f)
        si, ti = labels.sp_instance[eh[:, 0]], labels.sp_instance[eh[:, 1]]
        is1ins = np.where((si == NONE) | (ti == NONE), 0, np.where(si == ti, -1, 1))
        return _graph(S, labels, feats, edges, f, is1ins)


# ---- ScanNet mesh superpoints: segmentator.segment_mesh (prepare_data_inst_ScanNetV2.py:77, :157) --------------------

MESH_K_THRESH = 0.01             # kThresh and segMinVerts of the ScanNet Segmentator
MESH_SEG_MIN_VERTS = 20


def _mesh_stage(vertices, faces, device, what, mark=None):
    """Steps 1-4 of DESIGN.md 4.17 -> (a, b, w, vertex_normals, face_normals, err), device tensors.  ``err`` int32 [2] =
    (face indices outside [0, V), non-finite coordinates) is not read here: with either count non-zero the rest means
    nothing (``_mesh_refuse``).  ``mark(stage)``, if given, is called behind the launches of a stage."""
    dev = vertices.device if torch.is_tensor(vertices) and vertices.is_cuda else _cuda_device(device, what)
    if not torch.is_tensor(vertices):
        vertices = np.asarray(vertices)
    if not torch.is_tensor(faces):
        faces = np.asarray(faces)
    if len(vertices.shape) != 2 or vertices.shape[1] != 3 or len(faces.shape) != 2 or faces.shape[1] != 3:
        raise ValueError(f"{what}: vertices [V,3] and faces [F,3], got {tuple(vertices.shape)} and {tuple(faces.shape)}")
    V, F = int(vertices.shape[0]), int(faces.shape[0])
    if V >= 1 << 31 or 3 * F >= 1 << 31:
        raise ValueError(f"{what}: {V} vertices / {3 * F} face edges do not fit int32")
    if vertices.dtype not in (torch.float32, np.dtype(np.float32)):
        raise _n.WsisError(f"{what}: vertices must be float32, got {vertices.dtype}")
    if faces.dtype not in (torch.int32, torch.int64, np.dtype(np.int32), np.dtype(np.int64)):
        raise _n.WsisError(f"{what}: faces must be int32 or int64, got {faces.dtype}")
    if F and not V:
        raise ValueError(f"{what}: face vertex index outside [0, 0)")
    with torch.cuda.device(dev):
        xyz, fc = _to_device(vertices, dev), _to_device(faces, dev, torch.int64)
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)      # noqa: E731
        i32 = lambda n: torch.empty(n, dtype=torch.int32, device=dev)                 # noqa: E731
        fn, vn, a, b, w, err = f32(F, 3), f32(V, 3), i32(3 * F), i32(3 * F), f32(3 * F), i32(2)
        keys = torch.empty(3 * F, dtype=torch.int64, device=dev)
        lib, st = _n.hip(), _n.stream_ptr()
        _n.check(lib.wsis_mesh_face_normals(_n.ptr(xyz), V, _n.ptr(fc), F, _n.ptr(fn), _n.ptr(keys), _n.ptr(err), st),
                 "mesh_face_normals")
        csr = segment_csr(keys, V)                     # stable: a vertex's row lists its face slots ascending
        _n.check(lib.wsis_mesh_vertex_normals(_n.ptr(fn), _n.ptr(csr.perm), _n.ptr(csr.offsets), V, F, _n.ptr(vn), st),
                 "mesh_vertex_normals")
        if mark is not None:
            mark("normals")
        _n.check(lib.wsis_mesh_edge_weights(_n.ptr(xyz), _n.ptr(vn), V, _n.ptr(fc), F, _n.ptr(a), _n.ptr(b), _n.ptr(w), st),
                 "mesh_edge_weights")
        if mark is not None:
            mark("weights")
    return a, b, w, vn, fn, err


def _mesh_refuse(err, what):
    n_index, n_nonfinite = int(err[0]), int(err[1])
    if n_index:
        raise ValueError(f"{what}: {n_index} face vertex indices outside the vertices")
    if n_nonfinite:
        raise ValueError(f"{what}: {n_nonfinite} vertices with a non-finite coordinate")


def mesh_normals(vertices, faces, device="cuda"):
    """Steps 1-2 of ``segment_mesh`` on their own -> (face_normals fp32 [F,3], vertex_normals fp32 [V,3]), device tensors"""
    _, _, _, vn, fn, err = _mesh_stage(vertices, faces, device, "mesh_normals")
    _mesh_refuse(err.tolist(), "mesh_normals")
    return fn, vn


def mesh_edge_weights(vertices, faces, device="cuda"):
    """Steps 1-4 of ``segment_mesh`` on their own -> (a int32 [3F], b int32 [3F], w fp32 [3F], vertex_normals fp32 [V,3]),
    device tensors, the edges in face order (unsorted)"""
    a, b, w, vn, _, err = _mesh_stage(vertices, faces, device, "mesh_edge_weights")
    _mesh_refuse(err.tolist(), "mesh_edge_weights")
    return a, b, w, vn


def mesh_merge(a, b, w, n_vertices, kThresh=MESH_K_THRESH, segMinVerts=MESH_SEG_MIN_VERTS):
    """Steps 6-8 of ``segment_mesh`` on the host (``wsis_host_mesh_merge``; no device is touched): the two sweeps over
    edges already sorted by (w, edge index) -> (ids int64 [n_vertices], number of segments)"""
    import ctypes
    a, b = np.ascontiguousarray(a, dtype=np.int32).reshape(-1), np.ascontiguousarray(b, dtype=np.int32).reshape(-1)
    w = np.ascontiguousarray(w, dtype=np.float32).reshape(-1)
    if not len(a) == len(b) == len(w):
        raise ValueError(f"{len(a)} / {len(b)} edge ends for {len(w)} weights")
    ids, n_seg = np.empty(int(n_vertices), np.int64), ctypes.c_int64(0)
    _n.check_host(_n.host().wsis_host_mesh_merge(a.ctypes.data, b.ctypes.data, w.ctypes.data, len(w), int(n_vertices),
                                                 float(kThresh), int(segMinVerts), ids.ctypes.data, ctypes.byref(n_seg)),
                  "mesh_merge")
    return ids, int(n_seg.value)


def segment_mesh(vertices, faces, kThresh=MESH_K_THRESH, segMinVerts=MESH_SEG_MIN_VERTS, device="cuda", _mark=None):
    """``segmentator.segment_mesh(vertices, faces)`` (ScanNet :77, :157; [UPSTREAM], restated in DESIGN.md 4.17 -- parity
    with the external binary is not pinned): Felzenszwalb-Huttenlocher segmentation of the mesh edges weighted by the
    difference of the vertex normals.  ``vertices`` fp32 [V,3], ``faces`` int32 / int64 [F,3] -> int64 [V], dense ids
    numbered by each segment's smallest vertex.  numpy in: numpy out; tensors in: a device tensor out.

    Normals and weights are kernels (csrc/meshseg.hip), the stable sort is torch's, the two sweeps are a serial
    recurrence and run on the host: one read-back of the sorted (a, b, w) with the error word, one upload of the ids.
    Non-finite coordinates, a face index outside [0, V), V >= 2^31 or 3 F >= 2^31 raise ``ValueError``; there is no CPU
    fallback.  ``_mark(stage)`` is called behind every stage (tools/mesh_segment_bench.py times them with it)."""
    as_tensor = torch.is_tensor(vertices)
    mark = _mark if _mark is not None else (lambda stage: None)
    a, b, w, _, _, err = _mesh_stage(vertices, faces, device, "segment_mesh", _mark)
    dev, E = w.device, int(w.numel())
    V = int(vertices.shape[0])
    with torch.cuda.device(dev):
        w_sorted, order = torch.sort(w, stable=True)
        packed = torch.cat([a[order], b[order], w_sorted.view(torch.int32), err])
        mark("sort")
        host = packed.cpu().numpy()                                      # the read-back: 12 bytes per edge + the error word
        mark("read_back")
        _mesh_refuse(host[3 * E:], "segment_mesh")
        ids, _ = mesh_merge(host[:E], host[E:2 * E], host[2 * E:3 * E].view(np.float32), V, kThresh, segMinVerts)
        mark("host_sweeps")
        if as_tensor:
            ids = torch.from_numpy(ids).to(dev)
            mark("upload")
    return ids


def prepare_scannet_scene(points, faces, semantic_labels=None, instance_labels=None, rng=None, device="cuda", scene=""):
    """The array part of ``f`` / ``f_test`` (ScanNet :64-91, :107-166) from a mesh already read: ``points`` [V,6] = xyz and
    rgb in 0..255, ``faces`` [F,3].  ``coords`` = xyz - mean, ``colors`` = rgb / 127.5 - 1, ``superpoint`` =
    ``segment_mesh(float32(xyz), faces)``, and the graph of ``build_graph_scannet`` on the uncentred xyz (as float32),
    the reference passing ``points[:, :3]``.  No labels: zeros for both, as ``f_test`` sets them (:79-80).
    -> ((coords, colors, semantic_labels, instance_labels, superpoint, scene), PlainGraph), what ``ScenePrep`` /
    ``DeviceScenePrep.upload`` take.  Reading the PLY is the caller's."""
    points = np.asarray(points)
    if points.ndim != 2 or points.shape[1] < 6:
        raise ValueError(f"points [V,6] = xyz + rgb, got {points.shape}")
    faces = np.ascontiguousarray(faces)
    if (semantic_labels is None) != (instance_labels is None):
        raise ValueError("give both label arrays or neither")
    if semantic_labels is None:
        semantic_labels, instance_labels = np.zeros(points.shape[0]), np.zeros(points.shape[0])
    coords = np.ascontiguousarray(points[:, :3] - points[:, :3].mean(0))
    colors = np.ascontiguousarray(points[:, 3:6]) / 127.5 - 1
    xyz = np.ascontiguousarray(points[:, :3], dtype=np.float32)
    superpoint = segment_mesh(xyz, faces, device=device)
    graph = build_graph_scannet(xyz, faces, superpoint, semantic_labels, instance_labels, rng, device=device)
    return (coords, colors, semantic_labels, instance_labels, superpoint, scene), graph
