"""The S3DIS partition front end on the device: what ``generate_SPG_superpoint`` of the reference's
``data/S3DIS/partition/partition_S3DIS.py`` (:81-115) computes per room before and after the l0 cut-pursuit solver.

    prune(xyz, voxel_width, rgb, labels, n_labels)     libply_c.prune        ply_c/ply_c.cpp:293-392
    knn(xyz, k)                                        compute_graph_nn_2    graphs.py:26-83 (sklearn kd-tree)
    geometric_features(xyz, nbr)                       libply_c.compute_geof ply_c/ply_c.cpp:396-474 (Eigen)
    partition_inputs(xyz, rgb)                         :95-108, the argument list of libcp.cutpursuit
    cut_pursuit(features, source, target, w, lambda)   libcp.cutpursuit      cut-pursuit/src/cutpursuit.cpp:77-105
    generate_superpoints(xyz, rgb)                     :81-115, -> point-level superpoint ids

``cut_pursuit`` is the l0 cut-pursuit solver with L2 fidelity at the reference's "speed 4" settings, on the device
(``csrc/cutpursuit.hip``), and the default solver of ``generate_superpoints``; any callable with the
signature of ``libcp.cutpursuit`` can take its place: ``PartitionInputs.solver_args`` is exactly what that takes, in its
dtypes, and ``PartitionInputs.to_points`` is the back-projection of :113.  Its declared differences from ``libcp``: a
random stream of its own (a hash, not ``rand()``), capacities quantised to integers, the sink side is the set of nodes
the sink can be reached from (Boykov-Kolmogorov reports its search trees), component ids in order of smallest node, fp64
sums, energies from the component ids alone, no capacities left in saturated components -- partitions are not comparable
node for node.  ``cutoff``, ``spatial`` and ``weight_decay`` other than the reference's S3DIS values are refused.

Device tensors in and out (numpy input is uploaded); kernels in ``csrc/partition.hip``.  There is no
CPU fallback: a CPU device raises ``WsisError``.  Declared differences from the reference: neighbour
lists ascend in (d2, id) with self excluded by id (sklearn leaves ties open and drops position 0); the geometric
features are evaluated in fp64 and rounded once (the reference: fp32 through Eigen); ``mean_distance`` is an fp64 sum
rounded once (numpy: a pairwise fp32 sum); a neighbourhood whose largest eigenvalue is 0 gives NaN, as the
reference's expressions do.  Refused: non-fp32 ``xyz``, non-uint8 ``rgb``, no points, non-finite coordinates, k > 64,
fewer than k + 1 points, ``k_nn_adj > k_nn_geof``, a label above ``n_labels``.
"""
import collections

import numpy as np
import torch

import wsis_native as _n
from torch_scatter import segment_csr

K_MAX = 64                       # PT_K_MAX of csrc/partition.hip
CELL_VOXELS = 3.0                # k-NN cell edge of pruned input, in voxel widths

Pruned = collections.namedtuple("Pruned", "xyz rgb label_hist p2v count")
Knn = collections.namedtuple("Knn", "nbr dist2")
Geof = collections.namedtuple("Geof", "geof cov ev")
_PartitionInputs = collections.namedtuple(
    "PartitionInputs", "features source target edge_weight distances mean_distance target_geof p2v xyz rgb")


class PartitionInputs(_PartitionInputs):
    """device tensors over the V voxels of a room and their V * k_nn_adj edges: ``features`` fp32 [V,7], ``source`` /
    ``target`` int32 [E] (non-negative: read as uint32), ``edge_weight`` / ``distances`` fp32 [E], ``mean_distance`` fp32
    [1], ``target_geof`` int32 [V, k_nn_geof], ``p2v`` int32 [N], the pruned ``xyz`` fp32 [V,3] and ``rgb`` uint8 [V,3]"""
    __slots__ = ()

    def solver_args(self, reg_strength=0.03):
        """the numpy tuple ``libcp.cutpursuit(features, source, target, edge_weight, reg_strength)`` takes (:110-111)"""
        return (self.features.cpu().numpy(), self.source.cpu().numpy().view(np.uint32),
                self.target.cpu().numpy().view(np.uint32), self.edge_weight.cpu().numpy(), reg_strength)

    def to_points(self, in_component):
        """``in_component[p2v_map]`` (:113): voxel-level ids -> point-level ids, in the type given (numpy or tensor)"""
        if torch.is_tensor(in_component):
            if int(in_component.shape[0]) != int(self.xyz.shape[0]):
                raise ValueError(f"{int(in_component.shape[0])} ids for {int(self.xyz.shape[0])} voxels")
            return in_component.to(self.p2v.device)[self.p2v.long()]
        ids = np.asarray(in_component)
        if ids.shape[0] != int(self.xyz.shape[0]):
            raise ValueError(f"{ids.shape[0]} ids for {int(self.xyz.shape[0])} voxels")
        return ids[self.p2v.cpu().numpy()]


def _dtype_of(a):
    return a.dtype if hasattr(a, "dtype") else np.asarray(a).dtype


def _device_of(a, device, what):
    dev = a.device if torch.is_tensor(a) and a.is_cuda else torch.device(device)
    if dev.type != "cuda":
        raise _n.WsisError(f"{what} runs on the MI355X (there is no CPU fallback)")
    return dev


def _upload(a, dev):
    t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
    return t.to(dev).contiguous()


def _check_cloud(xyz, what, rgb=None):
    """the refusals that need no device: dtypes and an empty cloud -> the number of points"""
    if _dtype_of(xyz) not in (torch.float32, np.float32):
        raise _n.WsisError(f"{what}: xyz must be float32, got {_dtype_of(xyz)}")
    if rgb is not None and _dtype_of(rgb) not in (torch.uint8, np.uint8):
        raise _n.WsisError(f"{what}: rgb must be uint8, got {_dtype_of(rgb)}")
    for name, a in (("xyz", xyz), ("rgb", rgb)):
        if a is not None and (len(a.shape) != 2 or int(a.shape[1]) != 3):
            raise _n.WsisError(f"{what}: {name} must have shape [N,3], got {tuple(a.shape)}")
    n = int(xyz.shape[0])
    if n == 0:
        raise _n.WsisError(f"{what}: a cloud without points")
    return n


def _xyz(xyz, dev):
    return _upload(xyz, dev).reshape(-1, 3)


def _rgb(rgb, dev, n):
    t = _upload(rgb, dev).reshape(-1, 3)
    if int(t.shape[0]) != n:
        raise ValueError(f"{int(t.shape[0])} colours for {n} points")
    return t


def prune(xyz, voxel_width, rgb, labels=None, n_labels=0, device="cuda"):
    """``libply_c.prune`` (ply_c.cpp:293-392): the voxel-grid subsample of a room.  -> ``Pruned``: ``xyz`` fp32 [V,3]
    (sequential fp32 sums in point order over the count), ``rgb`` uint8 [V,3] (truncated means), ``label_hist`` int32
    [V, n_labels + 1] (``None`` without ``labels``; non-negative: read as uint32), ``p2v`` int32 [N] (voxel ids in order
    of first occurrence) and ``count`` int32 [V]."""
    _check_cloud(xyz, "prune", rgb)
    dev = _device_of(xyz, device, "prune")
    voxel_width = float(np.float32(voxel_width))
    if not (voxel_width > 0 and np.isfinite(voxel_width)):
        raise _n.WsisError(f"prune: voxel width {voxel_width}")
    with torch.cuda.device(dev):
        x = _xyz(xyz, dev)
        N = int(x.shape[0])
        c = _rgb(rgb, dev, N)
        lab, n_labels = None, int(n_labels)
        if labels is not None:
            lab = _upload(labels, dev).reshape(-1)
            if lab.dtype.is_floating_point or lab.dtype == torch.bool:
                raise _n.WsisError(f"prune: labels must be integers, got {lab.dtype}")
            if int(lab.numel()) != N:
                raise ValueError(f"{int(lab.numel())} labels for {N} points")
            lab = lab.to(torch.int32).contiguous()
            lo, hi = int(lab.min()), int(lab.max())
            if lo < 0 or hi > n_labels:
                raise _n.WsisError(f"prune: labels span {lo}..{hi}, outside 0..{n_labels}")
        lib, st = _n.hip(), _n.stream_ptr()
        coords = torch.empty((N, 4), dtype=torch.int64, device=dev)
        min3 = torch.empty(3, dtype=torch.float32, device=dev)
        flag = torch.empty(1, dtype=torch.int32, device=dev)
        ws_bytes = lib.wsis_pt_bins_workspace_bytes(N)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        _n.check(lib.wsis_pt_bins(_n.ptr(x), N, voxel_width, _n.ptr(coords), _n.ptr(min3), _n.ptr(flag), _n.ptr(ws), ws_bytes,
                                  st), "pt_bins")
        ws_bytes = lib.wsis_voxelize_idx_workspace_bytes(N)
        if ws_bytes < 0:
            raise _n.WsisError("voxelize_idx workspace query failed")
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        p2v = torch.empty(N, dtype=torch.int32, device=dev)
        counts2 = torch.zeros(2, dtype=torch.int32, device=dev)
        _n.check(lib.wsis_voxelize_idx_map(_n.ptr(coords), N, _n.ptr(p2v), _n.ptr(counts2), _n.ptr(ws), ws_bytes, st),
                 "voxelize_idx_map")
        bad, V = int(flag), int(counts2[0])          # the read-back: the refusal and the number of voxels
        if bad:
            raise _n.WsisError("prune: a coordinate is NaN or infinite")
        del coords, ws
        csr = segment_csr(p2v.long(), V)
        out = Pruned(torch.empty((V, 3), dtype=torch.float32, device=dev), torch.empty((V, 3), dtype=torch.uint8, device=dev),
                     None if lab is None else torch.empty((V, n_labels + 1), dtype=torch.int32, device=dev), p2v,
                     torch.empty(V, dtype=torch.int32, device=dev))
        _n.check(lib.wsis_pt_prune_accumulate(_n.ptr(x), _n.ptr(c), _n.ptr(lab), n_labels, _n.ptr(csr.perm),
                                              _n.ptr(csr.offsets), N, V, _n.ptr(out.xyz), _n.ptr(out.rgb),
                                              _n.ptr(out.label_hist), _n.ptr(out.count), st), "pt_prune_accumulate")
    return out


def knn(xyz, k, cell=0.0, stats=False, device="cuda"):
    """``NearestNeighbors(k + 1, 'kd_tree').kneighbors(xyz)[:, 1:]`` (graphs.py:34-38), exact: ``nbr`` int32 [V,k] and
    ``dist2`` float64 [V,k] (squared), every row ascending in (d2, id), self excluded by id.  ``cell``: the edge of the
    search grid's cells (0: chosen from the bounding box and V); it changes the time, never the result.  ``stats=True``
    also returns int32 [V,2]: candidates evaluated per query, 1 where the query scanned every point.

    Cost: a query visits the cells within 3 rings of its own (7 x 7 x 7) and, if its k neighbours are not settled by
    then, scans all V points instead -- V / 64 batches for that query.  That is meant for isolated points.  A ``cell``
    far below the point spacing (fewer than about k / 343 points per cell), or a cloud whose density varies by orders of
    magnitude under the automatic edge, sends many queries there and the call becomes O(V^2 / 64): still exact, but slow.
    ``stats=True`` shows the share; for pruned clouds use about 3 voxel widths, as ``partition_inputs`` does."""
    k = int(k)
    if not 1 <= k <= K_MAX:
        raise _n.WsisError(f"knn: k = {k} outside 1..{K_MAX}")
    V = _check_cloud(xyz, "knn")
    if V < k + 1:
        raise _n.WsisError(f"knn: {V} points have no {k} neighbours each")
    dev = _device_of(xyz, device, "knn")
    with torch.cuda.device(dev):
        x = _xyz(xyz, dev)
        if not bool(torch.isfinite(x).all()):
            raise _n.WsisError("knn: a coordinate is NaN or infinite")
        lib = _n.hip()
        ws_bytes = lib.wsis_pt_knn_workspace_bytes(V)
        if ws_bytes < 0:
            raise _n.WsisError("pt_knn workspace query failed")
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        out = Knn(torch.empty((V, k), dtype=torch.int32, device=dev), torch.empty((V, k), dtype=torch.float64, device=dev))
        st = torch.empty((V, 2), dtype=torch.int32, device=dev) if stats else None
        _n.check(lib.wsis_pt_knn(_n.ptr(x), V, k, float(cell), _n.ptr(out.nbr), _n.ptr(out.dist2), _n.ptr(st), _n.ptr(ws),
                                 ws_bytes, _n.stream_ptr()), "pt_knn")
    return (out, st) if stats else out


def geometric_features(xyz, nbr, device="cuda"):
    """``libply_c.compute_geof`` (ply_c.cpp:396-474) in fp64 -> ``Geof``: ``geof`` fp32 [V,4] = linearity, planarity,
    scattering, verticality; for the tests the fp64 covariance ``cov`` [V,6] = (xx, yy, zz, xy, xz, yz) of the k + 1
    positions and its eigenvalues ``ev`` [V,3], descending, clamped at 0.  ``nbr``: int32 [V,k] (``Knn.nbr``)."""
    _check_cloud(xyz, "geometric_features")
    dev = _device_of(xyz, device, "geometric_features")
    with torch.cuda.device(dev):
        x = _xyz(xyz, dev)
        V = int(x.shape[0])
        nb = _upload(nbr, dev).to(torch.int32).reshape(V, -1).contiguous()
        k = int(nb.shape[1])
        if not 1 <= k <= K_MAX:
            raise _n.WsisError(f"geometric_features: k = {k} outside 1..{K_MAX}")
        out = Geof(torch.empty((V, 4), dtype=torch.float32, device=dev), torch.empty((V, 6), dtype=torch.float64, device=dev),
                   torch.empty((V, 3), dtype=torch.float64, device=dev))
        _n.check(_n.hip().wsis_pt_geof(_n.ptr(x), _n.ptr(nb), V, k, _n.ptr(out.geof), _n.ptr(out.cov), _n.ptr(out.ev),
                                       _n.stream_ptr()), "pt_geof")
    return out


def edge_features(geof, rgb, nn, k_nn_adj, lambda_edge_weight=1.):
    """partition_S3DIS.py:105-108 and graphs.py:69-74 from device tensors -> (features fp32 [V,7], source int32 [E],
    target int32 [E], distances fp32 [E], edge_weight fp32 [E], mean_distance fp32 [1]), E = V * k_nn_adj"""
    _n.require_cuda(geof, rgb, nn.nbr, nn.dist2)
    dev = geof.device
    V, k, ka = int(geof.shape[0]), int(nn.nbr.shape[1]), int(k_nn_adj)
    if not 1 <= ka <= k:
        raise _n.WsisError(f"edge_features: k_nn_adj = {ka} outside 1..{k}")
    with torch.cuda.device(dev):
        lib = _n.hip()
        ws_bytes = lib.wsis_pt_edge_features_workspace_bytes(V, ka)
        if ws_bytes < 0:
            raise _n.WsisError("pt_edge_features workspace query failed")
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)      # noqa: E731
        i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)        # noqa: E731
        features, source, target, distances, weight, mean = f32(V, 7), i32(V * ka), i32(V * ka), f32(V * ka), f32(V * ka), f32(1)
        _n.check(lib.wsis_pt_edge_features(_n.ptr(geof.contiguous()), _n.ptr(rgb.contiguous()), _n.ptr(nn.nbr), _n.ptr(nn.dist2),
                                           V, k, ka, float(lambda_edge_weight), _n.ptr(features), _n.ptr(source), _n.ptr(target),
                                           _n.ptr(distances), _n.ptr(weight), _n.ptr(mean), _n.ptr(ws), ws_bytes,
                                           _n.stream_ptr()), "pt_edge_features")
    return features, source, target, distances, weight, mean


def partition_inputs(xyz, rgb, voxel_width=0.03, k_nn_adj=10, k_nn_geof=45, lambda_edge_weight=1., device="cuda"):
    """Lines :95-108 of ``generate_SPG_superpoint`` for one room (``xyz`` fp32 [N,3], ``rgb`` uint8 [N,3]):
    -> ``PartitionInputs``"""
    k_nn_adj, k_nn_geof = int(k_nn_adj), int(k_nn_geof)
    if k_nn_geof > K_MAX:
        raise _n.WsisError(f"partition_inputs: k_nn_geof = {k_nn_geof} above {K_MAX}")
    if not 1 <= k_nn_adj <= k_nn_geof:
        raise _n.WsisError(f"partition_inputs: k_nn_adj = {k_nn_adj} outside 1..k_nn_geof = {k_nn_geof}")
    _check_cloud(xyz, "partition_inputs", rgb)
    dev = _device_of(xyz, device, "partition_inputs")
    with torch.cuda.device(dev):
        pr = prune(xyz, voxel_width, rgb, device=dev)
        nn = knn(pr.xyz, k_nn_geof, cell=CELL_VOXELS * float(voxel_width))
        gf = geometric_features(pr.xyz, nn.nbr)
        features, source, target, distances, weight, mean = edge_features(gf.geof, pr.rgb, nn, k_nn_adj, lambda_edge_weight)
    return PartitionInputs(features, source, target, weight, distances, mean, nn.nbr, pr.p2v, pr.xyz, pr.rgb)


# ---- l0 cut pursuit: the stages of csrc/cutpursuit.hip, then the solver ------------------------------------------------

FLOW_STEPS, KMEANS_ITE, KMEANS_RESAMPLING, MAX_ITE_MAIN, STOPPING_RATIO = 3, 5, 10, 15, 0.05     # mode 1, speed 4
FLOW_ROUND_CAP = 4096            # rounds of one min cut before WsisError (the most seen is 24)

Arcs = collections.namedtuple("Arcs", "off head rev edge")
Reduced = collections.namedtuple("Reduced", "mean weight a b border_weight gain")
CutPursuitInfo = collections.namedtuple("CutPursuitInfo", "fidelity penalty components saturated flow_rounds stopped times")


def _ws(nbytes, dev, what):
    if nbytes < 0:
        raise _n.WsisError(f"{what} workspace query failed")
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=dev)


def cp_arcs(source, target, V):
    """the two arcs of every input edge as a CSR by tail node -> ``Arcs``: ``off`` int32 [V+1], and per position ``head``,
    ``rev`` (the position of the opposite arc) and ``edge`` (the input edge), int32 [2E]"""
    dev, E = source.device, int(source.numel())
    lib, st = _n.hip(), _n.stream_ptr()
    tails = torch.empty(2 * E, dtype=torch.int64, device=dev)
    _n.check(lib.wsis_cp_arc_tails(_n.ptr(source), _n.ptr(target), E, _n.ptr(tails), st), "cp_arc_tails")
    csr = segment_csr(tails, V)
    head, rev, edge = (torch.empty(2 * E, dtype=torch.int32, device=dev) for _ in range(3))
    nb = lib.wsis_cp_arcs_workspace_bytes(E)
    ws = _ws(nb, dev, "cp_arcs")
    _n.check(lib.wsis_cp_arcs(_n.ptr(source), _n.ptr(target), E, _n.ptr(csr.perm), _n.ptr(head), _n.ptr(rev), _n.ptr(edge),
                              _n.ptr(ws), nb, st), "cp_arcs")
    return Arcs(csr.offsets, head, rev, edge)


def cp_components(in_component, C):
    """(offsets int32 [C+1], nodes int32 [V]): the nodes of every component, ascending"""
    csr = segment_csr(in_component.long(), int(C))
    return csr.offsets, csr.perm


def cp_kmeans(features, off, nodes, sat, seed, iteration, restarts=KMEANS_RESAMPLING, kmeans_ite=KMEANS_ITE):
    """the 2-means start of a split -> label uint8 [V]"""
    dev, (V, D), C = features.device, features.shape, int(off.numel()) - 1
    label = torch.empty(V, dtype=torch.uint8, device=dev)
    lib = _n.hip()
    nb = lib.wsis_cp_kmeans_workspace_bytes(V)
    ws = _ws(nb, dev, "cp_kmeans")
    _n.check(lib.wsis_cp_kmeans(_n.ptr(features), D, _n.ptr(off), _n.ptr(nodes), _n.ptr(sat), C, V, int(seed) & 0xffffffff,
                                int(iteration), int(restarts), int(kmeans_ite), _n.ptr(label), _n.ptr(ws), nb,
                                _n.stream_ptr()), "cp_kmeans")
    return label


def cp_capacities(features, off, nodes, label, sat):
    """class centres and terminal differences; ``sat`` is updated in place -> (centres fp64 [C,2,D], term fp64 [V])"""
    dev, (V, D), C = features.device, features.shape, int(off.numel()) - 1
    centres = torch.empty((C, 2, D), dtype=torch.float64, device=dev)
    term = torch.empty(V, dtype=torch.float64, device=dev)
    _n.check(_n.hip().wsis_cp_capacities(_n.ptr(features), D, _n.ptr(off), _n.ptr(nodes), C, V, _n.ptr(label), _n.ptr(sat),
                                         _n.ptr(centres), _n.ptr(term), _n.stream_ptr()), "cp_capacities")
    return centres, term


def cp_quantize(term, edge_weight, active, lam, arcs):
    """-> (src_cap int32 [V], snk_cap int32 [V], arc_cap int32 [2E], scale fp64 [2] whose first entry is the scale)"""
    dev, V, E = term.device, int(term.numel()), int(edge_weight.numel())
    src, snk = (torch.empty(V, dtype=torch.int32, device=dev) for _ in range(2))
    cap = torch.empty(2 * E, dtype=torch.int32, device=dev)
    scale = torch.empty(2, dtype=torch.float64, device=dev)
    _n.check(_n.hip().wsis_cp_quantize(_n.ptr(term), V, _n.ptr(edge_weight), _n.ptr(active), E, float(lam), _n.ptr(arcs.edge),
                                       _n.ptr(src), _n.ptr(snk), _n.ptr(cap), _n.ptr(scale), _n.stream_ptr()), "cp_quantize")
    return src, snk, cap, scale


def cp_min_cut(src_cap, snk_cap, arcs, arc_cap, max_rounds=None):
    """-> (sink_side uint8 [V], cut int64 [1], rounds used); ``WsisError`` when ``max_rounds`` do not finish the flow"""
    import ctypes
    dev, V, A = src_cap.device, int(src_cap.numel()), int(arc_cap.numel())
    side = torch.empty(V, dtype=torch.uint8, device=dev)
    cut = torch.empty(1, dtype=torch.int64, device=dev)
    rounds = ctypes.c_int32(0)
    lib = _n.hip()
    nb = lib.wsis_cp_min_cut_workspace_bytes(V, A)
    ws = _ws(nb, dev, "cp_min_cut")
    _n.check(lib.wsis_cp_min_cut(_n.ptr(src_cap), _n.ptr(snk_cap), _n.ptr(arcs.off), _n.ptr(arcs.head), _n.ptr(arcs.rev),
                                 _n.ptr(arc_cap), V, A, int(FLOW_ROUND_CAP if max_rounds is None else max_rounds), _n.ptr(side),
                                 _n.ptr(cut), ctypes.addressof(rounds), _n.ptr(ws), nb, _n.stream_ptr()), "cp_min_cut")
    return side, cut, int(rounds.value)


def cp_activate(source, target, label, in_component, off, nodes, sat, active):
    """saturation and active edges from the last labels (``sat`` and ``active`` are updated in place), then the connected
    components over inactive edges -> (in_component int32 [V], sat uint8 [C'], C')"""
    import ctypes
    dev, V, E, C = label.device, int(label.numel()), int(source.numel()), int(off.numel()) - 1
    comp_new = torch.empty(V, dtype=torch.int32, device=dev)
    sat_new = torch.empty(V, dtype=torch.uint8, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    rounds = ctypes.c_int32(0)
    lib = _n.hip()
    nb = lib.wsis_cp_activate_workspace_bytes(V)
    ws = _ws(nb, dev, "cp_activate")
    _n.check(lib.wsis_cp_activate(_n.ptr(source), _n.ptr(target), E, _n.ptr(label), _n.ptr(in_component), _n.ptr(off),
                                  _n.ptr(nodes), C, V, _n.ptr(sat), _n.ptr(active), _n.ptr(comp_new), _n.ptr(sat_new),
                                  _n.ptr(count), ctypes.addressof(rounds), _n.ptr(ws), nb, _n.stream_ptr()), "cp_activate")
    C_new = int(count)
    return comp_new, sat_new[:C_new].clone(), C_new


def cp_values(features, off, nodes):
    """-> (mean fp64 [C,D], weight fp64 [C])"""
    dev, D, C = features.device, int(features.shape[1]), int(off.numel()) - 1
    mean = torch.empty((C, D), dtype=torch.float64, device=dev)
    weight = torch.empty(C, dtype=torch.float64, device=dev)
    _n.check(_n.hip().wsis_cp_values(_n.ptr(features), D, _n.ptr(off), _n.ptr(nodes), C, _n.ptr(mean), _n.ptr(weight),
                                     _n.stream_ptr()), "cp_values")
    return mean, weight


def cp_reduce(features, source, target, edge_weight, in_component, off, nodes, lam):
    """the reduced graph -> ``Reduced``: per component ``mean`` / ``weight``, per border its components ``a`` < ``b``, its
    ``border_weight`` and the ``gain`` of merging them"""
    dev, D, E, C = features.device, int(features.shape[1]), int(source.numel()), int(off.numel()) - 1
    lib, st = _n.hip(), _n.stream_ptr()
    mean, weight = cp_values(features, off, nodes)
    keys = torch.empty(E, dtype=torch.int64, device=dev)
    _n.check(lib.wsis_cp_border_keys(_n.ptr(source), _n.ptr(target), _n.ptr(in_component), E, C, _n.ptr(keys), st),
             "cp_border_keys")
    skeys, order = torch.sort(keys, stable=True)
    ukeys, counts = torch.unique_consecutive(skeys, return_counts=True)
    B = int(ukeys.numel())
    if B and int(ukeys[-1]) == 0x7fffffffffffffff:
        B -= 1
    boff = torch.zeros(B + 1, dtype=torch.int64, device=dev)
    boff[1:] = torch.cumsum(counts[:B], 0)
    a, b = (torch.empty(B, dtype=torch.int32, device=dev) for _ in range(2))
    bw, gain = (torch.empty(B, dtype=torch.float64, device=dev) for _ in range(2))
    _n.check(lib.wsis_cp_borders(_n.ptr(ukeys), _n.ptr(boff), _n.ptr(order), _n.ptr(edge_weight), E, _n.ptr(mean),
                                 _n.ptr(weight), D, float(lam), B, C, _n.ptr(a), _n.ptr(b), _n.ptr(bw), _n.ptr(gain), st),
             "cp_borders")
    return Reduced(mean, weight, a, b, bw, gain)


def cp_merge(a, b, gain, C):
    """the greedy matching of the borders -> (taken uint8 [B], map int32 [C], rounds)"""
    import ctypes
    dev, B = gain.device, int(gain.numel())
    taken = torch.empty(B, dtype=torch.uint8, device=dev)
    cmap = torch.empty(int(C), dtype=torch.int32, device=dev)
    rounds = ctypes.c_int32(0)
    lib = _n.hip()
    nb = lib.wsis_cp_merge_workspace_bytes(int(C))
    ws = _ws(nb, dev, "cp_merge")
    _n.check(lib.wsis_cp_merge(_n.ptr(a), _n.ptr(b), _n.ptr(gain), B, int(C), _n.ptr(taken), _n.ptr(cmap),
                               ctypes.addressof(rounds), _n.ptr(ws), nb, _n.stream_ptr()), "cp_merge")
    return taken, cmap, int(rounds.value)


def cp_relabel(cmap, source, target, in_component, sat, active):
    """the ids after the merges (``active`` is updated in place) -> (in_component int32 [V], sat uint8 [C'], C')"""
    dev, V, E, C = in_component.device, int(in_component.numel()), int(source.numel()), int(cmap.numel())
    comp_new = torch.empty(V, dtype=torch.int32, device=dev)
    sat_new = torch.empty(C, dtype=torch.uint8, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    lib = _n.hip()
    nb = lib.wsis_cp_relabel_workspace_bytes(C)
    ws = _ws(nb, dev, "cp_relabel")
    _n.check(lib.wsis_cp_relabel(_n.ptr(cmap), C, _n.ptr(source), _n.ptr(target), E, _n.ptr(in_component), V, _n.ptr(sat),
                                 _n.ptr(active), _n.ptr(comp_new), _n.ptr(sat_new), _n.ptr(count), _n.ptr(ws), nb,
                                 _n.stream_ptr()), "cp_relabel")
    C_new = int(count)
    return comp_new, sat_new[:C_new].clone(), C_new


def cp_energy(features, in_component, mean, source, target, edge_weight, lam, sat):
    """-> (fidelity, penalty, nodes in saturated components), read back"""
    dev, (V, D), E, C = features.device, features.shape, int(source.numel()), int(mean.shape[0])
    out = torch.empty(3, dtype=torch.float64, device=dev)
    lib = _n.hip()
    nb = lib.wsis_cp_energy_workspace_bytes()
    ws = _ws(nb, dev, "cp_energy")
    _n.check(lib.wsis_cp_energy(_n.ptr(features), D, _n.ptr(in_component), _n.ptr(mean), V, C, _n.ptr(source), _n.ptr(target),
                                _n.ptr(edge_weight), E, float(lam), _n.ptr(sat), _n.ptr(out), _n.ptr(ws), nb, _n.stream_ptr()),
             "cp_energy")
    fid, pen, nsat = out.tolist()
    return fid, pen, int(nsat)


class _StageTimes(object):
    """device time per stage between events (``None``: no events are recorded)"""

    def __init__(self):
        self.pairs = []

    def start(self):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def stop(self, name, e0):
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record()
        self.pairs.append((name, e0, e1))

    def totals(self):
        torch.cuda.synchronize()
        out = collections.OrderedDict()
        for name, e0, e1 in self.pairs:
            out[name] = out.get(name, 0.0) + e0.elapsed_time(e1)
        return out


def _cut_pursuit_device(features, source, target, edge_weight, lam, seed, timed):
    V, E = int(features.shape[0]), int(source.numel())
    dev = features.device
    times = _StageTimes() if timed else None

    def stage(name, fn, *args):
        if times is None:
            return fn(*args)
        e0 = times.start()
        out = fn(*args)
        times.stop(name, e0)
        return out

    arcs = stage("arcs", cp_arcs, source, target, V)
    in_comp = torch.zeros(V, dtype=torch.int32, device=dev)
    sat = torch.zeros(1, dtype=torch.uint8, device=dev)
    active = torch.zeros(E, dtype=torch.uint8, device=dev)
    C = 1
    off, nodes = cp_components(in_comp, C)
    mean, _ = cp_values(features, off, nodes)
    old_energy = cp_energy(features, in_comp, mean, source, target, edge_weight, lam, sat)[0]
    fidelity, penalty, components, saturated, flow_rounds, stopped = [], [], [], [], [], "iterations"
    for it in range(1, MAX_ITE_MAIN + 1):
        label = stage("kmeans", cp_kmeans, features, off, nodes, sat, seed, it)
        for _ in range(FLOW_STEPS):
            _, term = stage("capacities", cp_capacities, features, off, nodes, label, sat)
            src, snk, cap, _ = stage("capacities", cp_quantize, term, edge_weight, active, lam, arcs)
            label, _, rounds = stage("min_cut", cp_min_cut, src, snk, arcs, cap)
            flow_rounds.append(rounds)
        in_comp, sat, C = stage("activate", cp_activate, source, target, label, in_comp, off, nodes, sat, active)
        off, nodes = stage("reduce", cp_components, in_comp, C)
        red = stage("reduce", cp_reduce, features, source, target, edge_weight, in_comp, off, nodes, lam)
        _, cmap, _ = stage("merge", cp_merge, red.a, red.b, red.gain, C)
        in_comp, sat, C = stage("merge", cp_relabel, cmap, source, target, in_comp, sat, active)
        off, nodes = stage("merge", cp_components, in_comp, C)
        mean, _ = stage("energy", cp_values, features, off, nodes)
        fid, pen, nsat = stage("energy", cp_energy, features, in_comp, mean, source, target, edge_weight, lam, sat)
        fidelity.append(fid)
        penalty.append(pen)
        components.append(C)
        saturated.append(nsat)
        if nsat == V:
            stopped = "saturated"
            break
        if old_energy > 0 and (old_energy - fid - pen) / old_energy < STOPPING_RATIO:
            stopped = "energy"
            break
        old_energy = fid + pen
    info = CutPursuitInfo(fidelity, penalty, components, saturated, flow_rounds, stopped,
                          None if times is None else times.totals())
    return in_comp, off, nodes, info


def cut_pursuit(features, source, target, edge_weight, reg_strength, cutoff=0, spatial=0, weight_decay=1., *, seed=0,
                info=False, device="cuda", _timed=False):
    """``libcp.cutpursuit(features, source, target, edge_weight, reg_strength)`` (cut-pursuit/src/cutpursuit.cpp:77-105; l0
    cut pursuit, L2 fidelity, speed 4) on the device.  ``features`` fp32 [V,D] (D <= 8), ``source`` / ``target`` uint32 [E]
    (tensors: int32), ``edge_weight`` fp32 [E], all numpy or all device tensors.  Numpy in: ``(components, in_component)``
    as the reference returns them -- a list of ascending uint32 index arrays and uint32 [V].  Tensors in:
    ``((offsets int32 [C+1], nodes int32 [V]), in_component int32 [V])`` on the device.  Component ids ascend with the
    components' smallest nodes.  ``info=True`` appends a ``CutPursuitInfo``: per main iteration ``fidelity``,
    ``penalty``, ``components`` and ``saturated`` (nodes), ``flow_rounds`` per min cut, and ``stopped`` ('saturated',
    'energy' or 'iterations').  Same input and ``seed``: same bits."""
    what = "cut_pursuit"
    if cutoff != 0 or spatial != 0 or weight_decay != 1.:
        raise _n.WsisError(f"{what}: cutoff = {cutoff}, spatial = {spatial}, weight_decay = {weight_decay}: only 0, 0 and 1 "
                           f"(the S3DIS partition's values) are implemented")
    as_numpy = not torch.is_tensor(features)
    index_dtypes = (np.uint32, np.int32) if as_numpy else (torch.int32,)
    if _dtype_of(features) not in (torch.float32, np.float32) or _dtype_of(edge_weight) not in (torch.float32, np.float32):
        raise _n.WsisError(f"{what}: features and edge_weight must be float32, got {_dtype_of(features)} and "
                           f"{_dtype_of(edge_weight)}")
    if _dtype_of(source) not in index_dtypes or _dtype_of(target) not in index_dtypes:
        raise _n.WsisError(f"{what}: source and target must be uint32 (device tensors: int32), got {_dtype_of(source)} and "
                           f"{_dtype_of(target)}")
    if len(features.shape) != 2 or not 1 <= int(features.shape[1]) <= 8:
        raise _n.WsisError(f"{what}: features must have shape [V, D <= 8], got {tuple(features.shape)}")
    V, E = int(features.shape[0]), int(source.shape[0])
    if V == 0:
        raise _n.WsisError(f"{what}: a graph without nodes")
    if not (int(target.shape[0]) == E and int(edge_weight.shape[0]) == E):
        raise _n.WsisError(f"{what}: {E} sources, {int(target.shape[0])} targets and {int(edge_weight.shape[0])} weights")
    lam = float(reg_strength)
    if not (lam >= 0 and np.isfinite(lam)):
        raise _n.WsisError(f"{what}: reg_strength = {reg_strength}")
    dev = _device_of(features, device, what)
    with torch.cuda.device(dev):
        f = _upload(features, dev)
        w = _upload(edge_weight, dev).reshape(-1)
        if as_numpy:
            source, target = (np.ascontiguousarray(a).view(np.int32) if a.dtype == np.uint32 else a for a in (source, target))
        s, t = _upload(source, dev).reshape(-1), _upload(target, dev).reshape(-1)
        if E:
            lo, hi = min(int(s.min()), int(t.min())), max(int(s.max()), int(t.max()))
            if lo < 0 or hi >= V:
                raise _n.WsisError(f"{what}: node indices span {np.uint32(lo)}..{np.uint32(hi)}, outside 0..{V - 1}")
            if not bool(torch.isfinite(w).all()) or float(w.min()) < 0 or not np.isfinite(lam * float(w.max())):
                raise _n.WsisError(f"{what}: an edge weight is negative or not finite")
        if not bool(torch.isfinite(f).all()):
            raise _n.WsisError(f"{what}: a feature is NaN or infinite")
        in_comp, off, nodes, run = _cut_pursuit_device(f, s, t, w, lam, seed, _timed)
    if as_numpy:
        o, n = off.cpu().numpy(), nodes.cpu().numpy().astype(np.uint32)
        out = ([n[o[c]:o[c + 1]] for c in range(len(o) - 1)], in_comp.cpu().numpy().astype(np.uint32))
    else:
        out = ((off, nodes), in_comp)
    return out + (run,) if info else out


def generate_superpoints(xyz, rgb, cutpursuit=None, reg_strength=0.03, device="cuda", **kwargs):
    """``generate_SPG_superpoint`` (:81-115).  ``cutpursuit=None``: the device solver ``cut_pursuit``, fed the device
    tensors of ``partition_inputs`` directly; or a callable ``cutpursuit(features, source, target, edge_weight,
    reg_strength) -> (components, in_component)``, the signature of ``libcp.cutpursuit``, which gets numpy arrays.
    Returns the point-level superpoint ids the reference stores in its ``.npy`` (:172-177), a numpy array of N entries."""
    inputs = partition_inputs(xyz, rgb, device=device, **kwargs)
    if cutpursuit is None:
        _, in_component = cut_pursuit(inputs.features, inputs.source, inputs.target, inputs.edge_weight, reg_strength)
        return inputs.to_points(in_component).cpu().numpy().astype(np.uint32)
    _, in_component = cutpursuit(*inputs.solver_args(reg_strength))
    return inputs.to_points(np.asarray(in_component))
