"""The S3DIS partition front end on the device: what ``generate_SPG_superpoint`` of the reference's
``data/S3DIS/partition/partition_S3DIS.py`` (:81-115) computes per room before and after the l0 cut-pursuit solver.

    prune(xyz, voxel_width, rgb, labels, n_labels)     libply_c.prune        ply_c/ply_c.cpp:293-392
    knn(xyz, k)                                        compute_graph_nn_2    graphs.py:26-83 (sklearn kd-tree)
    geometric_features(xyz, nbr)                       libply_c.compute_geof ply_c/ply_c.cpp:396-474 (Eigen)
    partition_inputs(xyz, rgb)                         :95-108, the argument list of libcp.cutpursuit
    generate_superpoints(xyz, rgb, cutpursuit)         :81-115 with the caller's solver, -> point-level superpoint ids

Cut pursuit itself is a max-flow solver and is not part of this package: ``PartitionInputs.solver_args`` is exactly
what ``libcp.cutpursuit`` takes, in its dtypes, and ``PartitionInputs.to_points`` is the back-projection of :113.

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


def generate_superpoints(xyz, rgb, cutpursuit, reg_strength=0.03, device="cuda", **kwargs):
    """``generate_SPG_superpoint`` (:81-115) with the caller's solver: ``cutpursuit(features, source, target,
    edge_weight, reg_strength) -> (components, in_component)``, the signature of ``libcp.cutpursuit``.  Returns the
    point-level superpoint ids the reference stores in its ``.npy`` (:172-177), a numpy array of N entries."""
    inputs = partition_inputs(xyz, rgb, device=device, **kwargs)
    _, in_component = cutpursuit(*inputs.solver_args(reg_strength))
    return inputs.to_points(np.asarray(in_component))
