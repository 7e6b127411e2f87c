"""Test-time instance grouping on the superpoint graph: drop-in for ``clustering_in_graph`` of the reference's
``test_scannetv2.py:281-455`` (called at :257-260 for every scene; ``test_s3dis.py`` uses the same routine).

Same signature, same return values ``(conf [n] float, label_id [n] int, ins_mask [n, N] int)``.  The reference
builds a boolean point mask per superpoint (``superpoint == spID``: O(S*N)), ORs masks while it grows a group and
calls the CPU ``voxelization_idx`` once per group.  Here the per-point work is segmented and runs on the MI355X:

  superpoint centres        one segmented mean over the points        (torch_scatter drop-in -> wsis_segment_reduce)
  graph BFS                 wsis_host_graph_bfs over the S superpoints (host, O(S + E), seed order = reference)
  group voxel counts        ONE wsis_voxelize_idx over (group id, floor-to-zero(xyz*50)) of all grouped points
  instance masks            one gather + compare on the device
  S3DIS walls (wall_class)  get_room_walls: per wall ONE wsis_plane_score over all candidate planes + wsis_plane_mark

The per-group scalars (occupancy, radii, centres) and the fragment absorption are the reference's expressions on
<= a few hundred groups (host numpy).  The group sets equal the reference's (the acceptance test depends on the seed
only, so a group is a connected component of accepted edges among unvisited superpoints -- independent of the
visiting order); float results agree to rounding (member order of a Python ``set`` is not reproducible).
"""
from math import sqrt

import numpy as np
import torch

import pointgroup_ops
import wsis_native as _n
from torch_scatter import scatter

# test_scannetv2.py:288-289
SEMANTIC_IND2LABEL = np.array([1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39])
INSTANCE_VALID_LABELS = np.array([3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39])


def adjacency_csr(graph, S):
    """``graph``: an igraph-like object (``neighbors(vertex=, mode='all')``) or a pair of edge index arrays
    (u, v).  -> (offsets int32 [S+1], neighbours int32 [nnz]) with mode='all' semantics (both directions)."""
    if hasattr(graph, "neighbors"):
        lists = [np.asarray(graph.neighbors(vertex=s, mode="all"), dtype=np.int64) for s in range(S)]
        off = np.zeros(S + 1, dtype=np.int32)
        off[1:] = np.cumsum([len(l) for l in lists])
        adj = np.concatenate(lists).astype(np.int32) if S else np.zeros(0, np.int32)
        return off, adj
    u, v = (np.asarray(a, dtype=np.int64).reshape(-1) for a in graph)
    src = np.concatenate([u, v])
    dst = np.concatenate([v, u])
    order = np.lexsort((dst, src))
    src, dst = src[order], dst[order]
    off = np.zeros(S + 1, dtype=np.int32)
    off[1:] = np.cumsum(np.bincount(src, minlength=S))
    return off, dst.astype(np.int32)


# test_s3dis.py:297-541: 13 classes, ceiling / floor / wall (0, 1, 2) are stuff, growth radius 0.8 * size
S3DIS_LABEL_IDX = np.array([1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13])
S3DIS_VALID_LABELS = S3DIS_LABEL_IDX[3:]


def graph_bfs(label, class_valid, centre, ins_size, adj_off, adj):
    """wsis_host_graph_bfs -> (group int32 [S], n_groups)"""
    import ctypes
    S = int(label.shape[0])
    label = np.ascontiguousarray(label, dtype=np.int32)
    class_valid = np.ascontiguousarray(class_valid, dtype=np.uint8)
    centre = np.ascontiguousarray(centre, dtype=np.float32)
    ins_size = np.ascontiguousarray(ins_size, dtype=np.float32).reshape(-1)
    adj_off = np.ascontiguousarray(adj_off, dtype=np.int32)
    adj = np.ascontiguousarray(adj, dtype=np.int32)
    group = np.empty(S, dtype=np.int32)
    ng = ctypes.c_int64(0)
    _n.check_host(_n.host().wsis_host_graph_bfs(label.ctypes.data, class_valid.ctypes.data, len(class_valid),
                                                centre.ctypes.data, ins_size.ctypes.data, adj_off.ctypes.data,
                                                adj.ctypes.data, S, group.ctypes.data, ctypes.addressof(ng)),
                  "graph_bfs")
    return group, int(ng.value)


# ---- S3DIS wall split: utils/planeSegment.py:29-63 (open3d segment_plane per wall) ------------------------------

PLANE_SCORE_MAX_H = 1024          # hypotheses per wsis_plane_score call


def plane_score(xyz, planes, thr, out=None, workspace=None):
    """wsis_plane_score: ``xyz`` fp32 [N,3] and ``planes`` fp64 [H,4] (unit normals) on the device ->
    (count int64 [H], sumsq fp64 [H]): points with |((a*x + b*y) + c*z) + d| < thr and the sum of their squared
    distances.  ``out`` = (count, sumsq) / ``workspace`` (uint8): caller-owned buffers instead of fresh ones."""
    _n.require_cuda(xyz, planes)
    if xyz.dtype != torch.float32 or planes.dtype != torch.float64 or xyz.dim() != 2 or xyz.shape[1] != 3 \
            or planes.dim() != 2 or planes.shape[1] != 4:
        raise ValueError("plane_score wants xyz fp32 [N,3] and planes fp64 [H,4]")
    xyz, planes = xyz.contiguous(), planes.contiguous()
    N, H = int(xyz.shape[0]), int(planes.shape[0])
    if out is None:
        out = (torch.empty(H, dtype=torch.int64, device=xyz.device), torch.empty(H, dtype=torch.float64, device=xyz.device))
    count, sumsq = out
    _n.require_cuda(count, sumsq, workspace)
    assert count.dtype == torch.int64 and sumsq.dtype == torch.float64 and count.numel() >= H and sumsq.numel() >= H
    with torch.cuda.device(xyz.device):
        if workspace is None:
            nbytes = int(_n.hip().wsis_plane_score_workspace_bytes(N, H))
            if nbytes < 0:
                raise _n.WsisError(f"plane_score: no workspace for N={N}, H={H} (1 <= H <= {PLANE_SCORE_MAX_H})")
            workspace = torch.empty(nbytes, dtype=torch.uint8, device=xyz.device)
        _n.check(_n.hip().wsis_plane_score(_n.ptr(xyz), N, _n.ptr(planes), H, float(thr), _n.ptr(count), _n.ptr(sumsq),
                                           _n.ptr(workspace), int(workspace.numel()), _n.stream_ptr()), "plane_score")
    return count, sumsq


def plane_mark(xyz, plane4, thr, out=None):
    """wsis_plane_mark: uint8 [N], 1 where the point is closer than ``thr`` to the plane ``plane4`` (fp64 [4], device)"""
    _n.require_cuda(xyz, plane4, out)
    if xyz.dtype != torch.float32 or plane4.dtype != torch.float64 or xyz.dim() != 2 or xyz.shape[1] != 3 \
            or plane4.numel() != 4:
        raise ValueError("plane_mark wants xyz fp32 [N,3] and one fp64 plane (a, b, c, d)")
    xyz, plane4 = xyz.contiguous(), plane4.contiguous()
    N = int(xyz.shape[0])
    if out is None:
        out = torch.empty(N, dtype=torch.uint8, device=xyz.device)
    assert out.dtype == torch.uint8 and out.numel() >= N
    with torch.cuda.device(xyz.device):
        _n.check(_n.hip().wsis_plane_mark(_n.ptr(xyz), N, _n.ptr(plane4), float(thr), _n.ptr(out), _n.stream_ptr()),
                 "plane_mark")
    return out


def sample_triples(n, iters, rng):
    """int64 [iters, 3]: per iteration three distinct indices below ``n``, one ``rng.choice(n, 3, replace=False)`` each"""
    if n < 3:
        raise ValueError("a plane needs three distinct points")
    if iters < 1:
        return np.zeros((0, 3), dtype=np.int64)
    return np.stack([rng.choice(n, 3, replace=False) for _ in range(iters)]).astype(np.int64).reshape(iters, 3)


def planes_from_triples(pts):
    """``pts`` [H,3,3] (hypothesis, point, coordinate) -> (planes fp64 [H,4], valid bool [H]).  n = (p1-p0) x (p2-p0),
    plane = (n / |n|, -n.p0) in fp64, written element-wise (no BLAS: its fused or reordered sums round differently).
    |n| = 0 -- collinear or repeated points -- or a non-finite point marks the hypothesis invalid, as open3d skips it."""
    p = np.asarray(pts, dtype=np.float64).reshape(-1, 3, 3)
    p0, u, v = p[:, 0], p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        nx = u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1]
        ny = u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2]
        nz = u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]
        norm = np.sqrt((nx * nx + ny * ny) + nz * nz)
        valid = norm > 0                         # NaN compares false
        a, b, c = nx / norm, ny / norm, nz / norm
        d = -((a * p0[:, 0] + b * p0[:, 1]) + c * p0[:, 2])
        planes = np.stack([a, b, c, d], 1)
    valid &= np.isfinite(planes).all(1)
    planes[~valid] = 0.0
    return planes, valid


def choose_plane(count, sumsq):
    """open3d's choice among the scored hypotheses: most inliers; on equal counts the smaller inlier RMSE (equal counts:
    the smaller sum of squares); on equal both the earliest (its comparison is strict).  -> index, or -1 for none."""
    count, sumsq = np.asarray(count), np.asarray(sumsq)
    if count.size == 0:
        return -1
    top = np.nonzero(count == count.max())[0]
    return int(top[np.argmin(sumsq[top])])       # argmin returns the first minimum


def _room_walls_device(xyz, wall, distance, iters, max_num, seed, samples, min_points):
    """the loop of get_room_walls on device tensors: ``xyz`` fp32 [N,3], ``wall`` bool [N] -> list of bool [N] tensors"""
    rem_ind = torch.nonzero(wall).flatten()                      # ascending: the reference's remain_wall_ind
    rem_xyz = xyz[rem_ind].contiguous()
    rng = np.random.default_rng(seed) if samples is None else None
    walls = []
    for rnd in range(max_num):
        n = int(rem_ind.numel())
        if n < min_points or n < 3:
            break
        if samples is None:
            tri = sample_triples(n, iters, rng)
        else:
            tri = np.asarray(samples[rnd], dtype=np.int64).reshape(-1, 3)
            if tri.size and (tri.min() < 0 or tri.max() >= n):
                raise ValueError(f"samples[{rnd}] indexes outside the {n} remaining wall points")
        picked = rem_xyz[torch.from_numpy(tri.reshape(-1)).to(xyz.device)].cpu().numpy()     # <= 3 * iter points
        planes, valid = planes_from_triples(picked.reshape(-1, 3, 3))
        planes = planes[valid]                                   # keeps the iteration order
        if len(planes) == 0:
            break                                                # no plane at all (see get_room_walls)
        planes_d = torch.from_numpy(planes).to(xyz.device)
        count, sumsq = [], []
        for h0 in range(0, len(planes), PLANE_SCORE_MAX_H):
            c, s = plane_score(rem_xyz, planes_d[h0:h0 + PLANE_SCORE_MAX_H], distance)
            count.append(c.cpu().numpy())
            sumsq.append(s.cpu().numpy())
        count, sumsq = np.concatenate(count), np.concatenate(sumsq)
        best = choose_plane(count, sumsq)
        if count[best] == 0:
            break                                                # `distance` admits no point at all: no plane either
        inl = plane_mark(rem_xyz, planes_d[best], distance).bool()
        mask = torch.zeros(xyz.shape[0], dtype=torch.bool, device=xyz.device)
        mask[rem_ind[inl]] = True
        walls.append(mask)
        rem_ind, rem_xyz = rem_ind[~inl], rem_xyz[~inl].contiguous()
    return walls


def get_room_walls(xyz, wall_ind, distance=0.1, init_n=3, iter=200, max_num=4, device="cuda", seed=None, samples=None,
                   min_points=10000):
    """Drop-in for ``utils/planeSegment.py:get_room_walls`` (test_s3dis.py:533 calls it with ``max_num=10``): split
    the points flagged by ``wall_ind`` into planar walls, one RANSAC plane per round, and return one bool [N] numpy
    mask over the whole cloud per wall, in round order.  The first six parameters and the result are the reference's.

    A round works on the remaining wall points in their original order: ``iter`` 3-point planes are fitted on the host
    in fp64 from the sampled points, ONE wsis_plane_score call counts the points closer than ``distance`` to every
    plane (and sums their squared distances), the host keeps the plane with the most inliers (ties: smaller sum of
    squares = open3d's smaller RMSE, then the earlier iteration), wsis_plane_mark writes its inlier mask and the inliers
    leave the remaining set.  Like the reference, the wall is the inlier set of the best SAMPLED plane: open3d's refitted
    model is discarded there too.  Rounds stop when fewer than ``min_points`` (reference: 10000) points remain or after
    ``max_num`` rounds.  Per-point data reaches the host only as the final masks.

    Sampling.  open3d seeds its sampler from ``std::random_device``, so the reference's own draw is not reproducible
    and parity is pinned on the algorithm GIVEN the triples: ``samples[round]`` is an int [iter, 3] array of indices
    into that round's remaining points; without it the triples are drawn from ``numpy.random.default_rng(seed)``, one
    ``choice(n, 3, replace=False)`` per iteration.

    Deliberate difference: a round in which no triple spans a plane (all collinear or repeated points; such triples are
    skipped, as in open3d) ends the loop without a wall.  Upstream would return its zero-initialised model, for which
    every point is an inlier.  Coordinates are read as fp32, like everywhere on this path."""
    if init_n != 3:
        raise ValueError("get_room_walls fits planes through 3 points (the reference never passes another init_n)")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _n.WsisError("get_room_walls scores its planes on the MI355X (there is no CPU fallback)")
    xyz_d = torch.as_tensor(np.ascontiguousarray(xyz, dtype=np.float32) if not torch.is_tensor(xyz) else xyz)
    xyz_d = xyz_d.to(dev, torch.float32).reshape(-1, 3)
    wall_d = torch.as_tensor(np.asarray(wall_ind).astype(bool) if not torch.is_tensor(wall_ind) else wall_ind).to(dev).bool()
    assert wall_d.shape == (xyz_d.shape[0],)
    walls = _room_walls_device(xyz_d, wall_d, float(distance), int(iter), int(max_num), seed, samples, int(min_points))
    if not walls:
        return []
    return list(torch.stack(walls).cpu().numpy())


def clustering_in_graph(scene_name, xyz_origin, superpoint, graph, sp_semnatic_pred, pred_sp_offset_vectors,
                        pred_sp_occupancy, pred_sp_ins_size, device="cuda", semantic_ind2label=SEMANTIC_IND2LABEL,
                        valid_labels=INSTANCE_VALID_LABELS, radius_factor=0.25, stuff_classes=(), wall_class=None,
                        wall_kwargs=None, as_tensor=False):
    """``radius_factor``: 0.25 (ScanNet, test_scannetv2.py:331) / 0.8 (S3DIS, test_s3dis.py:349).
    ``stuff_classes``: predicted classes reported as ONE instance each (confidence 1) when they cover more than 100
    points -- ceiling and floor of test_s3dis.py:524-531, appended after the grouped instances.
    ``wall_class``: the predicted class (S3DIS: 2) whose points are split into planar walls by ``get_room_walls``
    (open3d's RANSAC ``segment_plane`` in the reference, utils/planeSegment.py); every wall is appended after the stuff
    entries with confidence 1 and label ``semantic_ind2label[wall_class]``, in round order (test_s3dis.py:533-538).
    ``wall_kwargs``: keyword arguments for ``get_room_walls`` (default ``max_num=10``, as test_s3dis.py:533).  With the
    default ``wall_class=None`` there is no wall split and the call is what it was without the keyword.
    ``as_tensor``: return ``ins_mask`` as the int64 [n, N] device tensor it is built as instead of copying it to the host
    (``wsis_eval`` takes it as it is); without instances it is an empty [0, N] tensor.  ``conf`` and ``label_id`` stay
    host arrays."""
    assert len(xyz_origin) == len(superpoint)
    N, S = len(xyz_origin), len(sp_semnatic_pred)
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _n.WsisError("clustering_in_graph runs its per-point stages on the MI355X (there is no CPU fallback)")
    xyz_h = np.ascontiguousarray(xyz_origin, dtype=np.float32)
    sp_h = np.ascontiguousarray(superpoint).astype(np.int64)
    label = np.asarray(sp_semnatic_pred).astype(np.int64)
    offs = np.asarray(pred_sp_offset_vectors, dtype=np.float32)
    occ = np.asarray(pred_sp_occupancy, dtype=np.float32).reshape(S, -1)
    size = np.asarray(pred_sp_ins_size, dtype=np.float32).reshape(S, -1)

    xyz = torch.from_numpy(xyz_h).to(dev)
    sp = torch.from_numpy(sp_h).to(dev)
    # superpoint centre + predicted offset = predicted instance centre (test_scannetv2.py:299-305)
    centre = scatter(xyz, sp, dim=0, reduce="mean")[:S]
    sp_count = torch.bincount(sp, minlength=S)[:S]
    inst_centre = (centre + torch.from_numpy(offs).to(dev)).cpu().numpy()
    sp_count_h = sp_count.cpu().numpy().astype(np.int64)

    class_valid = np.isin(semantic_ind2label, valid_labels)
    adj_off, adj = adjacency_csr(graph, S)
    # the operator compares against 0.25 * size[seed]: other radii go in through the size argument
    seed_size = size[:, 0] if radius_factor == 0.25 else (size[:, 0] * np.float32(radius_factor / 0.25))
    group, n_groups = graph_bfs(label, class_valid, inst_centre, seed_size, adj_off, adj)
    if n_groups == 0 and not stuff_classes and wall_class is None:
        return np.array([]), np.array([]), (torch.zeros((0, N), dtype=torch.int64, device=dev) if as_tensor else np.array([]))

    # points -> group id; voxels per group with ONE voxelization_idx over (group, trunc(xyz * 50))
    group_d = torch.from_numpy(group).to(dev)
    pg = group_d[sp]                                               # [N] group of every point, -1 = ungrouped
    if n_groups > 0:
        sel = torch.nonzero(pg >= 0).flatten()
        vox = (xyz[sel] * 50).long()                               # float32 product, truncation: as :381-383
        coords = torch.cat([pg[sel].long().unsqueeze(1), vox], 1).contiguous()
        voxel_locs, _, _ = pointgroup_ops.voxelization_idx(coords, n_groups, 4)
        group_voxels = torch.bincount(voxel_locs[:, 0], minlength=n_groups).cpu().numpy()
        group_n = torch.bincount(pg[sel].long(), minlength=n_groups).cpu().numpy()

    members = [np.nonzero(group == g)[0] for g in range(n_groups)]     # ascending superpoint ids
    seed_label = np.array([label[m[0]] for m in members])

    def occupancy_of(m):          # get_group_pred_occupancy, :345-349
        return np.exp(occ[m]).mean()

    def centre_of(m):             # get_group_instance_center, :352-360 (float64 accumulation)
        w = sp_count_h[m].astype(np.float64)
        return (inst_centre[m].astype(np.float64) * w[:, None]).sum(0) / w.sum()

    def size_of(m):               # get_group_instance_size, :362-364
        return np.mean(size[m])

    primaries, fragments = [], []
    for g in range(n_groups):
        m = members[g]
        group_occ = occupancy_of(m)
        if group_voxels[g] < 0.3 * group_occ:                          # :388-393
            fragments.append({"groups": [g], "members": m, "classLabel": seed_label[g], "centre": centre_of(m),
                              "group_n": int(group_n[g])})
        else:
            r_set = max(0.01 * sqrt(group_n[g]), 0.02 * sqrt(group_occ), size_of(m))   # :395-399
            primaries.append({"groups": [g], "members": m, "classLabel": seed_label[g], "centre": centre_of(m),
                              "r_set": r_set, "group_n": int(group_n[g])})

    for frag in fragments:                                             # :410-438
        index, dis_min = -1, float("inf")
        for i, prim in enumerate(primaries):
            dis = np.linalg.norm(frag["centre"] - prim["centre"], ord=2)
            if frag["classLabel"] == prim["classLabel"] and dis < dis_min:
                index, dis_min = i, dis
        if not primaries:
            break
        closest = primaries[index]
        if dis_min < closest["r_set"]:
            m = np.concatenate([frag["members"], closest["members"]])
            n_pts = frag["group_n"] + closest["group_n"]               # the masks are disjoint: |a or b| = |a| + |b|
            closest["r_set"] = max(0.02 * sqrt(occupancy_of(m)), 0.01 * sqrt(n_pts), closest["r_set"], size_of(m))
            closest["centre"] = centre_of(m)
            closest["group_n"] = n_pts
            closest["members"] = np.concatenate([closest["members"], frag["members"]])
            closest["groups"] += frag["groups"]

    # ---- results (:441-455) -------------------------------------------------------------------------------
    conf, label_id = [], []
    inst_of_group = np.full(max(n_groups, 1), -1, dtype=np.int64)
    for i, prim in enumerate(primaries):
        conf.append(min(prim["group_n"] / occupancy_of(prim["members"]), 1))
        label_id.append(semantic_ind2label[prim["classLabel"]])
        inst_of_group[prim["groups"]] = i
    mask_rows = []
    if primaries:
        inst_d = torch.from_numpy(inst_of_group).to(dev)
        pi = torch.where(pg >= 0, inst_d[pg.clamp(min=0).long()], torch.full_like(pg, -1, dtype=torch.int64))
        mask_rows.append((pi.unsqueeze(0) == torch.arange(len(primaries), device=dev).unsqueeze(1)).to(torch.int64))
    if stuff_classes or wall_class is not None:
        point_label = torch.from_numpy(label).to(dev)[sp]
    if stuff_classes:                                                  # test_s3dis.py:524-531
        for c in stuff_classes:
            m = point_label == int(c)
            if int(m.sum()) > 100:
                conf.append(1)
                label_id.append(semantic_ind2label[int(c)])
                mask_rows.append(m.to(torch.int64).unsqueeze(0))
    if wall_class is not None:                                         # test_s3dis.py:533-538
        kw = dict(max_num=10)
        kw.update(wall_kwargs or {})
        if kw.pop("init_n", 3) != 3:
            raise ValueError("get_room_walls fits planes through 3 points")
        walls = _room_walls_device(xyz, point_label == int(wall_class), float(kw.pop("distance", 0.1)),
                                   int(kw.pop("iter", 200)), int(kw.pop("max_num")), kw.pop("seed", None),
                                   kw.pop("samples", None), int(kw.pop("min_points", 10000)))
        if kw:
            raise TypeError(f"wall_kwargs: unknown get_room_walls arguments {sorted(kw)}")
        for w in walls:
            conf.append(1)
            label_id.append(semantic_ind2label[int(wall_class)])
            mask_rows.append(w.to(torch.int64).unsqueeze(0))
    if not mask_rows:
        return np.array([]), np.array([]), (torch.zeros((0, N), dtype=torch.int64, device=dev) if as_tensor else np.array([]))
    ins_mask = torch.cat(mask_rows, 0)
    return np.array(conf), np.array(label_id), (ins_mask if as_tensor else ins_mask.cpu().numpy())


def superpoint_majority_label(point_pred, superpoint, n_class, device="cuda"):
    """Middle-level semantic prediction of test_scannetv2.py:216-224: every point gets the most frequent point-level
    class of its superpoint (``scipy.stats.mode`` semantics: the SMALLEST class among ties).  The reference loops over
    the superpoints with one ``np.where`` each (O(S*N)); here it is one [S, n_class] histogram (index_add) + argmax
    + gather on the device.  Returns (per-point labels int64 [N], per-superpoint labels int64 [S])."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _n.WsisError("superpoint_majority_label runs on the MI355X (there is no CPU fallback)")
    pred = torch.as_tensor(point_pred).to(dev).long()
    sp = torch.as_tensor(superpoint).to(dev).long()
    S = int(sp.max().item()) + 1 if sp.numel() else 0
    hist = torch.zeros(S * n_class, dtype=torch.int32, device=dev)
    hist.index_add_(0, sp * n_class + pred, torch.ones_like(pred, dtype=torch.int32))
    hist = hist.view(S, n_class)
    # argmax with ties -> smallest class: torch.argmax may return any maximal index, so compare against the row max
    first = (hist == hist.max(1, keepdim=True)[0]).to(torch.int32).argmax(1) if S else hist.new_zeros(0).long()
    return first[sp], first


def broadcast_superpoint_label(sp_label, superpoint, device="cuda"):
    """test_scannetv2.py:236-240: point_level_pred[superpoint == spID] = sp_label[spID] for every spID, as one gather"""
    dev = torch.device(device)
    return torch.as_tensor(sp_label).to(dev)[torch.as_tensor(superpoint).to(dev).long()]
