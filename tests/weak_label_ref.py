"""Vectorised numpy oracle of the weak-label stage updates (``3d-wsis_amd/wsis_weak_labels.py``), written from the
semantics of ``modules/datasets/scannetv2_dataset.py:515-964`` of the reference, not from its code:

* a superpoint is LABELLED when its semantic and its instance label are both != -100;
* centres are fp32 means of the fp32 coordinates, accumulated in fp32 (point order of the superpoint);
* everything that enters a comparison -- instance centres, distances -- is fp64, evaluated element-wise as
  ``sqrt((dx*dx + dy*dy) + dz*dz)`` (no BLAS, no einsum: their fused or blocked sums round differently).

The functions work on plain arrays; ``Scene`` and the ``*_graph`` wrappers put them behind the interface of the device
module for the tests.  Nothing here forms an [S, N] mask either, so that it can stand in for the reference as the host
baseline of ``tools/weak_label_bench.py``.
"""
import numpy as np

NONE = -100
STAT_NAMES = ("GT_all", "GT_label", "semantic_label_num", "correct_semantic_label_num", "floor_wall_sem_num",
              "floor_wall_correct_sem_num", "instance_label_num", "correct_instance_label_num")


def gap_bound(xyz, superpoint):
    """GAP = 4 (n_max + 2) 2^-24 max|coordinate|: a first-order bound on what an fp32 mean of up to n_max points, taken
    in any summation order, can move a distance between two such centres (each of the n_max - 1 additions and the
    division rounds by at most 2^-24 relative, per centre; two centres, and a factor 2 for the three coordinates)."""
    n_max = int(np.bincount(np.asarray(superpoint).astype(np.int64)).max())
    return 4.0 * (n_max + 2) * 2.0 ** -24 * float(np.abs(np.asarray(xyz, dtype=np.float64)).max())


def labelled(sem, ins):
    return (np.asarray(sem) != NONE) & (np.asarray(ins) != NONE)


def sp_stats(xyz, superpoint, S):
    """-> (sum fp32 [S,3], count int64 [S], centre fp32 [S,3]); fp32 accumulation in point order"""
    xyz = np.ascontiguousarray(xyz, dtype=np.float32)
    sp = np.asarray(superpoint).astype(np.int64)
    count = np.bincount(sp, minlength=S)
    if (count == 0).any():
        raise ValueError("a superpoint without points")
    order = np.argsort(sp, kind="stable")
    starts = np.concatenate([[0], np.cumsum(count)[:-1]])
    total = np.add.reduceat(xyz[order], starts, axis=0).astype(np.float32)
    return total, count, (total / count[:, None].astype(np.float32)).astype(np.float32)


class Scene(object):
    def __init__(self, xyz_origin, superpoint, scale=50, n_superpoints=None):
        self.xyz = np.ascontiguousarray(xyz_origin, dtype=np.float32).reshape(-1, 3)
        self.superpoint = np.asarray(superpoint).astype(np.int64).reshape(-1)
        self.S = int(self.superpoint.max()) + 1 if n_superpoints is None else int(n_superpoints)
        self.N, self.scale = len(self.xyz), scale
        self.sum, self.count, self.centre = sp_stats(self.xyz, self.superpoint, self.S)


def is1ins_of(edges, ins):
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    a, b = ins[edges[:, 0]], ins[edges[:, 1]]
    return np.where((a == NONE) | (b == NONE), 0, np.where(a == b, -1, 1)).astype(np.int64)


def neighbor_source(edges, sem, ins, pred, conf=None, thr=0.8):
    """src int64 [S]: the largest qualifying labelled neighbour of every unlabelled superpoint, or -1; also the number
    of DISTINCT instance labels among the qualifying neighbours (coverage of the largest-id rule)"""
    S = len(sem)
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    k = np.concatenate([edges[:, 0], edges[:, 1]])
    n = np.concatenate([edges[:, 1], edges[:, 0]])
    ok = labelled(sem, ins)[k] & (sem[n] == NONE) & (ins[n] == NONE) & (sem[k] == np.asarray(pred)[n])
    if conf is not None:
        ok &= np.asarray(conf)[n].astype(np.float64) > thr
    src = np.full(S, -1, dtype=np.int64)
    np.maximum.at(src, n[ok], k[ok])
    pairs = np.unique(np.stack([n[ok], ins[k[ok]]], 1), axis=0) if ok.any() else np.zeros((0, 2), np.int64)
    return src, np.bincount(pairs[:, 0], minlength=S)


def apply_source(src, sem, ins, off, centre, edges):
    """-> (sem, ins, off fp64, is1ins) after every i with src[i] >= 0 took labels and instance centre of src[i]"""
    src = np.asarray(src, dtype=np.int64)
    take = src >= 0
    k = np.where(take, src, 0)
    c = centre.astype(np.float64)
    sem2, ins2 = np.where(take, sem[k], sem), np.where(take, ins[k], ins)
    off2 = np.where(take[:, None], (c[k] + off[k]) - c, off)
    return sem2, ins2, off2, is1ins_of(edges, ins2)


def norm3(d):
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


def whole_scene(sem, ins, off, centre, total, count, pred, pred_off, max_dist=0.9):
    """-> dict: sem, ins, off (fp64), prior ids [P], assigned (index into prior or -1) [S], dist (fp64, +inf without a
    candidate), second (distance of the nearest candidate whose instance centre differs from the chosen one's, +inf if
    none), candidates (number of priors of the predicted class) [S]"""
    S = len(sem)
    lab = labelled(sem, ins)
    prior = np.nonzero(lab)[0]
    c = centre[prior].astype(np.float64) + off[prior]
    q = (centre + np.asarray(pred_off, dtype=np.float32)).astype(np.float32).astype(np.float64)
    assigned = np.full(S, -1, dtype=np.int64)
    dist = np.full(S, np.inf)
    second = np.full(S, np.inf)
    candidates = np.zeros(S, dtype=np.int64)
    open_ = np.nonzero(~lab)[0]
    if len(prior) and len(open_):
        d = norm3(c[None, :, :] - q[open_][:, None, :])
        match = sem[prior][None, :] == np.asarray(pred)[open_][:, None]
        d = np.where(match, d, np.inf)
        best = np.argmin(d, axis=1)                                 # the first of equal distances
        dmin = d[np.arange(len(open_)), best]
        has = match.any(1)
        dist[open_] = np.where(has, dmin, np.inf)
        candidates[open_] = match.sum(1)
        same_centre = (c[None, :, :] == c[best][:, None, :]).all(2)
        second[open_] = np.where(same_centre, np.inf, d).min(1)
        ok = has & ~(dmin > max_dist)
        assigned[open_[ok]] = best[ok]
    sem2, ins2, off2 = sem.copy(), ins.copy(), np.array(off, dtype=np.float64, copy=True)
    ids = np.nonzero(assigned >= 0)[0]                              # ascending
    if len(ids):
        g = np.zeros((len(prior), 3))
        np.add.at(g, assigned[ids], total[ids].astype(np.float64))  # unbuffered: added one by one in ascending id
        n = np.zeros(len(prior), dtype=np.int64)
        np.add.at(n, assigned[ids], np.asarray(count, dtype=np.int64)[ids])
        with np.errstate(invalid="ignore", divide="ignore"):
            g = g / n[:, None].astype(np.float64)
        sem2[ids], ins2[ids] = sem[prior[assigned[ids]]], ins[prior[assigned[ids]]]
        off2[ids] = g[assigned[ids]] - centre[ids].astype(np.float64)
    return dict(sem=sem2, ins=ins2, off=off2, prior=prior, assigned=assigned, dist=dist, second=second,
                candidates=candidates)


def whole_scene_margin(res, max_dist):
    """smallest |d_min - max_dist| over the decisions taken and smallest gap between the nearest and the next distinct
    candidate -- what a test asserts to be > GAP before it compares discrete results"""
    has = np.isfinite(res["dist"])
    m1 = float(np.abs(res["dist"][has] - max_dist).min()) if has.any() else np.inf
    two = has & np.isfinite(res["second"])
    m2 = float((res["second"][two] - res["dist"][two]).min()) if two.any() else np.inf
    return m1, m2


def point_labels(superpoint, sem, ins):
    lab = labelled(sem, ins)[superpoint]
    return (np.where(lab, sem[superpoint], NONE).astype(np.float64),
            np.where(lab, ins[superpoint], NONE).astype(np.float64))


def voxels_of(xyz, scale):
    """trunc(float32(xyz) * float32(scale)): the product is an fp32 one, the conversion truncates toward zero"""
    return np.trunc(np.asarray(xyz, dtype=np.float32) * np.float32(scale)).astype(np.int64)


def occupancy(xyz, superpoint, sem, ins, scale=50):
    """instance_voxel_num int64 [S]: distinct voxels among the points carrying the vertex's instance label"""
    carried = np.where(labelled(sem, ins), ins, NONE)
    labels, rank_sp = np.unique(carried, return_inverse=True)
    keys = np.concatenate([rank_sp.reshape(-1)[superpoint][:, None], voxels_of(xyz, scale)], 1)
    per_rank = np.bincount(np.unique(keys, axis=0)[:, 0], minlength=len(labels))
    pos = np.minimum(np.searchsorted(labels, ins), len(labels) - 1)
    return np.where(labels[pos] == ins, per_rank[pos], 0).astype(np.int64)


def instance_size(ins, off):
    labels, rank = np.unique(np.asarray(ins).astype(np.int64), return_inverse=True)
    r = np.zeros(len(labels))
    np.maximum.at(r, rank.reshape(-1), norm3(np.asarray(off, dtype=np.float64)))
    return r[rank.reshape(-1)]


def statistics(weak_sem, weak_ins, sem_gt, ins_gt, stuff=(0, 1)):
    ws, wi, gs, gi = (np.asarray(a, dtype=np.float64) for a in (weak_sem, weak_ins, sem_gt, ins_gt))
    is_stuff = np.isin(ws, np.asarray(stuff, dtype=np.float64))
    has_sem, has_ins = ws != NONE, (wi != NONE) & ~is_stuff
    vals = (len(ws), (gs != NONE).sum(), has_sem.sum(), (has_sem & (ws == gs)).sum(), (has_sem & is_stuff).sum(),
            (has_sem & (ws == gs) & is_stuff).sum(), has_ins.sum(), (has_ins & (wi == gi)).sum())
    return {k: int(v) for k, v in zip(STAT_NAMES, vals)}


# ---- the interface of wsis_weak_labels on PlainGraph objects ---------------------------------------------------------

def _arrays(graph):
    return (np.asarray(graph.vs["semantic_label"]).astype(np.int64), np.asarray(graph.vs["instance_label"]).astype(np.int64),
            np.asarray(graph.vs["superpoint_offset_vector"], dtype=np.float64).reshape(-1, 3))


def _rewritten(graph, sem, ins, off, is1ins=None):
    out = graph.copy()
    out.vs["semantic_label"], out.vs["instance_label"], out.vs["superpoint_offset_vector"] = sem, ins, off
    if is1ins is not None:
        out.is1ins = is1ins
    return out


def extend_label_to_neighbor(scene, graph, conf, pred, thr=0.8):
    sem, ins, off = _arrays(graph)
    src, _ = neighbor_source(graph.edges, sem, ins, pred, conf, thr)
    return _rewritten(graph, *apply_source(src, sem, ins, off, scene.centre, graph.edges))


def propagate_label_to_neighbor(scene, graph, pred):
    sem, ins, off = _arrays(graph)
    src, _ = neighbor_source(graph.edges, sem, ins, pred)
    return _rewritten(graph, *apply_source(src, sem, ins, off, scene.centre, graph.edges))


def apply_propagated_labels(scene, graph, pseudo_label_final):
    sem, ins, off = _arrays(graph)
    plf = np.asarray(pseudo_label_final)
    src = np.where(plf != NONE, plf, -1).astype(np.int64)
    return _rewritten(graph, *apply_source(src, sem, ins, off, scene.centre, graph.edges))


def propagate_label_to_whole_scene(scene, graph, pred, pred_off, max_dist=0.9, return_info=False):
    sem, ins, off = _arrays(graph)
    res = whole_scene(sem, ins, off, scene.centre, scene.sum, scene.count, pred, pred_off, max_dist)
    out = _rewritten(graph, res["sem"], res["ins"], res["off"])
    return (out, res) if return_info else out


def generate_point_level_weak_label(scene, graph, add_occupancy_signal=False, add_instance_size_signal=False):
    sem, ins, off = _arrays(graph)
    graph.vs["instance_voxel_num"] = (occupancy(scene.xyz, scene.superpoint, sem, ins, scene.scale)
                                      if add_occupancy_signal else np.zeros(scene.S, np.int64))
    graph.vs["instance_size"] = instance_size(ins, off) if add_instance_size_signal else np.zeros(scene.S)
    return point_labels(scene.superpoint, sem, ins)
