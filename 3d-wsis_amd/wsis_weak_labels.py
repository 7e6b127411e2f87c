"""The dataset's label rewrites between the three training stages, on the device: drop-ins for the methods of
``ScanNetV2Inst_spg`` (``modules/datasets/scannetv2_dataset.py``; ``s3dis_dataset.py`` has the same ones) that
``train_scannetv2.py:477-480, 575-577, 664-666`` calls at the stage boundaries.

    scene = WeakLabelScene(xyz_origin, superpoint)                    once per scene: upload, point CSR, centres
    extend_label_to_neighbor(scene, graph, conf, pred)                :780-818    semantic -> propagation
    propagate_label_to_neighbor(scene, weak_graph, pred)              :823-865    (the same without the confidence test)
    apply_propagated_labels(scene, graph, pseudo_label_final)         :739-772    after wsis_ops.weak_label_propagation
    propagate_label_to_whole_scene(scene, graph, pred, pred_offsets)  :873-964    -> whole-scene pseudo instances
    generate_point_level_weak_label(scene, weak_graph, ...)           :568-595    with cal_occupancy / cal_instance_size
    weak_label_statistics(weak_sem, weak_ins, sem_gt, ins_gt)         :602-640    the eight counters behind the log lines

Graphs are :class:`wsis_datasets.PlainGraph`.  Every stage function returns a NEW graph and leaves its input untouched
(the reference deep-copies the graph and reads the old one while it writes the copy);
``generate_point_level_weak_label`` sets the two regression targets on the graph it is given, as the reference does.

The reference forms one mask ``superpoint == spID`` per superpoint (O(S*N) per scene and call).  Here the per-point
work is one pass each (``csrc/weaklabel.hip``); the graph attributes are small host arrays, uploaded per call, and only
they and the final point-label arrays come back.  There is no CPU fallback: a CPU device raises ``WsisError``.
"""
import ctypes

import numpy as np
import torch

import wsis_native as _n
from torch_scatter import segment_csr

NONE = -100
STAT_NAMES = ("GT_all", "GT_label", "semantic_label_num", "correct_semantic_label_num", "floor_wall_sem_num",
              "floor_wall_correct_sem_num", "instance_label_num", "correct_instance_label_num")


def _cuda_device(device, what):
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _n.WsisError(f"{what} runs on the MI355X (there is no CPU fallback)")
    return dev


class WeakLabelScene(object):
    """What the stage updates need of one scene, uploaded once: ``xyz`` fp32 [N,3], ``superpoint`` int64 [N], the point
    CSR of the superpoints and -- one wave per superpoint, fp32, fixed order -- ``sum`` fp32 [S,3], ``count`` int32 [S]
    and ``centre`` fp32 [S,3] (``xyz_origin[superpoint == spID].mean(0)`` of the reference).  ``scale``: voxels per metre
    of the occupancy count (``self.scale``, config ``data.scale`` = 50).  ``n_superpoints``: S, if the largest id may
    be missing from ``superpoint``.  An id without points raises ``ValueError`` (the reference's centre would be NaN)."""

    def __init__(self, xyz_origin, superpoint, device="cuda", scale=50, n_superpoints=None):
        xyz = np.ascontiguousarray(xyz_origin, dtype=np.float32).reshape(-1, 3)
        sp = np.ascontiguousarray(np.asarray(superpoint).reshape(-1)).astype(np.int64)
        if len(xyz) != len(sp):
            raise ValueError(f"{len(xyz)} points but {len(sp)} superpoint ids")
        if len(sp) and sp.min() < 0:
            raise ValueError("negative superpoint id")
        S = (int(sp.max()) + 1 if len(sp) else 0) if n_superpoints is None else int(n_superpoints)
        if len(sp) and int(sp.max()) >= S:
            raise ValueError(f"superpoint id {int(sp.max())} with {S} superpoints")
        empty = np.nonzero(np.bincount(sp, minlength=S) == 0)[0]
        if len(empty):
            raise ValueError(f"superpoint {int(empty[0])} has no points ({len(empty)} such ids of {S})")
        dev = _cuda_device(device, "WeakLabelScene")
        self.device, self.scale, self.N, self.S = dev, scale, len(sp), S
        with torch.cuda.device(dev):
            self.xyz = torch.from_numpy(xyz).to(dev)
            self.superpoint = torch.from_numpy(sp).to(dev)
            self.csr = segment_csr(self.superpoint, S)
            self.sum = torch.empty((S, 3), dtype=torch.float32, device=dev)
            self.count = torch.empty(S, dtype=torch.int32, device=dev)
            self.centre = torch.empty((S, 3), dtype=torch.float32, device=dev)
            _n.check(_n.hip().wsis_wl_sp_stats(_n.ptr(self.xyz), _n.ptr(self.csr.perm), _n.ptr(self.csr.offsets), self.N, S,
                                               _n.ptr(self.sum), _n.ptr(self.count), _n.ptr(self.centre), _n.stream_ptr()),
                     "wl_sp_stats")


class _DeviceGraph(object):
    """the attributes of a PlainGraph the stages read, as host arrays of fixed dtype and their device copies"""

    def __init__(self, scene, graph):
        if graph.vcount != scene.S:
            raise ValueError(f"the graph has {graph.vcount} vertices, the scene {scene.S} superpoints")
        self.sem_h = np.asarray(graph.vs["semantic_label"]).astype(np.int64).reshape(-1)
        self.ins_h = np.asarray(graph.vs["instance_label"]).astype(np.int64).reshape(-1)
        self.off_h = np.ascontiguousarray(graph.vs["superpoint_offset_vector"], dtype=np.float64).reshape(scene.S, 3)
        self.edges_h = np.ascontiguousarray(graph.edges, dtype=np.int64).reshape(-1, 2)
        if len(self.edges_h) and (self.edges_h.min() < 0 or self.edges_h.max() >= scene.S):
            raise ValueError("edge endpoint outside the graph")
        dev = scene.device
        self.sem, self.ins = torch.from_numpy(self.sem_h).to(dev), torch.from_numpy(self.ins_h).to(dev)
        self.off, self.edges = torch.from_numpy(self.off_h).to(dev), torch.from_numpy(self.edges_h).to(dev)
        self.E = len(self.edges_h)

    @property
    def labelled_h(self):
        return (self.sem_h != NONE) & (self.ins_h != NONE)


def _sp_vector(values, S, dtype, what, width=None):
    a = np.ascontiguousarray(np.asarray(values).reshape((S,) if width is None else (S, width)), dtype=dtype)
    if a.shape[0] != S:
        raise ValueError(f"{what}: expected {S} rows")
    return a


def _rewritten(graph, sem, ins, off, is1ins=None):
    out = graph.copy()
    out.vs["semantic_label"] = sem.cpu().numpy().astype(np.asarray(graph.vs["semantic_label"]).dtype)
    out.vs["instance_label"] = ins.cpu().numpy().astype(np.asarray(graph.vs["instance_label"]).dtype)
    out.vs["superpoint_offset_vector"] = off.cpu().numpy()
    if is1ins is not None:
        out.is1ins = is1ins.cpu().numpy()
    return out


def _apply_source(scene, g, src, graph):
    dev, S = scene.device, scene.S
    sem, ins, off = torch.empty_like(g.sem), torch.empty_like(g.ins), torch.empty_like(g.off)
    is1ins = torch.empty(g.E, dtype=torch.int64, device=dev)
    _n.check(_n.hip().wsis_wl_apply_source(_n.ptr(src), _n.ptr(g.sem), _n.ptr(g.ins), _n.ptr(g.off), _n.ptr(scene.centre),
                                           _n.ptr(g.edges), g.E, S, _n.ptr(sem), _n.ptr(ins), _n.ptr(off), _n.ptr(is1ins),
                                           _n.stream_ptr()), "wl_apply_source")
    return _rewritten(graph, sem, ins, off, is1ins)


def _neighbor_stage(scene, graph, sp_semantic_value, sp_semantic_pred, thr):
    with torch.cuda.device(scene.device):
        g = _DeviceGraph(scene, graph)
        pred = torch.from_numpy(_sp_vector(sp_semantic_pred, scene.S, np.int64, "sp_semantic_pred")).to(scene.device)
        conf = None
        if sp_semantic_value is not None:
            conf = torch.from_numpy(_sp_vector(sp_semantic_value, scene.S, np.float32, "sp_semantic_value")).to(scene.device)
        src = torch.empty(scene.S, dtype=torch.int32, device=scene.device)
        _n.check(_n.hip().wsis_wl_neighbor_source(_n.ptr(g.edges), g.E, _n.ptr(g.sem), _n.ptr(g.ins), _n.ptr(pred),
                                                  _n.ptr(conf), float(thr), scene.S, _n.ptr(src), _n.stream_ptr()),
                 "wl_neighbor_source")
        return _apply_source(scene, g, src, graph)


def extend_label_to_neighbor(scene, graph, sp_semantic_value, sp_semantic_pred, thr=0.8):
    """``extend_label_to_neighbor`` (:780-818): an unlabelled superpoint n next to a labelled k (either edge direction)
    with ``sem[k] == sp_semantic_pred[n]`` and ``float64(sp_semantic_value[n]) > thr`` (fp32 confidences) takes k's two
    labels and the offset to k's instance centre; among several such k the largest id (the reference's last writer).
    ``is1ins`` is recomputed for every edge."""
    if sp_semantic_value is None:
        raise ValueError("extend_label_to_neighbor needs the confidences (propagate_label_to_neighbor does not)")
    return _neighbor_stage(scene, graph, sp_semantic_value, sp_semantic_pred, thr)


def propagate_label_to_neighbor(scene, weak_graph, sp_semantic_pred):
    """``propagate_label_to_neighbor`` (:823-865): the same step on the weak-label graph without the confidence test"""
    return _neighbor_stage(scene, weak_graph, None, sp_semantic_pred, 0.0)


def apply_propagated_labels(scene, graph, pseudo_label_final):
    """The tail of ``weak_label_propagation`` (:739-772): ``pseudo_label_final`` [S] (the first result of
    ``wsis_ops.weak_label_propagation``) names for every superpoint the labelled superpoint it takes labels and
    instance centre from, or -100."""
    plf = np.asarray(pseudo_label_final).reshape(-1)
    if len(plf) != scene.S:
        raise ValueError(f"pseudo_label_final: expected {scene.S} entries")
    src = np.where(plf != NONE, plf, -1).astype(np.int64)
    if len(src) and (src.min() < -1 or src.max() >= scene.S):
        raise ValueError("pseudo_label_final names a superpoint outside the graph")
    with torch.cuda.device(scene.device):
        g = _DeviceGraph(scene, graph)
        return _apply_source(scene, g, torch.from_numpy(src.astype(np.int32)).to(scene.device), graph)


def propagate_label_to_whole_scene(scene, graph, sp_semantic_pred, pred_sp_offset_vectors, max_dist=0.9,
                                   return_info=False):
    """``propagate_label_to_whole_scene`` (:873-964; S3DIS: ``max_dist=1.2``, s3dis_dataset.py:986).  Priors = the
    labelled superpoints in ascending order, each with the instance centre ``centre + offset``.  An unlabelled
    superpoint joins the nearest prior of its predicted class (fp64 distance from ``centre + predicted offset``, first
    index on ties) unless that distance is > ``max_dist``; it gets the prior's labels and the offset to the point mean
    of everything that joined that prior.  Priors and ``is1ins`` stay as they are.
    ``return_info=True`` also returns ``{"prior": ids [P], "assigned": index into prior or -1 [S], "dist": fp64 [S]}``
    (``dist`` = +inf for labelled superpoints and for those without a prior of their class)."""
    S, dev = scene.S, scene.device
    with torch.cuda.device(dev):
        g = _DeviceGraph(scene, graph)
        prior_h = np.nonzero(g.labelled_h)[0].astype(np.int32)
        prior = torch.from_numpy(prior_h).to(dev)
        pred = torch.from_numpy(_sp_vector(sp_semantic_pred, S, np.int64, "sp_semantic_pred")).to(dev)
        pred_off = torch.from_numpy(_sp_vector(pred_sp_offset_vectors, S, np.float32, "pred_sp_offset_vectors", 3)).to(dev)
        sem, ins, off = torch.empty_like(g.sem), torch.empty_like(g.ins), torch.empty_like(g.off)
        assigned = torch.empty(S, dtype=torch.int32, device=dev)
        dist = torch.empty(S, dtype=torch.float64, device=dev)
        _n.check(_n.hip().wsis_wl_scene_assign(_n.ptr(prior), len(prior_h), _n.ptr(g.sem), _n.ptr(g.ins), _n.ptr(g.off),
                                               _n.ptr(scene.centre), _n.ptr(scene.sum), _n.ptr(scene.count), _n.ptr(pred),
                                               _n.ptr(pred_off), float(max_dist), S, _n.ptr(assigned), _n.ptr(dist),
                                               _n.ptr(sem), _n.ptr(ins), _n.ptr(off), _n.stream_ptr()), "wl_scene_assign")
        out = _rewritten(graph, sem, ins, off)
        if return_info:
            return out, {"prior": prior_h.astype(np.int64), "assigned": assigned.cpu().numpy().astype(np.int64),
                         "dist": dist.cpu().numpy()}
        return out


def _ranks(values):
    """-> (sorted distinct values, rank of every entry)"""
    u, inv = np.unique(values, return_inverse=True)
    return u, inv.reshape(-1).astype(np.int32)


def generate_point_level_weak_label(scene, weak_graph, add_occupancy_signal=False, add_instance_size_signal=False):
    """``generate_point_level_weak_label`` (:568-595) for one scene -> (weak_semantic_label, weak_instance_label), fp64
    [N]: the labels of the point's superpoint if it is labelled, else -100.  Sets ``instance_voxel_num`` (int64) and
    ``instance_size`` (fp64) on ``weak_graph``:

    * occupancy (``cal_occupancy`` :515-542): per distinct point-level instance label L, -100 INCLUDED, the number of
      distinct ``trunc(float32(xyz) * scale)`` voxels among the points carrying L; a vertex gets the count of its own
      ``instance_label`` -- every unlabelled vertex therefore the voxel count of all unlabelled points, the
      reference's quirk -- and 0 if no point carries that value;
    * size (``cal_instance_size`` :545-564): the largest ``||offset||`` (fp64) among the vertices sharing
      ``int(instance_label)``, at least 0.

    With a flag off the attribute is all zeros."""
    S, N, dev = scene.S, scene.N, scene.device
    lib = _n.hip()
    with torch.cuda.device(dev):
        g = _DeviceGraph(scene, weak_graph)
        weak_sem = torch.empty(N, dtype=torch.float64, device=dev)
        weak_ins = torch.empty(N, dtype=torch.float64, device=dev)
        _n.check(lib.wsis_wl_point_labels(_n.ptr(scene.superpoint), N, _n.ptr(g.sem), _n.ptr(g.ins), _n.ptr(weak_sem),
                                          _n.ptr(weak_ins), _n.stream_ptr()), "wl_point_labels")
        voxel_num = np.zeros(S, dtype=np.int64)
        if add_occupancy_signal and S:
            carried = np.where(g.labelled_h, g.ins_h, NONE)            # the label the points of a superpoint carry
            labels, rank_sp = _ranks(carried)
            R = len(labels)
            nbytes = int(lib.wsis_wl_occupancy_workspace_bytes(N))
            if nbytes < 0:
                raise _n.WsisError("wl_occupancy workspace query failed")
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            count = torch.empty(R, dtype=torch.int64, device=dev)
            rank_d = torch.from_numpy(rank_sp).to(dev)
            _n.check(lib.wsis_wl_occupancy(_n.ptr(scene.xyz), _n.ptr(scene.superpoint), _n.ptr(rank_d), N, R,
                                           float(np.float32(scene.scale)), _n.ptr(count), _n.ptr(ws), nbytes,
                                           _n.stream_ptr()), "wl_occupancy")
            count_h = count.cpu().numpy()
            del ws
            pos = np.minimum(np.searchsorted(labels, g.ins_h), R - 1)
            voxel_num = np.where(labels[pos] == g.ins_h, count_h[pos], 0).astype(np.int64)
        size = np.zeros(S, dtype=np.float64)
        if add_instance_size_signal and S:
            labels, rank = _ranks(g.ins_h)
            R = len(labels)
            rmax = torch.empty(R, dtype=torch.float64, device=dev)
            size_d = torch.empty(S, dtype=torch.float64, device=dev)
            rank_d = torch.from_numpy(rank).to(dev)
            _n.check(lib.wsis_wl_instance_size(_n.ptr(g.off), _n.ptr(rank_d), S, R, _n.ptr(rmax),
                                               _n.ptr(size_d), _n.stream_ptr()), "wl_instance_size")
            size = size_d.cpu().numpy()
        weak_graph.vs["instance_voxel_num"] = voxel_num
        weak_graph.vs["instance_size"] = size
        return weak_sem.cpu().numpy(), weak_ins.cpu().numpy()


def weak_label_statistics(weak_sem, weak_ins, sem_gt, ins_gt, stuff=(0, 1), device="cuda"):
    """The counters behind the log lines of :602-661 for one scene, in one pass over the points: a dict with the keys
    ``STAT_NAMES`` (Python ints).  The four inputs are [N] label arrays (-100 = none; numpy or device tensors);
    ``stuff``: the "floor & wall" classes (0, 1 in both datasets), which the instance counters leave out."""
    dev = _cuda_device(device, "weak_label_statistics")
    stuff = [float(c) for c in stuff]
    if len(stuff) > 8:
        raise ValueError("at most 8 stuff classes")
    with torch.cuda.device(dev):
        cols = [torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64) if not torch.is_tensor(a) else a)
                .to(dev, torch.float64).reshape(-1).contiguous() for a in (weak_sem, weak_ins, sem_gt, ins_gt)]
        N = int(cols[0].numel())
        if any(int(c.numel()) != N for c in cols):
            raise ValueError("the four label arrays differ in length")
        counters = torch.empty(len(STAT_NAMES), dtype=torch.int64, device=dev)
        h_stuff = (ctypes.c_double * max(len(stuff), 1))(*stuff)
        _n.check(_n.hip().wsis_wl_label_stats(_n.ptr(cols[0]), _n.ptr(cols[1]), _n.ptr(cols[2]), _n.ptr(cols[3]), N,
                                              ctypes.addressof(h_stuff), len(stuff), _n.ptr(counters), _n.stream_ptr()),
                 "wl_label_stats")
        return {k: int(v) for k, v in zip(STAT_NAMES, counters.cpu().tolist())}
