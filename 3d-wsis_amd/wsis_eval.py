"""Evaluation on the device: instance AP, S3DIS coverage / precision / recall and semantic IoU -- the per-scene stage
of the reference's ``test_scannetv2.py:133-143, 212-275``, ``test_s3dis.py:135-148, 216-292`` and ``do_validation``
(``train_scannetv2.py:296-400``) that turns predictions into AP / AP50 / AP25, mCov / mWCov / mPrec / mRec and mIoU.

The reference's evaluators (``evaluation/basic/ins_seg_evaluator.py``, ``utils/eval_s3dis.py``,
``evaluation/basic/sem_seg_evaluator.py``) form one boolean mask per (prediction, ground-truth instance) pair on the
host.  All three reduce to integer counting over the points followed by arithmetic on tables with a few hundred entries:

  InstanceEvaluator         T[p, u] = #{i : mask[p, i] != 0 and gt_ids[i] == id_u}        wsis_mask_overlap
  S3DISInstanceEvaluator    the same table against ins_gt + the (instance, class) histogram  wsis_mask_overlap, wsis_label_pairs
  SemanticEvaluator         the confusion matrix, np.add.at(confusion, (gt, pred), 1)        wsis_label_pairs

``process`` maps ids to columns, runs the kernels on the current stream, reads the small tables back and hands them to
the host-only ``add_counts``, which holds the reference's expressions.  Per-point data never returns to the host.  The
counts are exact integers; the metrics are the reference's fp64 expressions on them.  The evaluators return values
instead of log lines; reading ground-truth files is the caller's business.
"""
import warnings

import numpy as np

import wsis_native as _n

MASK_OVERLAP_MAX_G = 4096         # distinct ground-truth ids per wsis_mask_overlap call
LABEL_PAIRS_MAX = 65536           # A * B of wsis_label_pairs


def mask_overlap_chunk():
    """points a workgroup of wsis_mask_overlap owns"""
    return int(_n.hip().wsis_mask_overlap_chunk())


def mask_overlap_tile_rows(G):
    """mask rows per workgroup of wsis_mask_overlap for ``G`` columns"""
    r = int(_n.hip().wsis_mask_overlap_tile_rows(int(G)))
    if r < 0:
        raise ValueError(f"mask_overlap: G={G} outside [1, {MASK_OVERLAP_MAX_G}]")
    return r


def _device(device):
    import torch
    dev = torch.device(device)
    if dev.type != "cuda" or not torch.cuda.is_available():
        raise _n.WsisError("the evaluators count on the MI355X (there is no CPU fallback); add_counts takes host tables")
    return dev


def _to_device(x, dev, dtype=None):
    import torch
    t = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))
    t = t.to(dev)
    return t if dtype is None or t.dtype == dtype else t.to(dtype)


def _masks_on_device(masks, dev):
    """[P, N] masks as a contiguous uint8 or int64 device tensor (bool is reinterpreted; other dtypes are compared != 0)"""
    import torch
    t = _to_device(masks, dev)
    if t.dim() != 2:
        raise ValueError("masks must be [P, N]")
    if t.dtype == torch.bool:
        t = t.contiguous().view(torch.uint8)
    elif t.dtype not in (torch.uint8, torch.int64):
        t = (t != 0).to(torch.uint8)
    return t.contiguous()


def mask_overlap(masks, col, G, out=None):
    """wsis_mask_overlap: ``masks`` uint8 / int64 [P, N] and ``col`` int32 [N] on the device ->
    (table int64 [P, G], rows int64 [P]) on the device.  ``out`` = (table, rows): caller-owned buffers."""
    import torch
    _n.require_cuda(masks, col)
    if masks.dim() != 2 or masks.dtype not in (torch.uint8, torch.int64) or col.dtype != torch.int32 \
            or col.numel() != masks.shape[1]:
        raise ValueError("mask_overlap wants masks uint8 / int64 [P, N] and col int32 [N]")
    masks, col = masks.contiguous(), col.contiguous()
    P, N, G = int(masks.shape[0]), int(masks.shape[1]), int(G)
    if out is None:
        out = (torch.empty((P, max(G, 0)), dtype=torch.int64, device=masks.device),
               torch.empty(P, dtype=torch.int64, device=masks.device))
    table, rows = out
    _n.require_cuda(table, rows)
    assert table.dtype == torch.int64 and rows.dtype == torch.int64 and table.is_contiguous() and rows.is_contiguous() \
        and table.numel() >= P * max(G, 0) and rows.numel() >= P
    with torch.cuda.device(masks.device):
        _n.check(_n.hip().wsis_mask_overlap(_n.ptr(masks), masks.element_size(), P, N, _n.ptr(col), G, _n.ptr(table),
                                            _n.ptr(rows), None, 0, _n.stream_ptr()), "mask_overlap")
    return table, rows


def label_pairs(a, b, A, B, out=None):
    """wsis_label_pairs: ``a``, ``b`` int32 [N] on the device -> int64 [A, B] counts of the pairs inside the table
    (``out``: a caller-owned buffer)"""
    import torch
    _n.require_cuda(a, b)
    if a.dtype != torch.int32 or b.dtype != torch.int32 or a.numel() != b.numel():
        raise ValueError("label_pairs wants two int32 arrays of one length")
    a, b = a.contiguous(), b.contiguous()
    A, B = int(A), int(B)
    table = torch.empty((max(A, 0), max(B, 0)), dtype=torch.int64, device=a.device) if out is None else out
    _n.require_cuda(table)
    assert table.dtype == torch.int64 and table.is_contiguous() and table.numel() >= max(A, 0) * max(B, 0)
    with torch.cuda.device(a.device):
        _n.check(_n.hip().wsis_label_pairs(_n.ptr(a), _n.ptr(b), int(a.numel()), A, B, _n.ptr(table), _n.stream_ptr()),
                 "label_pairs")
    return table


def _id_columns(ids, dev):
    """distinct ids ascending (host int64 [U]), their counts (host int64 [U]), column of every point (device int32 [N])"""
    import torch
    t = _to_device(ids, dev).reshape(-1)
    if t.is_floating_point():
        t = t.to(torch.int64)         # np.loadtxt hands the reference float64 ids; they are integers
    uniq, inverse, counts = torch.unique(t, sorted=True, return_inverse=True, return_counts=True)
    if int(uniq.numel()) > MASK_OVERLAP_MAX_G:
        raise ValueError(f"{int(uniq.numel())} distinct ground-truth ids: more than {MASK_OVERLAP_MAX_G}")
    return uniq.cpu().numpy().astype(np.int64), counts.cpu().numpy().astype(np.int64), inverse.to(torch.int32)


# ---- semantic IoU: evaluation/basic/sem_seg_evaluator.py ---------------------------------------------------------

# evaluation/scannet_evaluator.py:10-16, evaluation/s3dis_evaluator.py:9-14
SCANNET_CLASS_LABELS = ("wall", "floor", "cabinet", "bed", "chair", "sofa", "table", "door", "window", "bookshelf",
                        "picture", "counter", "desk", "curtain", "refrigerator", "shower curtain", "toilet", "sink",
                        "bathtub", "otherfurniture")
SCANNET_CLASS_IDS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39)     # inference.SEMANTIC_IND2LABEL
SCANNET_INSTANCE_CLASS_LABELS = SCANNET_CLASS_LABELS[2:]                                        # scannet_evaluator.py:59-65
SCANNET_INSTANCE_CLASS_IDS = SCANNET_CLASS_IDS[2:]                                              # inference.INSTANCE_VALID_LABELS
S3DIS_CLASS_LABELS = ("ceiling", "floor", "wall", "beam", "column", "window", "door", "table", "chair", "sofa",
                      "bookcase", "board", "clutter")
S3DIS_CLASS_IDS = tuple(range(13))
S3DIS_INSTANCE_CLASS_IDS = tuple(range(1, 14))                                                  # s3dis_evaluator.py:16


class SemanticEvaluator(object):
    """``SemanticEvaluator`` of sem_seg_evaluator.py.  ``confusion[gt, pred]`` is int64 [max_id + 2, max_id + 2]."""

    def __init__(self, class_ids, class_labels, ignore=()):
        self.class_ids = np.asarray(class_ids, dtype=np.int64)
        self.class_labels = list(class_labels)
        if len(self.class_ids) != len(self.class_labels) or len(self.class_ids) == 0:
            raise ValueError("class_ids and class_labels must have one (non-zero) length")
        self.ignore = tuple(ignore)
        self.include = [int(i) for i in self.class_ids if i not in self.ignore]
        self.size = int(self.class_ids.max()) + 2
        if self.size * self.size > LABEL_PAIRS_MAX:
            raise ValueError(f"confusion matrix of {self.size}^2 entries: more than {LABEL_PAIRS_MAX}")
        self.reset()

    @classmethod
    def scannet(cls, ignore=()):
        return cls(SCANNET_CLASS_IDS, SCANNET_CLASS_LABELS, ignore)

    @classmethod
    def s3dis(cls, ignore=()):
        return cls(S3DIS_CLASS_IDS, S3DIS_CLASS_LABELS, ignore)

    def reset(self):
        self.confusion = np.zeros((self.size, self.size), dtype=np.int64)

    def add_counts(self, table, n_points=None):
        """``table`` int64 [size, size]: the scene's (gt, pred) counts.  With ``n_points`` the table must hold every
        point: an id outside the matrix (numpy would wrap a negative one, the reference raises beyond it) is an error."""
        table = np.asarray(table)
        if table.shape != self.confusion.shape or table.dtype.kind not in "iu" or (table < 0).any():
            raise ValueError(f"the table must be a non-negative integer array of shape {self.confusion.shape}")
        if n_points is not None and int(table.sum()) != int(n_points):
            raise ValueError(f"{int(n_points) - int(table.sum())} of {int(n_points)} points carry an id outside "
                             f"[0, {self.size})")
        self.confusion += table.astype(np.int64)

    def process(self, pred_ids, gt_ids, device="cuda"):
        """``pred_ids`` / ``gt_ids``: numpy arrays or tensors of ids in the matrix's index space (ScanNet: after
        ``class_ids[pred]``, scannet_evaluator.py:48)"""
        import torch
        dev = _device(device)
        pred = _to_device(pred_ids, dev, torch.int32).reshape(-1)
        gt = _to_device(gt_ids, dev, torch.int32).reshape(-1)
        if pred.numel() != gt.numel():
            raise ValueError("pred_ids and gt_ids differ in length")
        table = label_pairs(gt, pred, self.size, self.size)
        self.add_counts(table.cpu().numpy(), int(gt.numel()))

    def iou(self):
        """prase_iou + the IoU lines of print_result -> dict(tp, fp, fn, union, ious [size] in percent, mean)"""
        conf = np.zeros_like(self.confusion)
        inc = np.asarray(self.include, dtype=np.int64)
        if len(inc):
            conf[np.ix_(inc, inc)] = self.confusion[np.ix_(inc, inc)]
        tp = conf.diagonal().copy()
        fp = conf.sum(axis=1) - tp
        fn = conf.sum(axis=0) - tp
        union = np.maximum(tp + fp + fn, 1)
        ious = (tp / union) * 100
        mean = float(np.nanmean(ious[inc])) if len(inc) else float("nan")
        return dict(tp=tp, fp=fp, fn=fn, union=union, ious=ious, mean=mean)


# ---- instance AP: evaluation/basic/ins_seg_evaluator.py ----------------------------------------------------------

class InstanceEvaluator(object):
    """``InstanceEvaluator`` of ins_seg_evaluator.py (``assign`` + ``evaluate_matches``)."""

    OVERLAPS = np.append(np.arange(0.5, 0.95, 0.05), 0.25)
    MIN_REGION_SIZE = 100

    def __init__(self, class_ids, class_labels):
        self.class_ids = np.asarray(class_ids, dtype=np.int64)
        self.class_labels = list(class_labels)
        if len(self.class_ids) != len(self.class_labels):
            raise ValueError("class_ids and class_labels differ in length")
        self._class_index = {int(c): i for i, c in enumerate(self.class_ids)}
        self.reset()

    @classmethod
    def scannet(cls):
        return cls(SCANNET_INSTANCE_CLASS_IDS, SCANNET_INSTANCE_CLASS_LABELS)

    @classmethod
    def s3dis(cls):
        return cls(S3DIS_INSTANCE_CLASS_IDS, S3DIS_CLASS_LABELS)

    def reset(self):
        self.scenes = {}              # scene name -> the small arrays of add_counts, in order of first arrival
        self.ap_scores = np.zeros((1, len(self.class_labels), len(self.OVERLAPS)))
        self.avgs = {}

    def add_counts(self, scene_name, conf, label_id, pred_size, gt_id, gt_size, table):
        """One scene from its counts.  ``conf`` / ``label_id`` / ``pred_size`` [P]: every prediction with its member
        count; ``gt_id`` / ``gt_size`` [U]: the distinct values of the scene's gt_ids, ascending, with their counts;
        ``table`` int [P, U]: members of prediction p that carry gt id u.  Keeps what assign_instances_for_scan keeps."""
        conf = np.asarray(conf, dtype=np.float64).reshape(-1)
        label_id = np.asarray(label_id).astype(np.int64).reshape(-1)
        pred_size = np.asarray(pred_size).astype(np.int64).reshape(-1)
        gt_id = np.asarray(gt_id).astype(np.int64).reshape(-1)
        gt_size = np.asarray(gt_size).astype(np.int64).reshape(-1)
        table = np.asarray(table)
        P, U = len(label_id), len(gt_id)
        if table.dtype.kind not in "iu":
            raise ValueError("the overlap table must hold integers")
        table = table.astype(np.int64).reshape(P, U)
        if len(conf) != P or len(pred_size) != P or len(gt_size) != U:
            raise ValueError("the arrays of a scene disagree in length")
        if (np.diff(gt_id) <= 0).any():
            raise ValueError("gt_id must be the distinct ids in ascending order")
        if (table < 0).any() or (table.sum(1) > pred_size).any() or (table > gt_size[None, :]).any():
            raise ValueError("the overlap table exceeds the sizes it comes with")
        is_class = np.isin(gt_id // 1000, self.class_ids)
        void_col = ~is_class                                            # ids 0, negative ids, ids of other classes
        inst_col = np.nonzero(is_class & (gt_id > 0))[0]                # VertInstance.get_instances: ascending ids
        keep = np.nonzero(np.isin(label_id, self.class_ids) & (pred_size >= self.MIN_REGION_SIZE))[0]
        cls_of = np.vectorize(self._class_index.get, otypes=[np.int64])
        gt_cls = cls_of(gt_id[inst_col] // 1000) if len(inst_col) else np.zeros(0, np.int64)
        pred_cls = cls_of(label_id[keep]) if len(keep) else np.zeros(0, np.int64)
        inter = table[np.ix_(keep, inst_col)] * (pred_cls[:, None] == gt_cls[None, :])
        ip, ig = np.nonzero(inter)                                      # row-major: prediction order, then id order
        self.scenes[scene_name] = dict(
            pred_cls=pred_cls, pred_conf=conf[keep], pred_size=pred_size[keep],
            pred_void=table[keep][:, void_col].sum(1), gt_id=gt_id[inst_col], gt_size=gt_size[inst_col], gt_cls=gt_cls,
            inter_pred=ip.astype(np.int64), inter_gt=ig.astype(np.int64), inter=inter[ip, ig])

    def process(self, scene_name, conf, label_id, masks, gt_ids, device="cuda"):
        """``masks`` [P, N] (bool / uint8 / int64, numpy or tensor; a member is an element != 0), ``gt_ids`` [N] =
        class_id * 1000 + k.  ``conf`` and ``label_id`` [P] are small host arrays."""
        dev = _device(device)
        m = _masks_on_device(masks, dev) if np.size(label_id) else None
        gt_id, gt_size, col = _id_columns(gt_ids, dev)
        if m is None:
            table, rows = np.zeros((0, len(gt_id)), np.int64), np.zeros(0, np.int64)
        else:
            if m.shape[1] != col.numel():
                raise ValueError(f"masks of {m.shape[1]} points against {col.numel()} ground-truth ids")
            if len(gt_id) == 0:
                raise ValueError("a scene without points")
            table, rows = (t.cpu().numpy() for t in mask_overlap(m, col, len(gt_id)))
        self.add_counts(scene_name, conf, label_id, rows, gt_id, gt_size, table)

    def _scene_class(self, sc, li, overlap_th, visited):
        """y_true, y_score, hard false negatives, has_gt, has_pred of one scene and class at one threshold"""
        preds = np.nonzero(sc["pred_cls"] == li)[0]
        gts_all = np.nonzero(sc["gt_cls"] == li)[0]
        gts = gts_all[sc["gt_size"][gts_all] >= self.MIN_REGION_SIZE]
        K, M = len(sc["pred_cls"]), len(sc["gt_id"])
        inter = np.zeros((K, M), dtype=np.int64)
        inter[sc["inter_pred"], sc["inter_gt"]] = sc["inter"]
        psize, gsize, pconf = sc["pred_size"], sc["gt_size"], sc["pred_conf"]

        def overlap(p, g):
            return float(inter[p, g]) / (gsize[g] + psize[p] - inter[p, g])

        true, score, hard_fn = [], [], 0
        extra_score = []                                               # second matches on one ground truth
        for g in gts:
            best = None
            for p in preds[inter[preds, g] > 0]:                       # matched_pred, in prediction order
                if visited[p]:
                    continue
                if overlap(p, g) > overlap_th:
                    if best is None:
                        best = pconf[p]
                        visited[p] = True
                    else:                                              # the lower score is a false positive
                        extra_score.append(min(best, pconf[p]))
                        best = max(best, pconf[p])
            if best is None:
                hard_fn += 1
            else:
                true.append(1.0)
                score.append(best)
        true += [0.0] * len(extra_score)
        score += extra_score
        for p in preds:                                                # unmatched predictions
            matched = gts_all[inter[p, gts_all] > 0]
            if any(overlap(p, g) > overlap_th for g in matched):
                continue
            n_ignore = int(sc["pred_void"][p])
            for g in matched:
                if sc["gt_id"][g] < 1000:                              # group
                    n_ignore += int(inter[p, g])
                if gsize[g] < self.MIN_REGION_SIZE:                    # small ground-truth instance
                    n_ignore += int(inter[p, g])
            if float(n_ignore) / psize[p] <= overlap_th:
                true.append(0.0)
                score.append(pconf[p])
        return true, score, hard_fn, len(gts) > 0, len(preds) > 0

    @staticmethod
    def _average_precision(y_true, y_score, hard_fn):
        """area under the precision-recall curve over the unique scores, ins_seg_evaluator.py:272-323"""
        order = np.argsort(y_score, kind="stable")
        y_score, y_true = y_score[order], y_true[order]
        cum = np.cumsum(y_true)
        _, first = np.unique(y_score, return_index=True)
        n, n_true = len(y_score), (cum[-1] if len(cum) else 0)
        below = np.where(first > 0, cum[np.maximum(first, 1) - 1], 0.0) if len(first) else np.zeros(0)
        tp = n_true - below                                            # true positives at scores >= the threshold
        fp = n - first - tp
        fn = below + hard_fn
        precision = np.append(tp / (tp + fp), 1.0)
        recall = np.append(tp / (tp + fn), 0.0)
        padded = np.concatenate([recall[:1], recall, [0.0]])
        return float(np.dot(precision, np.convolve(padded, [-0.5, 0, 0.5], "valid")))

    def evaluate(self):
        """evaluate_matches -> dict(ap_scores [1, C, 10], all_ap, all_ap_50%, all_ap_25%, classes {label: {ap, ap50%,
        ap25%}}); a class without ground truth is nan, one with ground truth and no prediction 0"""
        for oi, overlap_th in enumerate(self.OVERLAPS):
            visited = {name: np.zeros(len(sc["pred_cls"]), dtype=bool) for name, sc in self.scenes.items()}
            for li in range(len(self.class_labels)):
                y_true, y_score, hard_fn, has_gt, has_pred = [], [], 0, False, False
                for name, sc in self.scenes.items():
                    t, s, h, g, p = self._scene_class(sc, li, overlap_th, visited[name])
                    y_true += t
                    y_score += s
                    hard_fn += h
                    has_gt |= g
                    has_pred |= p
                if has_gt and has_pred:
                    ap = self._average_precision(np.asarray(y_true, np.float64), np.asarray(y_score, np.float64), hard_fn)
                elif has_gt:
                    ap = 0.0
                else:
                    ap = float("nan")
                self.ap_scores[0, li, oi] = ap
        o50 = np.isclose(self.OVERLAPS, 0.5)
        o25 = np.isclose(self.OVERLAPS, 0.25)
        rest = ~o25
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)            # nanmean of an all-nan slice is nan
            by_overlap = np.ascontiguousarray(self.ap_scores[0].T)    # [overlap, class]: the reference's order of additions
            self.avgs = {"all_ap": np.nanmean(by_overlap[rest]), "all_ap_50%": np.nanmean(by_overlap[o50]),
                         "all_ap_25%": np.nanmean(by_overlap[o25]), "classes": {}}
        for li, label in enumerate(self.class_labels):
            self.avgs["classes"][label] = {"ap": np.average(self.ap_scores[0, li, rest]),
                                           "ap50%": np.average(self.ap_scores[0, li, o50]),
                                           "ap25%": np.average(self.ap_scores[0, li, o25])}
        return dict(self.avgs, ap_scores=self.ap_scores.copy())


# ---- S3DIS coverage / precision / recall: utils/eval_s3dis.py ----------------------------------------------------

class S3DISInstanceEvaluator(object):
    """``S3DIS_Instance_evaluator`` of utils/eval_s3dis.py."""

    def __init__(self, num_classes=13, iou_threshold=0.5):
        self.num_classes = int(num_classes)
        self.iou_threshold = float(iou_threshold)
        self.reset()

    def reset(self):
        C = self.num_classes
        self.total_gt_ins = np.zeros(C)
        self.tp = [[] for _ in range(C)]
        self.fp = [[] for _ in range(C)]
        self.all_mean_cov = [[] for _ in range(C)]
        self.all_mean_weighted_cov = [[] for _ in range(C)]

    def add_counts(self, sem_label, pred_size, gt_size, gt_class_hist, table):
        """One scene from its counts.  ``sem_label`` / ``pred_size`` [P]: every prediction (labels 1 .. num_classes) with
        its member count; ``gt_size`` [U]: the sizes of the distinct values of ins_gt, ascending by id;
        ``gt_class_hist`` int [U, num_classes]: points of instance u whose sem_gt is c; ``table`` int [P, U]."""
        C = self.num_classes
        sem_id = np.asarray(sem_label).astype(np.int64).reshape(-1) - 1
        pred_size = np.asarray(pred_size).astype(np.int64).reshape(-1)
        gt_size = np.asarray(gt_size).astype(np.int64).reshape(-1)
        hist, table = np.asarray(gt_class_hist), np.asarray(table)
        P, U = len(sem_id), len(gt_size)
        if hist.dtype.kind not in "iu" or table.dtype.kind not in "iu":
            raise ValueError("the tables must hold integers")
        hist, table = hist.astype(np.int64).reshape(U, C), table.astype(np.int64).reshape(P, U)
        if len(pred_size) != P:
            raise ValueError("the arrays of a scene disagree in length")
        if ((sem_id < 0) | (sem_id >= C)).any():
            raise ValueError(f"sem_label outside [1, {C}]")
        if (hist < 0).any() or (hist.sum(1) != gt_size).any() or (gt_size <= 0).any():
            raise ValueError(f"a ground-truth instance has points whose sem_gt is outside [0, {C})")
        if (table < 0).any() or (table.sum(1) > pred_size).any() or (table > gt_size[None, :]).any():
            raise ValueError("the overlap table exceeds the sizes it comes with")
        gt_cls = hist.argmax(1) if U else np.zeros(0, np.int64)        # the mode; argmax returns the smallest among ties
        union = gt_size[None, :] + pred_size[:, None] - table
        with np.errstate(divide="ignore", invalid="ignore"):
            iou = table.astype(np.float64) / union                    # int / int in fp64, as float(sum) / sum
        for c in range(C):
            preds, gts = np.nonzero(sem_id == c)[0], np.nonzero(gt_cls == c)[0]
            sum_cov, weighted, n_all = 0, 0, 0
            for g in gts:                                              # coverage: the best prediction of every instance
                iou_max = 0.
                for p in preds:
                    iou_max = max(iou_max, iou[p, g])
                n_all += gt_size[g]
                sum_cov += iou_max
                weighted += gt_size[g] * iou_max
            if len(gts):
                self.all_mean_cov[c].append(sum_cov / len(gts))
                self.all_mean_weighted_cov[c].append(weighted / n_all)
            self.total_gt_ins[c] += len(gts)
            for p in preds:                                            # precision / recall: the best instance of every prediction
                iou_max = -1.
                for g in gts:
                    if iou[p, g] > iou_max:                            # strict: the first of equal IoUs stays
                        iou_max = iou[p, g]
                hit = iou_max > self.iou_threshold
                self.tp[c].append(1. if hit else 0.)
                self.fp[c].append(0. if hit else 1.)

    def process(self, conf, sem_label, masks, sem_gt, ins_gt, device="cuda"):
        """``conf`` is accepted for the reference's signature; its evaluator never reads it"""
        import torch
        dev = _device(device)
        m = _masks_on_device(masks, dev) if np.size(sem_label) else None
        gt_id, gt_size, col = _id_columns(ins_gt, dev)
        U, C = len(gt_id), self.num_classes
        sem = _to_device(sem_gt, dev).reshape(-1)
        if sem.numel() != col.numel():
            raise ValueError("sem_gt and ins_gt differ in length")
        if U == 0:
            raise ValueError("a scene without points")
        if U * C > LABEL_PAIRS_MAX:
            raise ValueError(f"{U} instances x {C} classes: more than {LABEL_PAIRS_MAX} histogram entries")
        hist = label_pairs(col, sem.to(torch.int32), U, C).cpu().numpy()
        if m is None:
            table, rows = np.zeros((0, U), np.int64), np.zeros(0, np.int64)
        else:
            if m.shape[1] != col.numel():
                raise ValueError(f"masks of {m.shape[1]} points against {col.numel()} ground-truth ids")
            table, rows = (t.cpu().numpy() for t in mask_overlap(m, col, U))
        self.add_counts(sem_label, rows, gt_size, hist, table)

    def evaluate(self):
        """-> dict(MUCov, MWCov, precision, recall [num_classes], mMUCov, mMWCov, mPrecision, mRecall); a class without
        ground truth (coverage, recall) or without predictions (precision) is nan, and so is a mean over such a class"""
        C = self.num_classes
        nan = float("nan")
        MUCov = np.array([np.mean(v) if v else nan for v in self.all_mean_cov])
        MWCov = np.array([np.mean(v) if v else nan for v in self.all_mean_weighted_cov])
        precision, recall = np.zeros(C), np.zeros(C)
        for c in range(C):
            tp, fp = np.sum(np.asarray(self.tp[c], dtype=np.float64)), np.sum(np.asarray(self.fp[c], dtype=np.float64))
            recall[c] = tp / self.total_gt_ins[c] if self.total_gt_ins[c] else nan
            precision[c] = tp / (tp + fp) if tp + fp else nan
        return dict(MUCov=MUCov, MWCov=MWCov, precision=precision, recall=recall, mMUCov=np.mean(MUCov),
                    mMWCov=np.mean(MWCov), mPrecision=np.mean(precision), mRecall=np.mean(recall))
