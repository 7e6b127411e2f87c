"""numpy oracle of wsis_eval: the three evaluators of the reference restated in their own mask-per-pair shape (one boolean
mask per prediction and per ground-truth instance, one ``logical_and`` per pair, lists of dicts), written from the
algorithms and independent of wsis_eval's table form.  tests/test_eval_host.py pins it on the results recorded from
the reference itself (tests/golden/eval_golden.npz); the GPU tests and tools/eval_bench.py use it for tables and timing.
"""
import numpy as np

OVERLAPS = np.append(np.arange(0.5, 0.95, 0.05), 0.25)
MIN_REGION = 100


# ---- the two tables ------------------------------------------------------------------------------------------------

def overlap_table(masks, col, G):
    """-> (T int64 [P, G] with T[p, u] = #{i : masks[p, i] != 0 and col[i] == u}, row member counts int64 [P])"""
    masks = np.asarray(masks)
    col = np.asarray(col)
    T = np.zeros((len(masks), G), dtype=np.int64)
    p, i = np.nonzero(masks)
    ok = (col[i] >= 0) & (col[i] < G)
    np.add.at(T, (p[ok], col[i][ok]), 1)
    return T, np.count_nonzero(masks, axis=1).astype(np.int64)


def pair_table(a, b, A, B):
    """-> int64 [A, B] counts of (a_i, b_i) with 0 <= a_i < A and 0 <= b_i < B"""
    a, b = np.asarray(a).astype(np.int64), np.asarray(b).astype(np.int64)
    ok = (a >= 0) & (a < A) & (b >= 0) & (b < B)
    T = np.zeros((A, B), dtype=np.int64)
    np.add.at(T, (a[ok], b[ok]), 1)
    return T


def unpack_masks(bits, N):
    """the fixture's packed masks (np.packbits along the points) -> bool [P, N]"""
    return np.unpackbits(bits, axis=1, count=N).astype(bool)


# ---- semantic IoU ------------------------------------------------------------------------------------------------

def semantic_iou(confusion, include):
    conf = np.zeros_like(confusion)
    for i in include:
        conf[i, include] = confusion[i, include]
    tp = conf.diagonal()
    fp, fn = conf.sum(axis=1) - tp, conf.sum(axis=0) - tp
    union = np.maximum(tp + fp + fn, 1)
    ious = (tp / union) * 100
    return dict(tp=tp, fp=fp, fn=fn, union=union, ious=ious, mean=np.nanmean(ious[include]))


# ---- instance AP -------------------------------------------------------------------------------------------------

def assign_scene(class_ids, conf, label_id, masks, gt_ids):
    """one scene in the reference's shape -> (gt instances per class, kept predictions per class), lists of dicts"""
    class_ids = [int(c) for c in class_ids]
    gt_ids = np.asarray(gt_ids)
    gts = {c: [] for c in class_ids}
    for i in np.unique(gt_ids):
        if i > 0 and int(i // 1000) in gts:
            gts[int(i // 1000)].append(dict(id=int(i), count=int((gt_ids == i).sum()), matched=[]))
    void = ~np.isin(gt_ids // 1000, class_ids)
    preds = {c: [] for c in class_ids}
    for k in range(len(label_id)):
        c = int(label_id[k])
        if c not in preds:
            continue
        mask = np.not_equal(masks[k], 0)
        n = int(np.count_nonzero(mask))
        if n < MIN_REGION:
            continue
        pred = dict(key=sum(len(v) for v in preds.values()), count=n, conf=conf[k],
                    void=int(np.count_nonzero(void & mask)), matched=[])
        for gt in gts[c]:
            inter = int(np.count_nonzero((gt_ids == gt["id"]) & mask))
            if inter > 0:
                pred["matched"].append((gt, inter))
                gt["matched"].append((pred, inter))
        preds[c].append(pred)
    return gts, preds


def scene_counts(class_ids, gts, preds):
    """the integer intermediates of a scene: per kept prediction (in order of appearance) its size and void
    intersection, per ground-truth instance (ascending id) its id and size, and the non-zero intersections as
    (prediction, instance, count) rows"""
    plist = sorted((p for c in class_ids for p in preds[int(c)]), key=lambda p: p["key"])
    glist = sorted((g for c in class_ids for g in gts[int(c)]), key=lambda g: g["id"])
    gpos = {g["id"]: j for j, g in enumerate(glist)}
    inter = [(p["key"], gpos[g["id"]], n) for p in plist for g, n in p["matched"]]
    return dict(pred_size=np.array([p["count"] for p in plist], dtype=np.int64),
                pred_void=np.array([p["void"] for p in plist], dtype=np.int64),
                gt_id=np.array([g["id"] for g in glist], dtype=np.int64),
                gt_size=np.array([g["count"] for g in glist], dtype=np.int64),
                inter=np.array(sorted(inter), dtype=np.int64).reshape(-1, 3))


def average_precision(scenes, class_ids):
    """``scenes``: list of (gts, preds) of assign_scene -> ap_scores [1, C, 10]"""
    ap = np.zeros((1, len(class_ids), len(OVERLAPS)))
    for oi, th in enumerate(OVERLAPS):
        visited = set()
        for li, c in enumerate(int(c) for c in class_ids):
            y_true, y_score, hard_fn, has_gt, has_pred = [], [], 0, False, False
            for si, (gts, preds) in enumerate(scenes):
                big = [g for g in gts[c] if g["count"] >= MIN_REGION]
                has_gt |= bool(big)
                has_pred |= bool(preds[c])
                extra = []
                for gt in big:
                    score = None
                    for pred, inter in gt["matched"]:
                        if (si, pred["key"]) in visited:
                            continue
                        if float(inter) / (gt["count"] + pred["count"] - inter) > th:
                            if score is None:
                                score = pred["conf"]
                                visited.add((si, pred["key"]))
                            else:
                                extra.append(min(score, pred["conf"]))
                                score = max(score, pred["conf"])
                    if score is None:
                        hard_fn += 1
                    else:
                        y_true.append(1)
                        y_score.append(score)
                y_true += [0] * len(extra)
                y_score += extra
                for pred in preds[c]:
                    if any(float(n) / (g["count"] + pred["count"] - n) > th for g, n in pred["matched"]):
                        continue
                    ignore = pred["void"] + sum(n for g, n in pred["matched"] if g["id"] < 1000) \
                        + sum(n for g, n in pred["matched"] if g["count"] < MIN_REGION)
                    if float(ignore) / pred["count"] <= th:
                        y_true.append(0)
                        y_score.append(pred["conf"])
            if has_gt and has_pred:
                y_true, y_score = np.array(y_true, dtype=np.float64), np.array(y_score, dtype=np.float64)
                thresholds = np.unique(y_score)
                prec, rec = np.zeros(len(thresholds) + 1), np.zeros(len(thresholds) + 1)
                for k, t in enumerate(thresholds):
                    tp = y_true[y_score >= t].sum()
                    fp = (y_score >= t).sum() - tp
                    fn = y_true[y_score < t].sum() + hard_fn
                    prec[k], rec[k] = tp / (tp + fp), tp / (tp + fn)
                prec[-1], rec[-1] = 1., 0.
                r = np.concatenate([rec[:1], rec, [0.]])
                ap[0, li, oi] = np.dot(prec, np.convolve(r, [-0.5, 0, 0.5], "valid"))
            else:
                ap[0, li, oi] = 0.0 if has_gt else np.nan
    return ap


def ap_averages(ap):
    """all_ap, all_ap_50%, all_ap_25% and the per-class triples [C, 3] of ap_scores [1, C, 10]"""
    o25, o50 = np.isclose(OVERLAPS, 0.25), np.isclose(OVERLAPS, 0.5)
    t = np.ascontiguousarray(ap[0].T)
    with np.errstate(all="ignore"):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            alls = np.array([np.nanmean(t[~o25]), np.nanmean(t[o50]), np.nanmean(t[o25])])
    per_class = np.stack([np.average(ap[0][:, ~o25], axis=1), ap[0][:, o50][:, 0], ap[0][:, o25][:, 0]], 1)
    return alls, per_class


# ---- S3DIS coverage / precision / recall -------------------------------------------------------------------------

class S3DISRef(object):
    def __init__(self, num_classes=13, iou_threshold=0.5):
        self.C, self.thr = num_classes, iou_threshold
        self.total_gt = np.zeros(num_classes)
        self.tp = [[] for _ in range(num_classes)]
        self.fp = [[] for _ in range(num_classes)]
        self.cov = [[] for _ in range(num_classes)]
        self.wcov = [[] for _ in range(num_classes)]

    def process(self, sem_label, masks, sem_gt, ins_gt):
        pred = [[] for _ in range(self.C)]
        for c, m in zip(np.asarray(sem_label) - 1, masks):
            pred[int(c)].append(np.asarray(m).astype(bool))
        gt = [[] for _ in range(self.C)]
        for i in np.unique(ins_gt):
            m = ins_gt == i
            hist = np.bincount(sem_gt[m].astype(np.int64))
            gt[int(np.argmax(hist))].append(m)                         # the mode, the smallest class among ties
        for c in range(self.C):
            cov, wcov, n_all = 0, 0, 0
            for g in gt[c]:
                best = 0.
                for p in pred[c]:
                    best = max(best, float(np.sum(g & p)) / np.sum(g | p))
                cov += best
                wcov += np.sum(g) * best
                n_all += np.sum(g)
            if gt[c]:
                self.cov[c].append(cov / len(gt[c]))
                self.wcov[c].append(wcov / n_all)
            self.total_gt[c] += len(gt[c])
            for p in pred[c]:
                best = -1.
                for g in gt[c]:
                    iou = float(np.sum(g & p)) / np.sum(g | p)
                    if iou > best:
                        best = iou
                self.tp[c].append(1. if best > self.thr else 0.)
                self.fp[c].append(0. if best > self.thr else 1.)

    def evaluate(self):
        nan = float("nan")
        out = dict(MUCov=np.array([np.mean(v) if v else nan for v in self.cov]),
                   MWCov=np.array([np.mean(v) if v else nan for v in self.wcov]))
        tp, fp = np.array([np.sum(v) for v in self.tp]), np.array([np.sum(v) for v in self.fp])
        with np.errstate(divide="ignore", invalid="ignore"):
            out["precision"], out["recall"] = tp / (tp + fp), tp / self.total_gt
        return out
