"""CPU: the host layer of wsis_eval (``add_counts`` + the metric expressions) against the results recorded from the
reference's own evaluators (tests/golden/eval_golden.npz, made by tests/golden/make_eval_golden.py), fed with tables
that the numpy oracle tests/eval_ref.py computes from the fixture; and the oracle's own metrics against the same file.

Integers are compared with equality.  The fp64 metrics are the reference's expressions on identical integers; they may
differ from the recorded values only by the order of additions of their longest sum: an average precision is a dot
product over at most (kept predictions + 1) points of the precision-recall curve, whose terms are all >= 0, so each side
is within n * 2^-53 of the exact value, relative -- n * 2^-52 between them.  An average over the C x 9 table adds as
many terms again.
"""
import os

import numpy as np
import pytest

import eval_ref
import wsis_eval
import wsis_native

HERE = os.path.dirname(os.path.abspath(__file__))
TABLES = ("scannet", "s3dis")
_CACHE = {}


def golden():
    if not _CACHE:
        g = dict(np.load(os.path.join(HERE, "golden", "eval_golden.npz")))
        _CACHE["g"] = g
        _CACHE["masks"] = {t: eval_ref.unpack_masks(g[f"{t}_masks_bits"], int(g[f"{t}_n_points"])) for t in "ab"}
    return _CACHE["g"], _CACHE["masks"]


def n_terms(g, averaged=0):
    return sum(len(g[f"{t}_conf"]) for t in "ab") + 1 + averaged


def assert_close(got, want, n, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    assert (np.isnan(got) == np.isnan(want)).all(), f"{what}: nan pattern"
    ok = ~np.isnan(want)
    err = np.abs(got[ok] - want[ok])
    bound = n * 2.0 ** -52 * np.abs(want[ok])
    assert (err <= bound).all(), f"{what}: error {err.max()} above {n} * 2^-52 relative"


def instance_tables(g, masks, tag):
    """what process() hands to InstanceEvaluator.add_counts, computed by the oracle"""
    gt_id, col, gt_size = np.unique(g[f"{tag}_gt_ids"], return_inverse=True, return_counts=True)
    T, rows = eval_ref.overlap_table(masks[tag], col, len(gt_id))
    return rows, gt_id, gt_size, T


def s3dis_tables(g, masks, tag, C=13):
    gt_id, col, gt_size = np.unique(g[f"{tag}_ins_gt"], return_inverse=True, return_counts=True)
    T, rows = eval_ref.overlap_table(masks[tag], col, len(gt_id))
    return rows, gt_size, eval_ref.pair_table(col, g[f"{tag}_sem_gt"], len(gt_id), C), T


def check_instance_results(g, table, n, res):
    C = len(g[f"class_ids_{table}"])
    assert_close(res["ap_scores"], g[f"ap_{table}_{n}_scores"], n_terms(g), f"ap_scores {table} {n}")
    alls = [res["all_ap"], res["all_ap_50%"], res["all_ap_25%"]]
    assert_close(alls, g[f"ap_{table}_{n}_all"], n_terms(g, 9 * C), f"averages {table} {n}")
    per_class = [[res["classes"][f"c{i}"][k] for k in ("ap", "ap50%", "ap25%")] for i in g[f"class_ids_{table}"]]
    assert_close(per_class, g[f"ap_{table}_{n}_classes"], n_terms(g, 9), f"class averages {table} {n}")


def check_scene_record(g, table, tag, sc):
    """the integers the evaluator keeps per scene against the reference's own"""
    for key in ("pred_size", "pred_void", "gt_id", "gt_size"):
        assert np.array_equal(sc[key], g[f"ap_{table}_{tag}_{key}"]), (table, tag, key)
    inter = np.stack([sc["inter_pred"], sc["inter_gt"], sc["inter"]], 1)
    assert np.array_equal(inter, g[f"ap_{table}_{tag}_inter"]), (table, tag, "intersections")


@pytest.mark.parametrize("table", TABLES)
def test_instance_ap_from_counts(table):
    g, masks = golden()
    ids = g[f"class_ids_{table}"]
    ev = wsis_eval.InstanceEvaluator(ids, [f"c{i}" for i in ids])
    for n, tag in enumerate("ab", 1):
        ev.add_counts(tag, g[f"{tag}_conf"], g[f"{tag}_label_id"], *instance_tables(g, masks, tag))
        check_scene_record(g, table, tag, ev.scenes[tag])
        check_instance_results(g, table, n, ev.evaluate())
    scores = g[f"ap_{table}_2_scores"][0]
    assert np.isnan(scores).all(1).any() and (scores > 0).any()         # the nan rows are compared above (equal_nan)
    ev.reset()
    assert not ev.scenes
    ev.add_counts("a", g["a_conf"], g["a_label_id"], *instance_tables(g, masks, "a"))
    check_instance_results(g, table, 1, ev.evaluate())                  # after reset: scene a alone again


def test_instance_evaluator_constructors_and_errors():
    g, masks = golden()
    ev = wsis_eval.InstanceEvaluator.scannet()
    assert np.array_equal(ev.class_ids, g["class_ids_scannet"]) and len(ev.class_labels) == 18
    assert np.array_equal(wsis_eval.InstanceEvaluator.s3dis().class_ids, g["class_ids_s3dis"])
    rows, gt_id, gt_size, T = instance_tables(g, masks, "a")
    with pytest.raises(ValueError):
        ev.add_counts("a", g["a_conf"], g["a_label_id"], rows, gt_id[::-1], gt_size, T)         # ids not ascending
    with pytest.raises(ValueError):
        ev.add_counts("a", g["a_conf"], g["a_label_id"], rows, gt_id, gt_size, T.astype(np.float64))
    with pytest.raises(ValueError):
        ev.add_counts("a", g["a_conf"], g["a_label_id"], rows - 1, gt_id, gt_size, T)           # table above the sizes
    with pytest.raises(ValueError):
        ev.add_counts("a", g["a_conf"][:-1], g["a_label_id"], rows, gt_id, gt_size, T)
    assert not ev.scenes
    res = ev.evaluate()                                                 # nothing processed: every class is nan, no warning
    assert np.isnan(res["ap_scores"]).all() and np.isnan(res["all_ap"])


def test_s3dis_coverage_from_counts():
    g, masks = golden()
    ev = wsis_eval.S3DISInstanceEvaluator()
    for n, tag in enumerate("ab", 1):
        ev.add_counts(g[f"{tag}_s3_label"], *s3dis_tables(g, masks, tag))
        res = ev.evaluate()
        assert np.array_equal(ev.total_gt_ins, g[f"s3_{n}_total_gt"])
        for key in ("MUCov", "MWCov", "precision", "recall"):
            assert_close(res[key], g[f"s3_{n}_{key}"], n_terms(g), f"{key} {n}")
        assert_close(res["mMUCov"], np.mean(g[f"s3_{n}_MUCov"]), n_terms(g, 13), "mMUCov")
        assert_close(res["mRecall"], np.mean(g[f"s3_{n}_recall"]), n_terms(g, 13), "mRecall")
    assert np.isnan(g["s3_2_precision"]).any() and np.isnan(g["s3_2_MUCov"]).any()      # empty classes are in the fixture
    ev.reset()
    ev.add_counts(g["a_s3_label"], *s3dis_tables(g, masks, "a"))
    assert_close(ev.evaluate()["MWCov"], g["s3_1_MWCov"], n_terms(g), "MWCov after reset")


def test_s3dis_errors_and_no_warning():
    import warnings
    g, masks = golden()
    rows, gt_size, hist, T = s3dis_tables(g, masks, "b")
    ev = wsis_eval.S3DISInstanceEvaluator()
    with pytest.raises(ValueError):
        ev.add_counts(g["b_s3_label"] * 0, rows, gt_size, hist, T)                              # label 0 -> class -1
    with pytest.raises(ValueError):
        ev.add_counts(g["b_s3_label"] + 13, rows, gt_size, hist, T)
    bad = hist.copy()
    bad[0, np.argmax(hist[0])] -= 1                                                             # a point with sem_gt outside
    with pytest.raises(ValueError):
        ev.add_counts(g["b_s3_label"], rows, gt_size, bad, T)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        res = ev.evaluate()                                             # all classes empty: nan, as np.mean([]) gives
    assert all(np.isnan(res[k]).all() for k in ("MUCov", "MWCov", "precision", "recall"))


@pytest.mark.parametrize("tag", "ab")
def test_semantic_iou_from_counts(tag):
    g, _ = golden()
    make = wsis_eval.SemanticEvaluator.scannet if tag == "a" else wsis_eval.SemanticEvaluator.s3dis
    ev = make(ignore=tuple(g[f"sem_{tag}_ignore"].tolist()))
    size = ev.confusion.shape[0]
    assert ev.confusion.shape == g[f"sem_{tag}_1_confusion"].shape and ev.confusion.dtype == np.int64
    gt = g[f"{tag}_sem_eval_gt"]
    for n, key in enumerate(("sem_eval_pred", "sem_eval_pred2"), 1):
        ev.add_counts(eval_ref.pair_table(gt, g[f"{tag}_{key}"], size, size), len(gt))
        assert np.array_equal(ev.confusion, g[f"sem_{tag}_{n}_confusion"])
        res = ev.iou()
        for k in ("tp", "fp", "fn", "union"):
            assert np.array_equal(res[k], g[f"sem_{tag}_{n}_{k}"]), k
        want = g[f"sem_{tag}_{n}_ious"]                                  # recorded for the included classes
        inc = ~np.isnan(want)
        assert np.array_equal(res["ious"][inc], want[inc])              # one division each: identical
        assert_close(res["mean"], np.mean(want[inc]), int(inc.sum()), "mean IoU")
    ev.reset()
    assert not ev.confusion.any()
    table = eval_ref.pair_table(gt, g[f"{tag}_sem_eval_pred"], size, size)
    with pytest.raises(ValueError):
        ev.add_counts(table, len(gt) + 1)                               # a point outside the matrix
    with pytest.raises(ValueError):
        ev.add_counts(table[:-1], None)
    with pytest.raises(ValueError):
        wsis_eval.SemanticEvaluator([300], ["too large"])


def test_process_refuses_the_host():
    g, masks = golden()
    with pytest.raises(wsis_native.WsisError):
        wsis_eval.InstanceEvaluator.scannet().process("a", g["a_conf"], g["a_label_id"], masks["a"], g["a_gt_ids"],
                                                      device="cpu")
    with pytest.raises(wsis_native.WsisError):
        wsis_eval.S3DISInstanceEvaluator().process(g["a_conf"], g["a_s3_label"], masks["a"], g["a_sem_gt"], g["a_ins_gt"],
                                                   device="cpu")
    with pytest.raises(wsis_native.WsisError):
        wsis_eval.SemanticEvaluator.s3dis().process(g["b_sem_eval_pred"], g["b_sem_eval_gt"], device="cpu")


# ---- the oracle itself, pinned on the reference ------------------------------------------------------------------

@pytest.mark.parametrize("table", TABLES)
def test_oracle_instance_ap_equals_the_reference(table):
    g, masks = golden()
    ids = g[f"class_ids_{table}"]
    scenes = []
    for n, tag in enumerate("ab", 1):
        gts, preds = eval_ref.assign_scene(ids, g[f"{tag}_conf"], g[f"{tag}_label_id"], masks[tag], g[f"{tag}_gt_ids"])
        rec = eval_ref.scene_counts(ids, gts, preds)
        for key, v in rec.items():
            assert np.array_equal(v, g[f"ap_{table}_{tag}_{key}"]), (table, tag, key)
        scenes.append((gts, preds))
        ap = eval_ref.average_precision(scenes, ids)
        assert_close(ap, g[f"ap_{table}_{n}_scores"], n_terms(g), f"oracle ap_scores {table} {n}")
        alls, per_class = eval_ref.ap_averages(ap)
        assert_close(alls, g[f"ap_{table}_{n}_all"], n_terms(g, 9 * len(ids)), "oracle averages")
        assert_close(per_class, g[f"ap_{table}_{n}_classes"], n_terms(g, 9), "oracle class averages")


def test_oracle_s3dis_and_semantic_equal_the_reference():
    g, masks = golden()
    ref = eval_ref.S3DISRef()
    for n, tag in enumerate("ab", 1):
        ref.process(g[f"{tag}_s3_label"], masks[tag], g[f"{tag}_sem_gt"], g[f"{tag}_ins_gt"])
        res = ref.evaluate()
        for key in ("MUCov", "MWCov", "precision", "recall"):
            assert_close(res[key], g[f"s3_{n}_{key}"], n_terms(g), f"oracle {key} {n}")
    for tag, ids in (("a", wsis_eval.SCANNET_CLASS_IDS), ("b", wsis_eval.S3DIS_CLASS_IDS)):
        size = max(ids) + 2
        conf = eval_ref.pair_table(g[f"{tag}_sem_eval_gt"], g[f"{tag}_sem_eval_pred"], size, size)
        assert np.array_equal(conf, g[f"sem_{tag}_1_confusion"])
        include = [i for i in ids if i not in g[f"sem_{tag}_ignore"]]
        res = eval_ref.semantic_iou(conf, include)
        want = g[f"sem_{tag}_1_ious"]
        assert np.array_equal(res["union"], g[f"sem_{tag}_1_union"])
        assert np.array_equal(res["ious"][include], want[include])
