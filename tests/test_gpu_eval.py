"""GPU: the two counting kernels of csrc/evalcount.hip against ``np.add.at`` (tests/eval_ref.py) -- every comparison is
exact integer equality -- and the three evaluators of wsis_eval end to end on the fixture recorded from the reference
(tests/golden/eval_golden.npz), with the checks and the derived fp64 bound of tests/test_eval_host.py.

Shapes stand on the kernel's edges: a workgroup of wsis_mask_overlap owns ``chunk`` points (waves of 64 lanes) and a
tile of R(G) rows whose R x G counters must fit its LDS table, so N runs over the wave and chunk edges, P over the tile
edges and G over 1, 2, the largest G with the largest R, the next one and the maximum; wsis_label_pairs keeps its table
in LDS up to 4096 entries and adds to global memory above."""
import functools
import os

import numpy as np
import pytest
import torch

import eval_ref
import test_eval_host as host

pytestmark = pytest.mark.gpu
DEV = "cuda"
INT64_MIN = -2 ** 63


@functools.lru_cache(maxsize=None)
def _geometry():
    import wsis_eval
    chunk = wsis_eval.mask_overlap_chunk()
    rmax = wsis_eval.mask_overlap_tile_rows(1)
    g_edge = max(G for G in range(1, 4097) if wsis_eval.mask_overlap_tile_rows(G) == rmax)
    assert chunk % 64 == 0 and wsis_eval.mask_overlap_tile_rows(g_edge + 1) < rmax
    assert all(wsis_eval.mask_overlap_tile_rows(G) * G <= 4096 or wsis_eval.mask_overlap_tile_rows(G) == 1
               for G in (1, 2, g_edge, g_edge + 1, 4095, 4096))
    return chunk, g_edge


def _n_values():
    chunk, _ = _geometry()
    return (0, 1, 63, 64, 65, chunk - 1, chunk, chunk + 1, 2 * chunk + 7)


def _run_overlap(masks, col, G):
    """the device call on buffers pre-filled with garbage, twice: both calls must give the same bytes"""
    import wsis_eval
    m, c = torch.from_numpy(masks).to(DEV), torch.from_numpy(col).to(DEV)
    if m.dtype == torch.bool:
        m = m.view(torch.uint8)
    outs = []
    for fill in (-1, 0x5A5A5A5A):
        table = torch.full((len(masks), G), fill, dtype=torch.int64, device=DEV)
        rows = torch.full((len(masks),), fill, dtype=torch.int64, device=DEV)
        wsis_eval.mask_overlap(m, c, G, out=(table, rows))
        outs.append((table.cpu().numpy(), rows.cpu().numpy()))
    assert outs[0][0].tobytes() == outs[1][0].tobytes() and outs[0][1].tobytes() == outs[1][1].tobytes()
    return outs[0]


def _check_overlap(masks, col, G):
    table, rows = _run_overlap(masks, col, G)
    want_t, want_r = eval_ref.overlap_table(masks, col, G)
    assert np.array_equal(rows, want_r), (masks.shape, G, "rows")
    assert np.array_equal(table, want_t), (masks.shape, G, "table")


def _random_case(P, N, G, dtype, seed):
    rng = np.random.default_rng(seed)
    member = rng.random((P, N)) < 0.08                                  # sparse, as predictions are
    if dtype == np.int64:
        values = np.array([1, 2, -1, 1 << 40, INT64_MIN], dtype=np.int64)
        masks = np.where(member, values[rng.integers(0, len(values), (P, N))], 0).astype(np.int64)
    else:
        masks = member.astype(dtype)
    # coherent columns with runs, as ground-truth instances are, and a few points outside every column
    col = np.repeat(rng.integers(0, G, N // 37 + 1), 37)[:N].astype(np.int32)
    col[rng.random(N) < 0.05] = -1
    return np.ascontiguousarray(masks), col


@pytest.mark.parametrize("dtype", [np.uint8, np.int64])
@pytest.mark.parametrize("g_kind", ["one", "two", "edge", "past_edge", "max"])
def test_mask_overlap_over_the_tile_and_chunk_edges(g_kind, dtype):
    import wsis_eval
    _, g_edge = _geometry()
    G = {"one": 1, "two": 2, "edge": g_edge, "past_edge": g_edge + 1, "max": 4096}[g_kind]
    R = wsis_eval.mask_overlap_tile_rows(G)
    for P in (0, 1, R, R + 1, 2 * R + 3):
        for N in _n_values():
            masks, col = _random_case(P, N, G, dtype, 7919 * P + N)
            _check_overlap(masks, col, G)


def test_mask_overlap_int64_members_are_any_bit_set():
    N, G = 300, 5
    masks = np.zeros((5, N), dtype=np.int64)
    for r, v in enumerate((1, 2, -1, 1 << 40, INT64_MIN)):             # 1 << 40 and INT64_MIN have zero low words
        masks[r, r::7] = v
    col = (np.arange(N) % G).astype(np.int32)
    table, rows = _run_overlap(masks, col, G)
    assert np.array_equal(rows, np.count_nonzero(masks, axis=1)) and (rows > 0).all()
    assert np.array_equal(table, eval_ref.overlap_table(masks, col, G)[0])


@pytest.mark.parametrize("dtype", [np.bool_, np.int64])
def test_mask_overlap_column_patterns(dtype):
    import wsis_eval
    chunk, _ = _geometry()
    N, G = chunk + 200, 64
    R = wsis_eval.mask_overlap_tile_rows(G)
    P = R + 2
    lane = np.arange(N)
    patterns = {"one column": np.full(N, 3), "64 distinct columns": lane % 64, "alternating": lane % 2 * 63,
                "all negative": np.full(N, -1), "negative every third": np.where(lane % 3 == 0, -7, lane % 64)}
    rng = np.random.default_rng(5)
    masks = rng.random((P, N)) < 0.3
    masks[:, 100] = True                                                # a point in every row of the first tile
    masks[:, chunk + 64] = True
    masks[-2] = False                                                   # an all-zero row
    masks[-1] = True                                                    # an all-ones row
    masks = masks.astype(dtype)
    for name, col in patterns.items():
        table, rows = _run_overlap(masks, col.astype(np.int32), G)
        want_t, want_r = eval_ref.overlap_table(masks, col, G)
        assert np.array_equal(table, want_t) and np.array_equal(rows, want_r), name
        assert rows[-2] == 0 and rows[-1] == N and not table[-2].any()
    # a run of a few thousand points, every point a member of one row
    col = np.repeat(np.arange(3), 1500).astype(np.int32)
    table, rows = _run_overlap(np.ones((1, 4500), dtype=dtype), col, 3)
    assert table.tolist() == [[1500, 1500, 1500]] and rows.tolist() == [4500]


def test_mask_overlap_error_statuses_leave_the_outputs_alone():
    import wsis_native as _n
    hip = _n.hip()
    P, N = 2, 100
    masks = torch.ones((P, N), dtype=torch.int64, device=DEV)
    col = torch.zeros(N, dtype=torch.int32, device=DEV)
    table = torch.full((P * 4,), 77, dtype=torch.int64, device=DEV)
    rows = torch.full((P,), 77, dtype=torch.int64, device=DEV)
    for G, elem in ((0, 8), (4097, 8), (1, 4), (-1, 1)):
        status = hip.wsis_mask_overlap(_n.ptr(masks), elem, P, N, _n.ptr(col), G, _n.ptr(table), _n.ptr(rows), None, 0,
                                       _n.stream_ptr())
        assert status != 0 and hip.wsis_last_error()
    torch.cuda.synchronize()
    assert (table == 77).all() and (rows == 77).all()
    assert hip.wsis_mask_overlap_workspace_bytes(P, N, 0) == -1 and hip.wsis_mask_overlap_workspace_bytes(P, N, 4097) == -1
    assert hip.wsis_mask_overlap_workspace_bytes(-1, N, 1) == -1 and hip.wsis_mask_overlap_workspace_bytes(P, N, 4096) >= 0
    assert hip.wsis_label_pairs(_n.ptr(col), _n.ptr(col), N, 257, 256, _n.ptr(table), _n.stream_ptr()) != 0
    assert hip.wsis_label_pairs(_n.ptr(col), _n.ptr(col), N, 0, 1, _n.ptr(table), _n.stream_ptr()) != 0


@pytest.mark.parametrize("A,B", [(1, 1), (41, 41), (64, 64), (241, 17), (256, 256)])
def test_label_pairs(A, B):
    """A * B = 1, the ScanNet confusion matrix, the last LDS table (4096), the first global one (4097), the maximum"""
    import wsis_eval
    for N in _n_values():
        rng = np.random.default_rng(A * 100003 + N)
        a = np.repeat(rng.integers(0, A, N // 29 + 1), 29)[:N]          # labels are spatially coherent
        b = np.where(rng.random(N) < 0.2, rng.integers(0, B, N), a % B)
        a[rng.random(N) < 0.03] = -1                                    # negative and out-of-range labels are skipped
        b[rng.random(N) < 0.03] = B
        a[rng.random(N) < 0.02] = A + 5
        b[rng.random(N) < 0.02] = -100
        out = torch.full((A, B), -3, dtype=torch.int64, device=DEV)
        got = wsis_eval.label_pairs(torch.from_numpy(a.astype(np.int32)).to(DEV),
                                    torch.from_numpy(b.astype(np.int32)).to(DEV), A, B, out=out).cpu().numpy()
        assert np.array_equal(got, eval_ref.pair_table(a, b, A, B)), (A, B, N)
        assert N < 1000 or got.sum() < N                                # some points were outside the table


# ---- end to end on the fixture -------------------------------------------------------------------------------------

def _mask_forms(masks):
    yield "uint8 tensor", torch.from_numpy(masks.astype(np.uint8)).to(DEV)
    yield "int64 tensor", torch.from_numpy(masks.astype(np.int64) * -5).to(DEV)
    yield "numpy bool", masks


@pytest.mark.parametrize("table", host.TABLES)
def test_instance_evaluator_process_reproduces_the_reference(table):
    import wsis_eval
    g, masks = host.golden()
    ids = g[f"class_ids_{table}"]
    for form in range(3):
        ev = wsis_eval.InstanceEvaluator(ids, [f"c{i}" for i in ids])
        for n, tag in enumerate("ab", 1):
            name, m = list(_mask_forms(masks[tag]))[form]
            gt = g[f"{tag}_gt_ids"] if form else torch.from_numpy(g[f"{tag}_gt_ids"]).to(DEV)
            ev.process(tag, g[f"{tag}_conf"], g[f"{tag}_label_id"], m, gt)
            host.check_scene_record(g, table, tag, ev.scenes[tag])
            host.check_instance_results(g, table, n, ev.evaluate())


def test_s3dis_evaluator_process_reproduces_the_reference():
    import wsis_eval
    g, masks = host.golden()
    for form in range(3):
        ev = wsis_eval.S3DISInstanceEvaluator()
        for n, tag in enumerate("ab", 1):
            name, m = list(_mask_forms(masks[tag]))[form]
            ev.process(g[f"{tag}_conf"], g[f"{tag}_s3_label"], m, g[f"{tag}_sem_gt"], g[f"{tag}_ins_gt"])
            res = ev.evaluate()
            assert np.array_equal(ev.total_gt_ins, g[f"s3_{n}_total_gt"])
            for key in ("MUCov", "MWCov", "precision", "recall"):
                host.assert_close(res[key], g[f"s3_{n}_{key}"], host.n_terms(g), f"{key} {n} ({name})")


@pytest.mark.parametrize("tag", "ab")
def test_semantic_evaluator_process_reproduces_the_reference(tag):
    import wsis_eval
    g, _ = host.golden()
    make = wsis_eval.SemanticEvaluator.scannet if tag == "a" else wsis_eval.SemanticEvaluator.s3dis
    ev = make(ignore=tuple(g[f"sem_{tag}_ignore"].tolist()))
    gt = g[f"{tag}_sem_eval_gt"]
    ev.process(g[f"{tag}_sem_eval_pred"], gt)                           # numpy
    assert np.array_equal(ev.confusion, g[f"sem_{tag}_1_confusion"])
    ev.process(torch.from_numpy(g[f"{tag}_sem_eval_pred2"]).to(DEV), torch.from_numpy(gt).to(DEV))
    assert np.array_equal(ev.confusion, g[f"sem_{tag}_2_confusion"])
    res = ev.iou()
    for k in ("tp", "fp", "fn", "union"):
        assert np.array_equal(res[k], g[f"sem_{tag}_2_{k}"]), k
    inc = ~np.isnan(g[f"sem_{tag}_2_ious"])
    assert np.array_equal(res["ious"][inc], g[f"sem_{tag}_2_ious"][inc])
    with pytest.raises(ValueError):
        ev.process(g[f"{tag}_sem_eval_pred"], np.where(np.arange(len(gt)) == 5, -1, gt))      # numpy would wrap it
    with pytest.raises(ValueError):
        ev.process(np.where(np.arange(len(gt)) == 5, 1000, g[f"{tag}_sem_eval_pred"]), gt)
    assert np.array_equal(ev.confusion, g[f"sem_{tag}_2_confusion"])    # a refused scene adds nothing


def test_too_many_ground_truth_ids():
    import wsis_eval
    N = 5000
    with pytest.raises(ValueError):
        wsis_eval.InstanceEvaluator.scannet().process("s", [0.5], [3], np.ones((1, N), dtype=bool), np.arange(N) + 3000)


class _Graph(object):          # the one igraph method the reference calls
    def __init__(self, lists):
        self.lists = lists

    def neighbors(self, vertex, mode="all"):
        return [int(v) for v in self.lists[int(vertex)]]


def test_clustering_in_graph_as_tensor_feeds_the_instance_evaluator():
    import inference
    import wsis_eval
    from oracle import cluster_ref
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cluster_golden.npz"))
    S = len(g["a_sem"])
    graph = _Graph(cluster_ref.neighbour_lists(g["a_edges"], S))
    args = ("golden", g["a_xyz"], g["a_superpoint"], graph, g["a_sem"], g["a_off"], g["a_occ"], g["a_size"])
    conf0, label0, masks0 = inference.clustering_in_graph(*args)
    conf1, label1, masks1 = inference.clustering_in_graph(*args, as_tensor=True)
    assert isinstance(masks0, np.ndarray) and torch.is_tensor(masks1) and masks1.is_cuda and masks1.dtype == torch.int64
    assert np.array_equal(conf0, conf1) and np.array_equal(label0, label1) and len(masks0) > 0
    assert np.array_equal(masks1.cpu().numpy(), masks0)
    # ground truth = the predicted instances themselves under their predicted labels
    gt_ids = np.zeros(masks0.shape[1], dtype=np.int64)
    for k, (m, lab) in enumerate(zip(masks0, label0)):
        gt_ids[m != 0] = int(lab) * 1000 + k + 1
    ev = wsis_eval.InstanceEvaluator.scannet()
    ev.process("golden", conf1, label1, masks1, gt_ids)
    sc = ev.scenes["golden"]
    kept = masks0.astype(bool).sum(1) >= 100
    assert np.array_equal(sc["pred_size"], masks0.astype(bool).sum(1)[kept]) and not sc["pred_void"].any()
    res = ev.evaluate()
    present = ~np.isnan(res["ap_scores"][0, :, 0])
    assert present.any() and np.abs(res["ap_scores"][0][present] - 1.0).max() < 1e-12      # every instance found whole
