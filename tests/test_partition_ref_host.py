"""CPU: the numpy oracle of the partition front end (tests/partition_ref.py) against what the reference's own
``compute_graph_nn_2`` and edge-weight expression computed (tests/golden/partition_golden.npz), the oracle's own
invariants, the tolerance constants, and the refusals of ``wsis_partition`` that need no device."""
import os

import numpy as np
import pytest

import partition_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
TAGS = ("room_a", "room_b")
K_ADJ, K_GEOF = 10, 45
_CACHE = {}


class Golden(object):
    """one room of the fixture, with the oracle's neighbour lists and features computed once and shared"""

    def __init__(self, tag):
        z = _CACHE.get("npz")
        if z is None:
            with np.load(os.path.join(HERE, "golden", "partition_golden.npz")) as f:
                z = _CACHE["npz"] = {k: f[k] for k in f.files}
        for k, v in z.items():
            if k.startswith(tag + "_"):
                setattr(self, k[len(tag) + 1:], v)
        self.tag, self.V = tag, len(self.xyz)

    def knn(self):
        key = (self.tag, "knn")
        if key not in _CACHE:
            _CACHE[key] = ref.knn(self.xyz, K_GEOF)
        return _CACHE[key]

    def geof(self):
        key = (self.tag, "geof")
        if key not in _CACHE:
            _CACHE[key] = ref.geof(self.xyz, self.knn()[0])
        return _CACHE[key]


@pytest.mark.parametrize("tag", TAGS)
def test_oracle_reproduces_the_reference(tag):
    gold = Golden(tag)
    nbr, d2 = gold.knn()
    assert gold.target2.dtype == np.uint32 and np.array_equal(nbr.flatten().astype(np.uint32), gold.target2)
    a = ref.assemble(gold.geof()["geof"], gold.rgb, nbr, d2, K_ADJ)
    for name in ("source", "target", "distances"):
        assert a[name].dtype == getattr(gold, name).dtype and np.array_equal(a[name], getattr(gold, name)), name
    assert a["edge_weight"].dtype == gold.edge_weight.dtype == np.float32
    margin = ref.edge_weight_margin(gold.distances, a["mean"], gold.mean)
    err = np.abs(a["edge_weight"].astype(np.float64) - gold.edge_weight.astype(np.float64))
    print(f"{tag}: oracle mean {float(a['mean']):.9g} reference mean {float(gold.mean):.9g}; edge_weight largest error "
          f"{err.max():.3g}, largest error / margin {(err / margin).max():.3g}")
    assert (err <= margin).all()
    assert a["features"].dtype == np.float32 and a["features"].shape == (gold.V, 7)


@pytest.mark.parametrize("tag", TAGS)
def test_fixture_is_clear_of_ties(tag):
    gold = Golden(tag)
    assert len(np.unique(gold.xyz, axis=0)) == gold.V
    _, d2 = ref.knn(gold.xyz, K_GEOF + 1)
    assert (np.diff(d2, axis=1) > 0).all() and (d2[:, 0] > 0).all()


def test_ev_tol_is_eight_times_the_solvers_disagreement():
    worst, smallest_gap, left_out = 0.0, np.inf, 0.0
    for tag in TAGS:
        gold = Golden(tag)
        for c in ref.cov_of(gold.xyz, gold.knn()[0]):
            a = np.linalg.eig(c)[0]
            assert np.isrealobj(a)
            d = np.abs(-np.sort(-a) - -np.sort(-np.linalg.eigvalsh(c))).max()
            worst = max(worst, d / np.trace(c))
        gap = gold.geof()["gap"]
        smallest_gap, left_out = min(smallest_gap, float(gap.min())), max(left_out, float((gap <= ref.GAP_MIN).mean()))
    print("largest |eig - eigvalsh| / trace:", worst, " GAP_MIN:", ref.GAP_MIN, " smallest relative eigen-gap:", smallest_gap,
          " share of points left out of the verticality comparison:", left_out)
    # the recorded figure belongs to one LAPACK build: another may differ by a few steps, EV_TOL keeps a factor of 8
    assert worst <= 2 * ref.EV_MEASURED
    assert ref.EV_TOL == max(8 * ref.EV_MEASURED, 2.0 ** -50)
    assert ref.GAP_MIN == ref.gap_min() and 0 < ref.GAP_MIN < 1e-4
    bound = 2 * np.sqrt(3.0) * ref.EV_TOL * (9 + 6 / ref.GAP_MIN)
    assert abs(bound - ref.EPS32) <= 1e-9 * ref.EPS32          # at GAP_MIN the verticality bound is one fp32 step at 1
    assert ref.cov_tol(45) == 46 * 2.0 ** -52
    assert left_out <= 0.01


def test_prune_invariants():
    xyz, rgb = ref.make_room(3, n=6000, size=(1.5, 1.2, 1.0))
    labels = (np.arange(len(xyz)) * 5 % 14).astype(np.uint8)
    pr = ref.prune(xyz, 0.03, rgb, labels, 13)
    p2v, V = pr["p2v"].astype(np.int64), len(pr["xyz"])
    # ids appear in first-occurrence order
    first = np.full(V, len(xyz))
    np.minimum.at(first, p2v, np.arange(len(xyz)))
    assert (np.diff(first) > 0).all() and p2v[0] == 0 and p2v.max() == V - 1
    # every point lies in its voxel's cell
    b, mn = ref.bins(xyz, 0.03)
    assert np.array_equal(b, b[first][p2v])
    assert (b >= 0).all() and np.array_equal(mn, xyz.min(0))
    # positions are sequential float32 sums in point order; colours truncate
    for v in (0, 1, V // 2, V - 1, int(np.argmax(pr["count"]))):
        acc, col = np.zeros(3, np.float32), np.zeros(3, np.uint32)
        for p in np.nonzero(p2v == v)[0]:
            acc = acc + xyz[p]
            col = col + rgb[p]
        n = np.float32(pr["count"][v])
        assert acc.dtype == np.float32 and np.array_equal(acc / n, pr["xyz"][v])
        assert np.array_equal((col.astype(np.float32) / n).astype(np.uint8), pr["rgb"][v])
    assert np.array_equal(pr["label_hist"].sum(1), pr["count"]) and pr["label_hist"].shape == (V, 14)
    assert pr["count"].sum() == len(xyz) and pr["count"].max() > 1
    with pytest.raises(IndexError):
        ref.prune(xyz, 0.03, rgb, labels, 12)


def test_oracle_knn_orders_ties_by_id_and_drops_self_by_id():
    xyz = np.zeros((70, 3), np.float32)
    xyz[60:, 0] = np.arange(1, 11)
    nbr, d2 = ref.knn(xyz, 64)
    assert np.array_equal(nbr[5, :59], [i for i in range(60) if i != 5]) and (d2[5, :59] == 0).all()
    assert np.array_equal(nbr[5, 59:], [60, 61, 62, 63, 64])
    assert np.array_equal(nbr[69, :3], [68, 67, 66])
    with pytest.raises(ValueError):
        ref.knn(xyz[:10], 10)


def test_refusals_that_need_no_device():
    import torch
    import wsis_native
    import wsis_partition as wp
    xyz = np.zeros((100, 3), np.float32)
    rgb = np.zeros((100, 3), np.uint8)
    bad = [lambda: wp.prune(xyz.astype(np.float64), 0.03, rgb), lambda: wp.prune(xyz, 0.03, rgb.astype(np.int32)),
           lambda: wp.prune(xyz[:0], 0.03, rgb[:0]), lambda: wp.knn(xyz, 65), lambda: wp.knn(np.zeros((75, 4), np.float32), 10),
           lambda: wp.prune(np.zeros(100, np.float32), 0.03, rgb), lambda: wp.prune(xyz, 0.03, np.zeros((100, 4), np.uint8)), lambda: wp.knn(xyz, 0),
           lambda: wp.knn(xyz[:45], 45), lambda: wp.knn(xyz.astype(np.float64), 10),
           lambda: wp.partition_inputs(xyz, rgb, k_nn_adj=46, k_nn_geof=45), lambda: wp.partition_inputs(xyz, rgb, k_nn_geof=65),
           lambda: wp.partition_inputs(xyz.astype(np.float16), rgb), lambda: wp.geometric_features(xyz.astype(np.float64), None),
           # no CPU fallback
           lambda: wp.prune(xyz, 0.03, rgb, device="cpu"), lambda: wp.knn(torch.zeros(100, 3), 10, device="cpu"),
           lambda: wp.geometric_features(xyz, np.zeros((100, 10), np.int32), device="cpu"),
           lambda: wp.partition_inputs(xyz, rgb, device="cpu"),
           lambda: wp.generate_superpoints(xyz, rgb, lambda *a: (None, None), device="cpu")]
    for i, f in enumerate(bad):
        with pytest.raises(wsis_native.WsisError):
            f()
            print("not refused:", i)
