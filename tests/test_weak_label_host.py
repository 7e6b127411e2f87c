"""CPU: the numpy oracle of the weak-label stage updates (tests/weak_label_ref.py) against what the reference itself
computed (tests/golden/weak_label_golden.npz, written by tests/golden/make_weak_label_golden.py), the oracle's occupancy
against a brute-force count, the C ABI of the new kernels and the refusals that need no device."""
import ctypes
import os

import numpy as np
import pytest

import weak_label_ref as wl
import wsis_native
from wsis_datasets import PlainGraph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "weak_label_golden.npz")
NEW_SYMBOLS = ("wsis_wl_sp_stats", "wsis_wl_neighbor_source", "wsis_wl_apply_source", "wsis_wl_scene_assign",
               "wsis_wl_point_labels", "wsis_wl_occupancy_workspace_bytes", "wsis_wl_occupancy", "wsis_wl_instance_size",
               "wsis_wl_label_stats")


class Golden(object):
    """one scene of the npz: the inputs as a PlainGraph / Scene pair and the reference's results by tag"""

    def __init__(self, tag, scene_cls=wl.Scene, **scene_kw):
        z = np.load(GOLDEN)
        self.z = {k[len(tag) + 1:]: z[k] for k in z.files if k.startswith(tag + "_")}
        self.thr = float(z["thr"])
        self.iterations, self.classes = int(z["iterations"]), int(z["classes"])
        self.gap, self.max_dist = float(self.z["gap"]), float(self.z["max_dist"])
        self.scene = scene_cls(self.z["xyz"], self.z["superpoint"], **scene_kw)
        S = len(self.z["pred"])
        self.g0 = PlainGraph({"v": np.arange(S), "semantic_label": self.z["g0_sem"], "instance_label": self.z["g0_ins"],
                              "superpoint_offset_vector": self.z["g0_off"], "instance_voxel_num": np.zeros(S, np.int64),
                              "instance_size": np.zeros(S)}, self.z["edges"])

    def graph(self, tag):
        g = self.g0.copy()
        g.vs["semantic_label"], g.vs["instance_label"] = self.z[tag + "_sem"], self.z[tag + "_ins"]
        g.vs["superpoint_offset_vector"], g.is1ins = self.z[tag + "_off"], self.z[tag + "_is1ins"]
        return g

    def same_graph(self, got, tag, is1ins=True):
        """labels (and is1ins) equal, offsets within GAP"""
        assert np.array_equal(np.asarray(got.vs["semantic_label"]).astype(np.int64), self.z[tag + "_sem"]), tag
        assert np.array_equal(np.asarray(got.vs["instance_label"]).astype(np.int64), self.z[tag + "_ins"]), tag
        if is1ins:
            assert np.array_equal(got.is1ins, self.z[tag + "_is1ins"]), tag
        err = np.abs(np.asarray(got.vs["superpoint_offset_vector"], dtype=np.float64) - self.z[tag + "_off"]).max()
        assert err <= self.gap, (tag, err, self.gap)

    def same_points(self, got_labels, graph, tag, stats):
        assert np.array_equal(got_labels[0], self.z[tag + "_weak_sem"]) and got_labels[0].dtype == np.float64
        assert np.array_equal(got_labels[1], self.z[tag + "_weak_ins"]) and got_labels[1].dtype == np.float64
        assert np.array_equal(np.asarray(graph.vs["instance_voxel_num"]), self.z[tag + "_voxel_num"]), tag
        err = np.abs(np.asarray(graph.vs["instance_size"], dtype=np.float64) - self.z[tag + "_size"]).max()
        assert err <= self.gap, (tag, err, self.gap)
        assert [stats[k] for k in wl.STAT_NAMES] == self.z[tag + "_counters"].tolist(), tag


def check_stages(gold, mod, statistics):
    """every stage of ``mod`` (the oracle, or the device module) on the stored inputs against the reference's results"""
    z, scene, g0 = gold.z, gold.scene, gold.g0
    before = (g0.vs["semantic_label"].copy(), g0.vs["superpoint_offset_vector"].copy(), g0.is1ins.copy())
    g1 = mod.extend_label_to_neighbor(scene, g0, z["conf"], z["pred"], gold.thr)
    gold.same_graph(g1, "g1")
    assert (np.asarray(g1.vs["semantic_label"]) != g0.vs["semantic_label"]).any()
    gold.same_graph(mod.propagate_label_to_neighbor(scene, g1, z["pred"]), "gn")
    g2 = mod.apply_propagated_labels(scene, g0, z["plf"])
    gold.same_graph(g2, "g2")
    g3, info = mod.propagate_label_to_whole_scene(scene, g0, z["pred"], z["pred_off"], gold.max_dist, return_info=True)
    gold.same_graph(g3, "g3", is1ins=False)
    assert np.array_equal(g3.is1ins, g0.is1ins)                       # this stage leaves is1ins alone
    assert np.array_equal(info["prior"], z["ws_prior"]) and np.array_equal(info["assigned"], z["ws_assigned"])
    has = np.isfinite(z["ws_dist"])
    assert np.array_equal(np.isfinite(info["dist"]), has)
    assert np.abs(info["dist"][has] - z["ws_dist"][has]).max() <= gold.gap
    for tag, g, flags in (("p1", g1, (False, False)), ("p2", g2, (False, False)), ("p3", g3, (True, True))):
        labels = mod.generate_point_level_weak_label(scene, g, *flags)
        gold.same_points(labels, g, tag, statistics(labels[0], labels[1], z["sem_gt"], z["ins_gt"]))
    # the inputs are left as they were
    assert np.array_equal(g0.vs["semantic_label"], before[0]) and np.array_equal(g0.is1ins, before[2])
    assert np.array_equal(g0.vs["superpoint_offset_vector"], before[1])


@pytest.mark.parametrize("tag", ["a", "b"])
def test_fixture_keeps_its_margins_and_covers_every_outcome(tag):
    gold = Golden(tag)
    z = gold.z
    assert gold.gap == wl.gap_bound(z["xyz"], z["superpoint"]) and len(z["xyz"]) <= 12000
    assert gold.max_dist == {"a": 0.9, "b": 1.2}[tag]
    assert (np.abs(z["conf"].astype(np.float64) - gold.thr) > 1e-6).all() and z["conf"].dtype == np.float32
    has, two = np.isfinite(z["ws_dist"]), np.isfinite(z["ws_second"])
    assert np.abs(z["ws_dist"][has] - gold.max_dist).min() > gold.gap
    assert (z["ws_second"][two] - z["ws_dist"][two]).min() > gold.gap
    lab = wl.labelled(z["g0_sem"], z["g0_ins"])
    n_open = int((~lab).sum())
    assigned, far = z["ws_assigned"] >= 0, has & (z["ws_assigned"] < 0)
    for n in (assigned.sum(), far.sum(), n_open - has.sum()):
        assert 10 * int(n) >= n_open
    _, n_ins = wl.neighbor_source(z["edges"], z["g0_sem"], z["g0_ins"], z["pred"], z["conf"], gold.thr)
    assert (n_ins >= 2).any()                                         # the largest-id rule decides somewhere
    assert (z["p3_voxel_num"] > 0).all() and (z["p3_size"] > 0).any() and not z["p1_voxel_num"].any()


@pytest.mark.parametrize("tag", ["a", "b"])
def test_oracle_reproduces_the_reference(tag):
    check_stages(Golden(tag), wl, wl.statistics)


def test_oracle_margins_equal_the_recorded_ones():
    gold = Golden("a")
    z = gold.z
    res = wl.whole_scene(z["g0_sem"], z["g0_ins"], z["g0_off"], gold.scene.centre, gold.scene.sum, gold.scene.count,
                         z["pred"], z["pred_off"], gold.max_dist)
    m1, m2 = wl.whole_scene_margin(res, gold.max_dist)
    assert m1 > gold.gap and m2 > gold.gap
    two = np.isfinite(z["ws_second"])
    assert np.array_equal(np.isfinite(res["second"]), two)
    assert np.abs(res["second"][two] - z["ws_second"][two]).max() <= gold.gap


def test_oracle_occupancy_against_a_brute_force_count_per_label():
    rng = np.random.default_rng(5)
    N, S = 3000, 40
    xyz = ((rng.random((N, 3)) - 0.5) * 0.8).astype(np.float32)      # negative coordinates: truncation, not floor
    sp = rng.integers(0, S, N)
    sp[:S] = np.arange(S)
    sem = rng.integers(0, 5, S)
    ins = rng.integers(0, 6, S)
    sem[rng.random(S) < 0.3] = -100                                   # unlabelled with an instance label of their own
    ins[rng.random(S) < 0.2] = -100
    ins[7], sem[7] = 77, -100                                         # a label no point carries
    got = wl.occupancy(xyz, sp, sem, ins, 50)
    _, point_ins = wl.point_labels(sp, sem, ins)
    vox = (xyz * np.float32(50)).astype(np.int64)                     # astype truncates toward zero
    assert (vox != np.floor(xyz * np.float32(50)).astype(np.int64)).any()
    for v in range(S):
        mask = point_ins == ins[v]
        want = len(np.unique(vox[mask], axis=0)) if mask.any() else 0
        assert got[v] == want, v
    assert got[7] == 0 and got[ins == -100].min() > 0


def test_new_symbols_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "wsis_hip.h")).read()
    lib = ctypes.CDLL(os.path.join(ROOT, "3d-wsis_amd", "libwsis_hip.so"))
    _, hip_names = wsis_native.declared_symbols()
    for name in NEW_SYMBOLS:
        assert name + "(" in text and hasattr(lib, name) and name in hip_names
        assert getattr(wsis_native.hip(), name).argtypes is not None
    assert sorted(n for n in hip_names if n.startswith("wsis_wl_")) == sorted(NEW_SYMBOLS)
    assert "scannetv2_dataset.py:515-964" in text
    q = wsis_native.hip().wsis_wl_occupancy_workspace_bytes
    assert q(-1) < 0 and q(0) > 0          # N > 0 asks the device sort for its scratch size: test_gpu_weak_labels.py


def test_a_superpoint_without_points_is_refused():
    import wsis_weak_labels
    xyz = np.zeros((5, 3), np.float32)
    with pytest.raises(ValueError):
        wsis_weak_labels.WeakLabelScene(xyz, np.array([0, 1, 3, 3, 1]))              # id 2 is empty
    with pytest.raises(ValueError):
        wsis_weak_labels.WeakLabelScene(xyz, np.array([0, 1, 2, 2, 1]), n_superpoints=4)
    with pytest.raises(ValueError):
        wl.Scene(xyz, np.array([0, 1, 3, 3, 1]))


def test_a_cpu_device_is_refused():
    import wsis_weak_labels
    xyz = np.zeros((5, 3), np.float32)
    with pytest.raises(wsis_native.WsisError):
        wsis_weak_labels.WeakLabelScene(xyz, np.array([0, 1, 2, 2, 1]), device="cpu")
    with pytest.raises(wsis_native.WsisError):
        wsis_weak_labels.weak_label_statistics(np.zeros(4), np.zeros(4), np.zeros(4), np.zeros(4), device="cpu")
