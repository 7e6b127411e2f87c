"""GPU: the weak-label stage updates (3d-wsis_amd/wsis_weak_labels.py, csrc/weaklabel.hip) against

* what the reference computed (tests/golden/weak_label_golden.npz): the same comparisons as tests/test_weak_label_host.py
  makes for the numpy oracle -- labels, is1ins, assigned prior, voxel counts, point labels and counters equal, offsets,
  distances and sizes within the stored GAP -- and the whole chain with ``wsis_ops.weak_label_propagation`` in it;
* the numpy oracle (tests/weak_label_ref.py) on synthetic inputs at the kernels' own edges.  Every such comparison first
  asserts, on the ORACLE's distances, that no decision is closer than GAP to its threshold (the case generator takes the
  first seed for which that holds), then wants discrete results equal, floats within GAP and a second call bit-identical;
* a memory condition: no call may allocate anything of the order of S x N.
"""
import numpy as np
import pytest
import torch

import weak_label_ref as wl
from test_weak_label_host import Golden, check_stages
from wsis_datasets import PlainGraph

pytestmark = pytest.mark.gpu

MAX_DIST = 0.9
CHUNK = 256                     # WL_PC of csrc/weaklabel.hip: priors staged in LDS at a time
NO_PRIOR_CLASS = 4              # predicted, never labelled


def dev():
    import wsis_weak_labels
    return wsis_weak_labels


# ---- against the reference's results -------------------------------------------------------------------------------

@pytest.mark.parametrize("tag", ["a", "b"])
def test_device_reproduces_the_reference(tag):
    check_stages(Golden(tag, scene_cls=dev().WeakLabelScene), dev(), dev().weak_label_statistics)


def test_whole_chain_with_the_device_propagation():
    """extend -> generate -> wsis_ops.weak_label_propagation -> apply -> generate -> whole scene -> generate (both
    signals), every step against the reference's result of the same step"""
    import wsis_ops
    m, gold = dev(), Golden("a", scene_cls=dev().WeakLabelScene)
    z, scene, g0 = gold.z, gold.scene, gold.g0
    S = scene.S
    stats = lambda lab: m.weak_label_statistics(lab[0], lab[1], z["sem_gt"], z["ins_gt"])      # noqa: E731
    g1 = m.extend_label_to_neighbor(scene, g0, z["conf"], z["pred"], gold.thr)
    gold.same_graph(g1, "g1")
    lab = m.generate_point_level_weak_label(scene, g1)
    gold.same_points(lab, g1, "p1", stats(lab))
    eu, ev = (torch.from_numpy(np.ascontiguousarray(z["edges"][:, j])).cuda() for j in (0, 1))
    A = wsis_ops.affinity_matrix(eu, ev, torch.from_numpy(z["aff"]).cuda(), S)
    adjacency = torch.zeros((S, S), dtype=torch.int32, device="cuda")
    adjacency[eu, ev] = 1
    plf, _ = wsis_ops.weak_label_propagation(A, adjacency, z["conf"], z["pred"], g0.vs["semantic_label"],
                                             gold.iterations, gold.classes)
    assert np.array_equal(plf, z["plf"]) and (plf != -100).any()
    g2 = m.apply_propagated_labels(scene, g0, plf)
    gold.same_graph(g2, "g2")
    lab = m.generate_point_level_weak_label(scene, g2)
    gold.same_points(lab, g2, "p2", stats(lab))
    g3 = m.propagate_label_to_whole_scene(scene, g0, z["pred"], z["pred_off"], gold.max_dist)
    gold.same_graph(g3, "g3", is1ins=False)
    lab = m.generate_point_level_weak_label(scene, g3, add_occupancy_signal=True, add_instance_size_signal=True)
    gold.same_points(lab, g3, "p3", stats(lab))


# ---- against the oracle at the kernels' edges ------------------------------------------------------------------------

def build_case(S, P, seed, big=False, edges="dup"):
    """Random scene with S superpoints of which P are labelled (priors), coordinates in [-2, 2]^3 (negative voxels).
    Superpoint sizes: 1 for the first two (they become twin priors at one point when P >= 2), then -- ``big`` -- 63, 64, 65
    and 700 points (more than a workgroup), else 2..8.  Classes 0..3 carry priors, class 4 is only ever predicted.  With
    S >= 8 one unlabelled vertex has an instance label no point carries, one has a semantic label alone."""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(2, 9, S)
    sizes[:2] = 1
    if big and S >= 8:
        sizes[2:6] = (63, 64, 65, 700)
    sp = np.repeat(np.arange(S), sizes)
    centre = rng.uniform(-2, 2, (S, 3))
    if S >= 2:
        centre[1] = centre[0]                                     # the twins: identical points
    xyz = (centre[sp] + rng.uniform(-0.1, 0.1, (len(sp), 3)) * (sizes[sp] > 1)[:, None]).astype(np.float32)
    perm = rng.permutation(len(sp))
    xyz, sp = xyz[perm], sp[perm]
    sem, ins = np.full(S, -100, dtype=np.int64), np.full(S, -100, dtype=np.int64)
    off = np.zeros((S, 3))
    prior = np.sort(np.concatenate([np.arange(min(P, 2)), 2 + rng.choice(max(S - 2, 0), max(P - 2, 0), replace=False)]))
    prior = prior[:P].astype(np.int64)
    sem[prior] = rng.integers(0, NO_PRIOR_CLASS, len(prior))
    ins[prior] = 1000 + np.arange(len(prior))
    off[prior] = rng.normal(0, 0.2, (len(prior), 3))
    if P >= 2:
        sem[1], off[1] = sem[0], off[0]                           # same class, same instance centre: index 0 must win
    rest = np.setdiff1d(np.arange(S), prior)
    if S >= 8 and len(rest) >= 2:
        ins[rest[0]] = 555                                        # carried by no point: voxel count 0
        sem[rest[1]] = 2                                          # a semantic label alone does not make it labelled
    pred = rng.integers(0, NO_PRIOR_CLASS + 1, S)
    conf = rng.random(S).astype(np.float32)
    conf[np.abs(conf.astype(np.float64) - 0.8) <= 1e-6] = 0.5
    pred_off = rng.normal(0, 0.3, (S, 3)).astype(np.float32)
    near_twin = -1
    if P >= 2 and len(rest) >= 3:                                 # one superpoint predicted onto the twins' centre
        near_twin = int(rest[2])
        pred[near_twin] = sem[0]
        pred_off[near_twin] = (centre[0] + off[0] - centre[near_twin] + 0.01).astype(np.float32)
    if edges == "none" or S < 2:
        e = np.zeros((0, 2), dtype=np.int64)
    else:
        a = rng.integers(0, S, 4 * S)
        b = rng.integers(0, S, 4 * S)
        e = np.stack([a, b], 1)[a != b]
        e = np.concatenate([e, e[:, ::-1], e[:3]])                # both directions, and duplicates
    graph = PlainGraph({"v": np.arange(S), "semantic_label": sem, "instance_label": ins, "superpoint_offset_vector": off,
                        "instance_voxel_num": np.zeros(S, np.int64), "instance_size": np.zeros(S)}, e)
    plf = np.full(S, -100.0)
    if len(prior):
        take = rest[rng.random(len(rest)) < 0.5]
        plf[take] = prior[rng.integers(0, len(prior), len(take))]
    return dict(xyz=xyz, sp=sp, graph=graph, pred=pred, conf=conf, pred_off=pred_off, plf=plf, S=S, P=P, near_twin=near_twin,
                sem_gt=rng.integers(0, 5, len(sp)).astype(np.float64),
                ins_gt=(1000 + rng.integers(0, max(P, 1), len(sp))).astype(np.float64))


def case_with_margin(S, P, big=False, edges="dup"):
    """the first seed whose oracle distances keep every decision further than GAP from its threshold"""
    for seed in range(1000 * S + P, 1000 * S + P + 200):
        c = build_case(S, P, seed, big, edges)
        c["gap"] = wl.gap_bound(c["xyz"], c["sp"])
        c["ref_scene"] = wl.Scene(c["xyz"], c["sp"], n_superpoints=S)
        _, res = wl.propagate_label_to_whole_scene(c["ref_scene"], c["graph"], c["pred"], c["pred_off"], MAX_DIST, True)
        m1, m2 = wl.whole_scene_margin(res, MAX_DIST)
        if m1 > c["gap"] and m2 > c["gap"]:
            c["margins"] = (m1, m2)
            return c
    raise AssertionError("no seed keeps the margin")


def graphs_equal(a, b, gap, bitwise=False):
    for k in ("semantic_label", "instance_label", "instance_voxel_num"):
        assert np.array_equal(np.asarray(a.vs[k]).astype(np.int64), np.asarray(b.vs[k]).astype(np.int64)), k
    assert np.array_equal(a.is1ins, b.is1ins) and np.array_equal(a.edges, b.edges)
    for k in ("superpoint_offset_vector", "instance_size"):
        x, y = np.asarray(a.vs[k], dtype=np.float64), np.asarray(b.vs[k], dtype=np.float64)
        if bitwise:
            assert np.array_equal(x, y), k
        elif x.size:
            assert np.abs(x - y).max() <= gap, (k, np.abs(x - y).max(), gap)


def run_all(mod, scene, c, statistics):
    """every stage once -> (graphs by name, whole-scene info, point labels, counters)"""
    g = c["graph"]
    out = {"extend": mod.extend_label_to_neighbor(scene, g, c["conf"], c["pred"], 0.8),
           "neighbor": mod.propagate_label_to_neighbor(scene, g, c["pred"]),
           "apply": mod.apply_propagated_labels(scene, g, c["plf"])}
    out["whole"], info = mod.propagate_label_to_whole_scene(scene, g, c["pred"], c["pred_off"], MAX_DIST, return_info=True)
    labels = mod.generate_point_level_weak_label(scene, out["whole"], True, True)
    return out, info, labels, statistics(labels[0], labels[1], c["sem_gt"], c["ins_gt"], (0, 1))


def compare_with_oracle(c):
    m = dev()
    m1, m2 = c["margins"]
    assert m1 > c["gap"] and m2 > c["gap"]                           # the oracle's own distances decide nothing narrowly
    scene = m.WeakLabelScene(c["xyz"], c["sp"], n_superpoints=c["S"])
    ref = c["ref_scene"]
    assert np.array_equal(scene.count.cpu().numpy(), ref.count)
    assert np.abs(scene.centre.cpu().numpy().astype(np.float64) - ref.centre).max() <= c["gap"]
    before = c["graph"].copy()
    want, want_info, want_labels, want_stats = run_all(wl, ref, c, wl.statistics)
    got, info, labels, stats = run_all(m, scene, c, m.weak_label_statistics)
    graphs_equal(c["graph"], before, 0.0, bitwise=True)              # the input graph is left alone
    for k in want:
        graphs_equal(got[k], want[k], c["gap"])
    assert np.array_equal(info["prior"], want_info["prior"]) and np.array_equal(info["assigned"], want_info["assigned"])
    has = np.isfinite(want_info["dist"])
    assert np.array_equal(np.isfinite(info["dist"]), has)
    if has.any():
        assert np.abs(info["dist"][has] - want_info["dist"][has]).max() <= c["gap"]
    assert np.array_equal(labels[0], want_labels[0]) and np.array_equal(labels[1], want_labels[1])
    assert stats == want_stats and stats["GT_all"] == len(c["sp"])
    # a second call: bit-identical, floats included
    scene2 = m.WeakLabelScene(c["xyz"], c["sp"], n_superpoints=c["S"])
    for a, b in ((scene.sum, scene2.sum), (scene.centre, scene2.centre)):
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy())
    again, info2, labels2, stats2 = run_all(m, scene2, c, m.weak_label_statistics)
    for k in got:
        graphs_equal(again[k], got[k], 0.0, bitwise=True)
    assert np.array_equal(info2["dist"], info["dist"]) and np.array_equal(info2["assigned"], info["assigned"])
    assert np.array_equal(labels2[0], labels[0]) and np.array_equal(labels2[1], labels[1]) and stats2 == stats
    return got, info, want_info


@pytest.mark.parametrize("S,P", [(1, 0), (1, 1), (63, 2), (64, 5), (65, 3), (257, 40)])
def test_superpoint_counts_around_the_wave_and_block_sizes(S, P):
    c = case_with_margin(S, P, big=True, edges="none" if S == 1 else "dup")
    got, info, _ = compare_with_oracle(c)
    if S >= 8:
        n = np.bincount(c["sp"])
        assert sorted(n[2:6].tolist()) == [63, 64, 65, 700] and (n[:2] == 1).all()
        assert (c["xyz"] < 0).any() and info["assigned"][c["near_twin"]] == 0      # P >= 2: the twins' neighbour joins
        vox = np.asarray(got["whole"].vs["instance_voxel_num"])
        assert (vox[np.asarray(got["whole"].vs["instance_label"]) == 555] == 0).all() and (vox > 0).any()


@pytest.mark.parametrize("P", [0, 1, 2, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 188])
def test_prior_counts_around_the_lds_chunk(P):
    c = case_with_margin(P + 90, P)
    got, info, want = compare_with_oracle(c)
    if P == 0:
        assert (info["assigned"] == -1).all() and not np.isfinite(info["dist"]).any()
        return
    lab = wl.labelled(c["graph"].vs["semantic_label"], c["graph"].vs["instance_label"])
    open_ = ~lab
    assert (info["assigned"][lab] == -1).all()
    no_prior = open_ & (c["pred"] == NO_PRIOR_CLASS)
    assert no_prior.any() and not np.isfinite(info["dist"][no_prior]).any()          # a class without priors
    if P >= 2:
        # priors 0 and 1 are twins (one point, one class, one offset): equal distances, the first index wins
        assert (info["assigned"] != 1).all() and info["assigned"][c["near_twin"]] == 0
    if P > CHUNK:
        assert (info["assigned"] >= CHUNK).any() and ((info["assigned"] >= 0) & (info["assigned"] < CHUNK)).any()
    far = open_ & np.isfinite(info["dist"]) & (info["assigned"] < 0)
    if P >= CHUNK - 1:
        assert (info["dist"][far] > MAX_DIST).all() and (info["dist"][info["assigned"] >= 0] < MAX_DIST).all()


def test_graph_without_edges_and_with_duplicates():
    c = case_with_margin(120, 30, edges="none")
    got, _, _ = compare_with_oracle(c)
    assert got["extend"].is1ins.shape == (0,)
    assert np.array_equal(got["extend"].vs["semantic_label"], c["graph"].vs["semantic_label"])
    c = case_with_margin(120, 30, edges="dup")
    got, _, _ = compare_with_oracle(c)
    assert (np.asarray(got["extend"].vs["semantic_label"]) != c["graph"].vs["semantic_label"]).any()
    assert (np.asarray(got["neighbor"].vs["semantic_label"]) != np.asarray(got["extend"].vs["semantic_label"])).any()
    _, n_ins = wl.neighbor_source(c["graph"].edges, c["graph"].vs["semantic_label"], c["graph"].vs["instance_label"],
                                  c["pred"])
    assert (n_ins >= 2).any()                                        # the largest-id rule decided somewhere


def test_workspace_query_grows_with_n():
    import wsis_native
    q = wsis_native.hip().wsis_wl_occupancy_workspace_bytes
    assert 0 < q(0) <= q(1000) <= q(200000) and q(200000) < 100 * 200000 + (16 << 20)


def test_no_call_allocates_anything_like_s_times_n():
    """N = 200,000 points, S = 3,000 superpoints: the peak device allocation above what is allocated when a call starts
    stays below 100 N bytes + 16 MiB for every function (one S x N byte mask would be 600 MB)"""
    m = dev()
    N, S = 200000, 3000
    rng = np.random.default_rng(11)
    sp = rng.integers(0, S, N)
    sp[:S] = np.arange(S)
    xyz = rng.uniform(-3, 3, (N, 3)).astype(np.float32)
    sem, ins = np.full(S, -100, dtype=np.int64), np.full(S, -100, dtype=np.int64)
    prior = rng.choice(S, 300, replace=False)
    sem[prior], ins[prior] = rng.integers(0, 10, 300), np.arange(300)
    e = rng.integers(0, S, (20000, 2))
    graph = PlainGraph({"v": np.arange(S), "semantic_label": sem, "instance_label": ins,
                        "superpoint_offset_vector": rng.normal(0, 0.2, (S, 3)), "instance_voxel_num": np.zeros(S, np.int64),
                        "instance_size": np.zeros(S)}, e)
    pred, conf = rng.integers(0, 10, S), rng.random(S).astype(np.float32)
    pred_off = rng.normal(0, 0.3, (S, 3)).astype(np.float32)
    plf = np.where(rng.random(S) < 0.5, prior[rng.integers(0, 300, S)], -100).astype(np.float64)
    limit = 100 * N + (16 << 20)
    peaks = {}

    def measured(name, fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        peaks[name] = torch.cuda.max_memory_allocated() - base
        return out

    scene = measured("scene", lambda: m.WeakLabelScene(xyz, sp))
    g1 = measured("extend", lambda: m.extend_label_to_neighbor(scene, graph, conf, pred))
    measured("neighbor", lambda: m.propagate_label_to_neighbor(scene, g1, pred))
    measured("apply", lambda: m.apply_propagated_labels(scene, graph, plf))
    g3 = measured("whole", lambda: m.propagate_label_to_whole_scene(scene, graph, pred, pred_off, 1.2))
    lab = measured("generate", lambda: m.generate_point_level_weak_label(scene, g3, True, True))
    stats = measured("statistics", lambda: m.weak_label_statistics(lab[0], lab[1], lab[0], lab[1]))
    print("peak bytes above the start of the call:", peaks, "limit", limit)
    assert max(peaks.values()) < limit, peaks
    assert stats["GT_all"] == N and (np.asarray(g3.vs["semantic_label"]) != sem).any()
    assert np.asarray(g3.vs["instance_voxel_num"]).max() > 0
