"""The superpoint-graph preparation on the MI355X (wsis_graph_prep, csrc/graphprep.hip) on the C2 scene of bench.py
(harness.bench_scene, seed 1; random mesh faces between near points, as the scene has no mesh): every call between two
device events, median of --iters, next to the numpy oracle (tests/graph_prep_ref.py, the reference's mask-per-superpoint
shape) once on the same machine's host.  ``edge_features`` and the two builders include the host-side sampling draws
(one ``RandomState.choice`` per edge, the contract of the reference's random stream); ``edge_features_kernel_only``
reuses drawn samples.  ``reference_builders_ms_fixture_size`` quotes what tests/golden/make_graph_prep_golden.py printed
for the reference's own builders on the fixture scenes (N ~ 6,000, S = 150) on a container CPU: a different size and
machine, recorded for scale only.  Not a test: no threshold.

    python tools/graph_prep_bench.py [--out profiles/graph_prep_bench.json]
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
importlib.import_module("3d-wsis_amd")

import numpy as np  # noqa: E402
import torch  # noqa: E402

import graph_prep_ref as ref  # noqa: E402
import harness  # noqa: E402
import wsis_graph_prep as gp  # noqa: E402

REFERENCE_BUILDERS_MS = {"s3dis_a": 280, "s3dis_b": 276, "scannet_a": 266, "scannet_b": 83}


def timed(fn, iters, warmup):
    times, out = [], None
    for i in range(warmup + iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        if i >= warmup:
            times.append(a.elapsed_time(b))
    return round(statistics.median(times), 4), out


def host_once(fn):
    t0 = time.perf_counter()
    out = fn()
    return round((time.perf_counter() - t0) * 1e3, 1), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--no-oracle", action="store_true", help="skip the numpy oracle (minutes at C2 size)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "graph_prep_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("graph_prep_bench needs the MI355X: a CPU run measures only the oracle")
    sc = harness.bench_scene(args.seed)
    xyz, sp = sc["xyz"].astype(np.float32), sc["superpoint"].astype(np.int64)
    sem, ins = sc["sem_label"].astype(np.float64), sc["ins_label"].astype(np.float64)
    rng = np.random.default_rng(args.seed)
    from scipy.spatial import cKDTree
    pick = rng.choice(len(xyz), min(60000, len(xyz)), replace=False)
    near = cKDTree(xyz).query(xyz[pick], k=8)[1]
    faces = np.stack([pick, near[:, 3], near[:, 7]], 1).astype(np.int64)
    it, wu = args.iters, args.warmup
    dev, host = {}, {}
    dev["GraphScene"], scene = timed(lambda: gp.GraphScene(xyz, sp), it, wu)
    dev["superpoint_features"], ft = timed(lambda: gp.superpoint_features(scene), it, wu)
    dev["superpoint_labels"], _ = timed(lambda: gp.superpoint_labels(scene, sem, ins, ft), it, wu)
    dev["neighbor_lists_k10"], nl = timed(lambda: gp.neighbor_lists(ft.centroid, 10), it, wu)
    dev["neighbor_lists_k16_r0.3"], _ = timed(lambda: gp.neighbor_lists(ft.centroid, 16, 0.3), it, wu)
    dev["face_edges"], _ = timed(lambda: gp.face_edges(faces, scene.superpoint), it, wu)
    g = gp.build_graph_scannet(xyz, faces, sp, sem, ins, np.random.RandomState(args.seed))
    edges = g.edges
    counts = ft.count.cpu().numpy()
    host["draw_samples"], samples = host_once(lambda: gp.draw_samples(counts, edges, np.random.RandomState(args.seed)))
    dev["edge_features_kernel_only"], _ = timed(lambda: gp.edge_features(scene, ft, edges, None, samples=samples), it, wu)
    dev["edge_features"], f = timed(lambda: gp.edge_features(scene, ft, edges, np.random.RandomState(args.seed)), it, 1)
    dev["standardize_features"], _ = timed(lambda: gp.standardize_features(f), it, wu)
    dev["build_graph_s3dis"], g3 = timed(lambda: gp.build_graph_s3dis(xyz, sp, sem, ins, np.random.RandomState(args.seed)),
                                         it, 1)
    dev["build_graph_scannet"], _ = timed(lambda: gp.build_graph_scannet(xyz, faces, sp, sem, ins,
                                                                         np.random.RandomState(args.seed)), it, 1)
    if not args.no_oracle:
        host["oracle_superpoint_features"], oft = host_once(lambda: ref.superpoint_features(xyz, sp))
        host["oracle_superpoint_labels"], _ = host_once(lambda: ref.superpoint_labels(xyz, sp, sem, ins))
        host["oracle_neighbor_lists_k10"], _ = host_once(lambda: ref.neighbor_lists(oft["centroid"], 10))
        host["oracle_edge_features"], _ = host_once(lambda: ref.edge_features(xyz, sp, oft, edges, samples))
    res = {"device": torch.cuda.get_device_name(0), "iters": it,
           "scene": {"points": int(len(xyz)), "superpoints": int(scene.S), "faces": int(len(faces)),
                     "edges_scannet": int(len(edges)), "edges_s3dis": int(len(g3.edges)),
                     "sample_indices": int(len(samples[1]))},
           "device_ms_per_call": dev, "host_ms_once": host,
           "reference_builders_ms_fixture_size": REFERENCE_BUILDERS_MS}
    text = json.dumps(res, indent=1)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
