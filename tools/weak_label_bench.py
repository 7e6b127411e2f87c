"""Weak-label stage updates on the MI355X (3d-wsis_amd/wsis_weak_labels.py, csrc/weaklabel.hip) on the C2-shaped scene
of harness.bench_scene (mesh graph, sp_cell = 0.19): device-event time of one call of each of the four stage functions
-- extend_label_to_neighbor, apply_propagated_labels, propagate_label_to_whole_scene and
generate_point_level_weak_label with both signals -- plus the scene set-up and the statistics pass; median of --iters
calls after --warmup.  A call ends with the copy of its results to the host, so the events span upload, kernels and
read-back.  The numpy oracle of tests/weak_label_ref.py runs on the same inputs on this machine's host: the only
stand-in available here for the reference's mask-per-superpoint form.  Not a test: no threshold.

    python tools/weak_label_bench.py [--out profiles/weak_label_bench.json]
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

import harness  # noqa: E402
import weak_label_ref as wl  # noqa: E402
import wsis_datasets  # noqa: E402
import wsis_weak_labels as dev  # noqa: E402


def event_ms(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return round(statistics.median(times), 3)


def host_ms(fn, iters=3):
    times = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return round(statistics.median(times) * 1e3, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "weak_label_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("weak_label_bench needs the MI355X: a CPU run measures nothing")
    sc = harness.bench_scene(args.seed)
    tup, graph = wsis_datasets.synthetic_scene_to_reference_format(sc)
    xyz, sp, S = tup[0], tup[4], sc["S"]
    rng = np.random.default_rng(args.seed)
    truth = harness.synthetic_predictions(sc, args.seed)[0]
    pred = np.where(rng.random(S) < 0.25, rng.integers(0, 20, S), truth)
    graph.vs["semantic_label"] = np.where(sc["sp_sem"] != -100, truth, -100)      # priors agree with the predictions
    conf = rng.random(S).astype(np.float32)
    pred_off = (sc["sp_offset"] + rng.normal(0, 0.25, (S, 3))).astype(np.float32)
    prior = np.nonzero(sc["sp_sem"] != -100)[0]
    plf = np.where((rng.random(S) < 0.3) & (sc["sp_sem"] == -100), prior[rng.integers(0, len(prior), S)], -100.0)
    sem_gt, ins_gt = truth[sp].astype(np.float64), sc["ins_label"].astype(np.float64)

    scene, ref = dev.WeakLabelScene(xyz, sp), wl.Scene(xyz, sp)
    g3 = dev.propagate_label_to_whole_scene(scene, graph, pred, pred_off)
    lab = dev.generate_point_level_weak_label(scene, g3.copy(), True, True)
    calls = {
        "scene_setup": (lambda: dev.WeakLabelScene(xyz, sp), lambda: wl.Scene(xyz, sp)),
        "extend_label_to_neighbor": (lambda: dev.extend_label_to_neighbor(scene, graph, conf, pred),
                                     lambda: wl.extend_label_to_neighbor(ref, graph, conf, pred)),
        "apply_propagated_labels": (lambda: dev.apply_propagated_labels(scene, graph, plf),
                                    lambda: wl.apply_propagated_labels(ref, graph, plf)),
        "propagate_label_to_whole_scene": (lambda: dev.propagate_label_to_whole_scene(scene, graph, pred, pred_off),
                                           lambda: wl.propagate_label_to_whole_scene(ref, graph, pred, pred_off)),
        "generate_point_level_weak_label": (lambda: dev.generate_point_level_weak_label(scene, g3, True, True),
                                            lambda: wl.generate_point_level_weak_label(ref, g3, True, True)),
        "generate_point_level_weak_label_no_signals": (lambda: dev.generate_point_level_weak_label(scene, g3),
                                                       lambda: wl.generate_point_level_weak_label(ref, g3)),
        "weak_label_statistics": (lambda: dev.weak_label_statistics(lab[0], lab[1], sem_gt, ins_gt),
                                  lambda: wl.statistics(lab[0], lab[1], sem_gt, ins_gt)),
    }
    res = {"device": torch.cuda.get_device_name(0), "scene": {"points": int(len(xyz)), "superpoints": int(S),
                                                              "edges": int(len(graph.edges)), "priors": int(len(prior))},
           "iters": args.iters, "ms_per_call": {}}
    for name, (on_device, on_host) in calls.items():
        res["ms_per_call"][name] = {"device_events": event_ms(on_device, args.warmup, args.iters),
                                    "numpy_oracle_host": host_ms(on_host)}
    g3_ref = wl.propagate_label_to_whole_scene(ref, graph, pred, pred_off)
    res["labels_equal_oracle"] = bool(np.array_equal(g3.vs["instance_label"], g3_ref.vs["instance_label"]))
    text = json.dumps(res, indent=1)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
