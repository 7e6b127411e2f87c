"""The device l0 cut-pursuit solver (wsis_partition.cut_pursuit, csrc/cutpursuit.hip) on the C1 room of bench.py
(harness.make_scene(0, room = 3.0 x 3.0 x 2.4 m, two boxes)) sampled at 1 M points, as tools/partition_bench.py samples it:
the time of every stage between device events summed over one solve (the host's read-backs between launches fall inside
the stage they belong to), the rounds every min cut took, the main iterations, the whole solve and the whole
``generate_superpoints`` (median of --iters), and the numpy / scipy restatement (tests/cut_pursuit_ref.py) once on the
first --ref-voxels voxels of the room and the edges among them, with the device on the same subgraph, for scale.  The
reference's own solver (Boost.Graph) cannot be built there, so no speed target is set.  Not a test: no threshold.

    python tools/cut_pursuit_bench.py [--out profiles/cut_pursuit_bench.json]
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

import cut_pursuit_ref as cp  # noqa: E402
import harness  # noqa: E402
import wsis_partition as wp  # noqa: E402

C1_ROOM = (3.0, 3.0, 2.4)
LAMBDA = 0.03


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
    return round(statistics.median(times), 3), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--ref-voxels", type=int, default=20000, help="voxels of the restatement's subgraph (0: skip it)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cut_pursuit_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cut_pursuit_bench needs the MI355X")
    sc = harness.make_scene(0, room=C1_ROOM, n_box=2, voxel=0.006, max_points=args.points)
    xyz = torch.from_numpy(np.ascontiguousarray(sc["xyz"].astype(np.float32))).cuda()
    rgb = torch.from_numpy(np.ascontiguousarray(((sc["rgb"] + 1.0) * 127.5).astype(np.uint8))).cuda()
    inputs = wp.partition_inputs(xyz, rgb)
    f = torch.nan_to_num(inputs.features)
    graph = (f, inputs.source, inputs.target, inputs.edge_weight)
    wp.cut_pursuit(*graph, LAMBDA)                                      # code objects, allocator
    _, ids, run = wp.cut_pursuit(*graph, LAMBDA, info=True, _timed=True)
    solve_ms, _ = timed(lambda: wp.cut_pursuit(*graph, LAMBDA), args.iters, args.warmup)
    whole_ms, _ = timed(lambda: wp.generate_superpoints(xyz, rgb), args.iters, args.warmup)
    res = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "reg_strength": LAMBDA,
           "room": {"points": int(xyz.shape[0]), "voxels": int(f.shape[0]), "edges": int(inputs.source.numel())},
           "stage_ms_one_solve": {k: round(v, 3) for k, v in run.times.items()},
           "main_iterations": len(run.components), "stopped": run.stopped, "components": run.components,
           "saturated_nodes": run.saturated, "energy": [a + b for a, b in zip(run.fidelity, run.penalty)],
           "flow_rounds_per_min_cut": run.flow_rounds, "flow_round_cap": wp.FLOW_ROUND_CAP,
           "cut_pursuit_ms": solve_ms, "generate_superpoints_ms": whole_ms}
    if args.ref_voxels:
        n = min(args.ref_voxels, int(f.shape[0]))
        s, t = inputs.source.cpu().numpy(), inputs.target.cpu().numpy()
        keep = (s < n) & (t < n)
        sub = (f[:n].cpu().numpy(), s[keep], t[keep], inputs.edge_weight.cpu().numpy()[keep])
        t0 = time.perf_counter()
        comp, ref_run = cp.solve(*sub, LAMBDA, 0)
        ref_ms = (time.perf_counter() - t0) * 1e3
        sub_dev = tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in sub)
        dev_ms, (_, sub_ids) = timed(lambda: wp.cut_pursuit(*sub_dev, LAMBDA), args.iters, args.warmup)
        res["restatement_subgraph"] = {
            "voxels": n, "edges": int(keep.sum()), "restatement_ms_once": round(ref_ms, 1), "device_ms": dev_ms,
            "restatement_energy": sum(cp.energy(*sub, LAMBDA, comp)), "restatement_components": ref_run["components"][-1],
            "device_energy": sum(cp.energy(*sub, LAMBDA, sub_ids.cpu().numpy())),
            "device_components": int(sub_ids.max()) + 1}
    text = json.dumps(res, indent=1)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
