"""The S3DIS partition front end on the MI355X (wsis_partition, csrc/partition.hip) on the C1 room of bench.py
(harness.make_scene(0, room = 3.0 x 3.0 x 2.4 m, two boxes)) sampled at 1 M points (surface voxels of 6 mm instead of
the 10 k points of the bench leg), colours mapped to uint8: every stage and the whole ``partition_inputs`` between two
device events, median of --iters, next to the numpy oracle's stages (tests/partition_ref.py: cKDTree, eigh) once on the
same machine's host, for scale.  The reference's own stages (boost-python, Eigen, sklearn inside libply_c) cannot run
there, so no speed target is set.  For the k-NN kernel the mean number of candidates evaluated per query and the share
of queries that scanned every point are reported, with the cell edge ``partition_inputs`` uses (3 voxel widths) and with
the automatic one.  Not a test: no threshold.

    python tools/partition_bench.py [--out profiles/partition_bench.json]
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
import partition_ref as ref  # noqa: E402
import wsis_partition as wp  # noqa: E402

C1_ROOM = (3.0, 3.0, 2.4)
VOXEL, K_ADJ, K_GEOF = 0.03, 10, 45


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
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--no-oracle", action="store_true", help="skip the numpy oracle")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "partition_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("partition_bench needs the MI355X: a CPU run measures only the oracle")
    sc = harness.make_scene(0, room=C1_ROOM, n_box=2, voxel=0.006, max_points=args.points)
    xyz_h = np.ascontiguousarray(sc["xyz"].astype(np.float32))
    rgb_h = np.ascontiguousarray(((sc["rgb"] + 1.0) * 127.5).astype(np.uint8))
    xyz, rgb = torch.from_numpy(xyz_h).cuda(), torch.from_numpy(rgb_h).cuda()
    it, wu = args.iters, args.warmup
    dev, host = {}, {}
    dev["prune"], pr = timed(lambda: wp.prune(xyz, VOXEL, rgb), it, wu)
    cell = wp.CELL_VOXELS * VOXEL
    dev["knn_k45"], nn = timed(lambda: wp.knn(pr.xyz, K_GEOF, cell=cell), it, wu)
    dev["knn_k45_automatic_cell"], _ = timed(lambda: wp.knn(pr.xyz, K_GEOF), it, wu)
    dev["knn_k10"], _ = timed(lambda: wp.knn(pr.xyz, K_ADJ, cell=cell), it, wu)
    dev["geometric_features"], gf = timed(lambda: wp.geometric_features(pr.xyz, nn.nbr), it, wu)
    dev["edge_features"], _ = timed(lambda: wp.edge_features(gf.geof, pr.rgb, nn, K_ADJ, 1.), it, wu)
    dev["partition_inputs"], out = timed(lambda: wp.partition_inputs(xyz, rgb), it, wu)
    knn_stats = {}
    for name, c in (("cell_3_voxels", cell), ("automatic_cell", 0.0)):
        st = wp.knn(pr.xyz, K_GEOF, cell=c, stats=True)[1].cpu().numpy()
        knn_stats[name] = {"candidates_per_query": round(float(st[:, 0].mean()), 1),
                           "share_scanning_every_point": round(float(st[:, 1].mean()), 6)}
    if not args.no_oracle:
        host["oracle_prune"], opr = host_once(lambda: ref.prune(xyz_h, VOXEL, rgb_h))
        host["oracle_knn_k45"], (onbr, od2) = host_once(lambda: ref.knn(opr["xyz"], K_GEOF))
        host["oracle_geof"], og = host_once(lambda: ref.geof(opr["xyz"], onbr))
        host["oracle_assemble"], _ = host_once(lambda: ref.assemble(og["geof"], opr["rgb"], onbr, od2, K_ADJ))
        assert np.array_equal(out.p2v.cpu().numpy().astype(np.uint32), opr["p2v"])
        assert np.array_equal(out.target_geof.cpu().numpy(), onbr)
    res = {"device": torch.cuda.get_device_name(0), "iters": it,
           "room": {"points": int(len(xyz_h)), "voxels": int(pr.xyz.shape[0]), "edges": int(out.source.numel()),
                    "voxel_width": VOXEL, "k_nn_adj": K_ADJ, "k_nn_geof": K_GEOF},
           "device_ms_per_call": dev, "knn_k45": knn_stats, "host_ms_once": host}
    text = json.dumps(res, indent=1)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
