"""S3DIS wall split on the MI355X: time of one wsis_plane_score call (csrc/plane.hip) and of a whole
inference.get_room_walls, with the numpy oracle of tests/plane_ref.py on the same inputs on this machine's host as the
only available stand-in for open3d's segment_plane.  Not a test: no threshold.

  score     N = 10^5 and 10^6 points of a synthetic room, H = 200 planes from random triples.  Device-event time of one
            call (median of --iters after --warmup) and per call of --batch calls issued back to back inside one pair of
            events (launch latency hidden); achieved fp64 rate = 7 operations per point and plane (3 mul, 3 add, 1
            compare; the kernel also squares and accumulates the inliers) against the 78.6 TFLOP/s vector-fp64 peak of
            the MI355X (a peak counted in fused multiply-adds: the kernel runs uncontracted, so half of it is the ceiling
            for these operations); bytes = 12 per point read once.
  walls     get_room_walls(max_num=10, seed=...) on a 10^6-point room of which 30 % are wall points (four walls):
            host wall-clock time per call including the final copy of the masks (median of --wall-iters).

    python tools/wall_split_bench.py [--out profiles/wall_split_bench.json]
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

import inference  # noqa: E402
import plane_ref  # noqa: E402
import wsis_native as _n  # noqa: E402

FP64_VECTOR_PEAK = 78.6e12       # MI355X, FLOP/s, fused multiply-add = 2
OPS_PER_TEST = 7
ROOM = (10.0, 8.0, 3.0)


def room(n_total, wall_share, seed):
    """fp32 [n_total, 3] and the wall flag: four walls (40 / 27 / 20 / 13 % of the wall points), clutter elsewhere"""
    n_wall = int(n_total * wall_share)
    parts = [int(n_wall * f) for f in (0.40, 0.27, 0.20)]
    parts.append(n_wall - sum(parts))
    walls = plane_ref.make_room(seed, walls=tuple(parts), clutter=0, size=ROOM)
    rng = np.random.default_rng(seed + 1)
    clutter = (rng.random((n_total - n_wall, 3)) * np.array(ROOM)).astype(np.float32)
    flag = np.zeros(n_total, dtype=bool)
    flag[rng.permutation(n_total)[:n_wall]] = True
    xyz = np.empty((n_total, 3), dtype=np.float32)
    xyz[flag], xyz[~flag] = walls, clutter
    return xyz, flag


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
    return statistics.median(times)


def bench_score(N, H, args):
    parts = [int(N * f) for f in (0.4, 0.25, 0.15, 0.1)]
    xyz = plane_ref.make_room(3, walls=tuple(parts), clutter=N - sum(parts), size=ROOM)
    rng = np.random.default_rng(N + H)
    planes, valid = plane_ref.planes_from_triples(xyz[plane_ref.draw_triples(N, H, rng).reshape(-1)].reshape(H, 3, 3))
    assert valid.all()
    xyz_d, planes_d = torch.from_numpy(xyz).cuda(), torch.from_numpy(planes).cuda()
    out = (torch.empty(H, dtype=torch.int64, device="cuda"), torch.empty(H, dtype=torch.float64, device="cuda"))
    ws = torch.empty(int(_n.hip().wsis_plane_score_workspace_bytes(N, H)), dtype=torch.uint8, device="cuda")

    def one():
        inference.plane_score(xyz_d, planes_d, 0.1, out=out, workspace=ws)

    def batch():
        for _ in range(args.batch):
            one()

    single = event_ms(one, args.warmup, args.iters)
    batched = event_ms(batch, 2, args.iters) / args.batch
    t0 = time.perf_counter()
    count, sumsq, gap = plane_ref.score(xyz, planes, 0.1)
    host_s = time.perf_counter() - t0
    same = bool(np.array_equal(out[0].cpu().numpy(), count))
    flops = float(N) * H * OPS_PER_TEST
    return {"N": N, "H": H, "us_per_call_single": round(single * 1e3, 2), "us_per_call_batched": round(batched * 1e3, 2),
            "fp64_tflops": round(flops / (batched * 1e-3) / 1e12, 3),
            "fraction_of_fp64_vector_peak": round(flops / (batched * 1e-3) / FP64_VECTOR_PEAK, 4),
            "read_gbytes_per_s": round(12.0 * N / (batched * 1e-3) / 1e9, 1),
            "numpy_oracle_ms": round(host_s * 1e3, 1), "counts_equal_oracle": same, "oracle_min_gap": gap}


def bench_walls(args):
    xyz, flag = room(args.room_points, 0.30, 11)
    xyz_d, flag_d = torch.from_numpy(xyz).cuda(), torch.from_numpy(flag).cuda()
    times, walls = [], None
    for i in range(args.wall_warmup + args.wall_iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        walls = inference.get_room_walls(xyz_d, flag_d, max_num=10, seed=5)
        dt = time.perf_counter() - t0
        if i >= args.wall_warmup:
            times.append(dt)
    t0 = time.perf_counter()
    want, info = plane_ref.get_room_walls_ref(xyz, flag, max_num=10, seed=5)
    host_s = time.perf_counter() - t0
    same = len(want) == len(walls) and all(np.array_equal(a, b) for a, b in zip(want, walls))
    return {"points": int(len(xyz)), "wall_points": int(flag.sum()), "iter": 200, "max_num": 10,
            "walls": [int(w.sum()) for w in walls], "ms_per_call": round(statistics.median(times) * 1e3, 2),
            "numpy_oracle_ms": round(host_s * 1e3, 1), "masks_equal_oracle": bool(same), "oracle_min_gap": info["gap"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--wall-iters", type=int, default=7)
    ap.add_argument("--wall-warmup", type=int, default=2)
    ap.add_argument("--room-points", type=int, default=10 ** 6)
    ap.add_argument("--sizes", type=int, nargs="+", default=[10 ** 5, 10 ** 6])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wall_split_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("wall_split_bench needs the MI355X: a CPU run measures nothing")
    res = {"device": torch.cuda.get_device_name(0), "fp64_vector_peak_tflops": FP64_VECTOR_PEAK / 1e12,
           "ops_per_point_and_plane": OPS_PER_TEST, "score": [bench_score(N, 200, args) for N in args.sizes],
           "get_room_walls": bench_walls(args)}
    text = json.dumps(res, indent=1)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
