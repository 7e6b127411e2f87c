"""The ScanNet mesh superpoints (wsis_graph_prep.segment_mesh, csrc/meshseg.hip, wsis_host_mesh_merge) on
a synthetic room mesh of about 150 k vertices / 300 k faces: a heightfield floor with box furniture standing on it and a
little vertex noise, seeded.  Per stage of one call (the device drained behind each stage, median of --iters): normals
(face normals, the vertex -> face-slot CSR, vertex normals), weights, sort (stable sort and the gather of the ends),
read-back, host sweeps, upload; the whole call without the drains; and the whole definition on the host alone -- the
same arithmetic vectorised in numpy, numpy's stable argsort and the same host op -- whose ids must equal the device's.
No speed target is set.  Not a test: no threshold.

    python tools/mesh_segment_bench.py [--out profiles/mesh_segment_bench.json]
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
importlib.import_module("3d-wsis_amd")

import numpy as np  # noqa: E402
import torch  # noqa: E402

import wsis_graph_prep as gp  # noqa: E402

F32 = np.float32
STAGES = ("normals", "weights", "sort", "read_back", "host_sweeps", "upload")


def room_mesh(n=390, seed=0, cell=0.02, noise=0.0005, n_box=12):
    """n x n vertices over a (n * cell) m square: a gently rolling floor, ``n_box`` boxes 0.3 .. 0.9 m high standing on
    it (their sides one cell wide), Gaussian vertex noise -> (vertices fp32 [n*n,3], faces int64 [2 (n-1)^2, 3])"""
    rng = np.random.RandomState(seed)
    ix, iy = np.meshgrid(np.arange(n), np.arange(n))
    z = 0.01 * np.sin(ix * cell * 1.3) * np.cos(iy * cell * 0.7)
    for _ in range(n_box):
        x0, y0 = rng.randint(0, n - 60, 2)
        w, d = rng.randint(20, 60, 2)
        z = np.where((ix >= x0) & (ix < x0 + w) & (iy >= y0) & (iy < y0 + d), rng.uniform(0.3, 0.9), z)
    xyz = np.stack([ix * cell, iy * cell, z], -1).reshape(-1, 3) + rng.normal(0, noise, (n * n, 3))
    v = (iy[:-1, :-1] * n + ix[:-1, :-1]).reshape(-1)
    faces = np.concatenate([np.stack([v, v + 1, v + n], 1), np.stack([v + 1, v + n + 1, v + n], 1)])
    return xyz.astype(F32), faces.astype(np.int64)


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _unit(a):
    length = np.sqrt(_dot(a, a))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where((length != 0)[:, None], a / length[:, None], F32(0))


def host_definition(xyz, faces, k_thresh, seg_min_verts):
    """steps 1-8 on the host: fp32 numpy with the operations of the definition in its order (the vertex normals one
    incident slot of every vertex at a time), a stable argsort, wsis_host_mesh_merge"""
    V = len(xyz)
    p1, p2, p3 = xyz[faces[:, 0]], xyz[faces[:, 1]], xyz[faces[:, 2]]
    u, v = p2 - p1, p3 - p1
    fn = _unit(np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2],
                         u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], 1))
    slot_vertex = faces.reshape(-1)
    order = np.argsort(slot_vertex, kind="stable")
    start = np.searchsorted(slot_vertex[order], np.arange(V))
    rank = np.arange(len(order)) - start[slot_vertex[order]]
    vn = np.zeros((V, 3), F32)
    for r in range(int(rank.max()) + 1 if len(rank) else 0):
        slots = order[rank == r]
        vert = slot_vertex[slots]
        vn[vert] = vn[vert] + (fn[slots // 3] - vn[vert]) * (F32(1) / (F32(r) + F32(1)))
    a = np.stack([faces[:, 0], faces[:, 0], faces[:, 2]], 1).reshape(-1)
    b = np.stack([faces[:, 1], faces[:, 2], faces[:, 1]], 1).reshape(-1)
    d = _unit(xyz[b] - xyz[a])
    w = F32(1) - _dot(vn[a], vn[b])
    w = np.where(_dot(vn[b], d) > 0, w * w, w)
    by_weight = np.argsort(w, kind="stable")
    return gp.mesh_merge(a[by_weight], b[by_weight], w[by_weight], V, k_thresh, seg_min_verts)[0]


class StageClock(object):
    """``segment_mesh(..., _mark=clock)``: the device drained and the host clock read behind every stage"""

    def __init__(self):
        self.ms = {}
        torch.cuda.synchronize()
        self.t = time.perf_counter()

    def __call__(self, stage):
        torch.cuda.synchronize()
        now = time.perf_counter()
        self.ms[stage] = (now - self.t) * 1e3
        self.t = now


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--grid", type=int, default=390, help="vertices per side of the room")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_segment_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_segment_bench needs the MI355X")
    xyz, faces = room_mesh(args.grid)
    xyz_d, faces_d = torch.from_numpy(xyz).cuda(), torch.from_numpy(faces).cuda()
    k_thresh, seg_min_verts = gp.MESH_K_THRESH, gp.MESH_SEG_MIN_VERTS
    staged, whole, ids = [], [], None
    for i in range(args.warmup + args.iters):
        clock = StageClock()
        ids = gp.segment_mesh(xyz_d, faces_d, k_thresh, seg_min_verts, _mark=clock)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        gp.segment_mesh(xyz_d, faces_d, k_thresh, seg_min_verts)
        torch.cuda.synchronize()
        if i >= args.warmup:
            staged.append(clock.ms)
            whole.append((time.perf_counter() - t0) * 1e3)
    host_ms = []
    for _ in range(3):
        t0 = time.perf_counter()
        ids_host = host_definition(xyz, faces, k_thresh, seg_min_verts)
        host_ms.append((time.perf_counter() - t0) * 1e3)
    ids = ids.cpu().numpy()
    if not np.array_equal(ids, ids_host):
        raise SystemExit(f"the device's ids differ from the host definition's at {int((ids != ids_host).sum())} vertices")
    sizes = np.bincount(ids)
    res = {"device": torch.cuda.get_device_name(0), "iters": args.iters,
           "mesh": {"vertices": int(len(xyz)), "faces": int(len(faces)), "edges": int(3 * len(faces))},
           "kThresh": k_thresh, "segMinVerts": seg_min_verts, "segments": int(len(sizes)),
           "largest_segment": int(sizes.max()), "median_segment": float(np.median(sizes)),
           "stage_ms_drained": {s: round(statistics.median(run[s] for run in staged), 3) for s in STAGES},
           "read_back_bytes": int(12 * 3 * len(faces) + 8), "segment_mesh_ms": round(statistics.median(whole), 3),
           "host_definition_ms": round(statistics.median(host_ms), 1), "ids_equal_host_definition": True}
    text = json.dumps(res, indent=1)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
