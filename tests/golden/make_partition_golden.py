"""Generates tests/golden/partition_golden.npz by running the REFERENCE's own ``compute_graph_nn_2`` and the
expressions of ``generate_SPG_superpoint`` on two seeded synthetic pruned rooms:

    data/S3DIS/partition/graphs.py              compute_graph_nn_2       :26-83   (sklearn NearestNeighbors, kd_tree)
    data/S3DIS/partition/partition_S3DIS.py     generate_SPG_superpoint  :105-108 (distances -> edge_weight)

``graphs.py`` cannot be imported as a whole (its other functions need libraries that are absent), so the function's
source is read from the reference checkout AT GENERATION TIME, compiled and executed with the names it uses (numpy,
``numpy.matlib``, sklearn's ``NearestNeighbors``); nothing of it is stored here.  The edge-weight expression of :108 is
evaluated on what that function returned, with numpy's own ``np.mean``.  ``libply_c`` (prune, compute_geof) needs
boost-python and Eigen and cannot be built here: the rooms are pruned by tests/partition_ref.py, and there is no
fixture of the reference's fp32 geometric features.

A room: floor, one wall, a thin column and a cluttered volume, offset some metres from the origin, pruned at 3 cm to
about 2,600 voxels (3,000 would take the archive past 1 MiB).  The seeds are tried in order, a room starting after
the seed the room before it kept; a room keeps the first seed for which no row has two equal d2 among its first 46
candidates and no two points coincide, so that the neighbour order sklearn leaves open is not exercised, and asserts
that the reference's lists are then the (d2, id) order and its distances float32(sqrt(d2)).

The archive is written with fixed member timestamps: the same inputs give the same bytes.

    python tests/golden/make_partition_golden.py
"""
import ast
import io
import os
import sys
import zipfile

import numpy as np
import numpy.matlib  # noqa: F401  (compute_graph_nn_2 calls np.matlib.repmat)
from sklearn.neighbors import NearestNeighbors

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import partition_ref as ref        # noqa: E402

REF_GRAPHS = "/root/reference/data/S3DIS/partition/graphs.py"
VOXEL, K_ADJ, K_GEOF, LAMBDA = 0.03, 10, 45, 1.
N_POINTS, SIZE = 3150, (1.5, 1.2, 1.0)
ROOMS = (("room_a", (12.0, -7.0, 3.0)), ("room_b", (-4.5, 21.0, 0.5)))


def reference_function(path, name):
    tree = ast.parse(open(path).read())
    body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == name]
    assert len(body) == 1
    ns = {"np": np, "NearestNeighbors": NearestNeighbors}
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)
    return ns[name]


def clear_of_ties(xyz):
    """no two points coincide and no row has two equal d2 among its first 46 candidates"""
    if len(np.unique(xyz, axis=0)) != len(xyz):
        return False
    _, d2 = ref.knn(xyz, K_GEOF + 1)
    return bool((np.diff(d2, axis=1) > 0).all() and (d2[:, 0] > 0).all())


def run(compute_graph_nn_2, seed, offset):
    raw_xyz, raw_rgb = ref.make_room(seed, n=N_POINTS, offset=offset, size=SIZE)
    pr = ref.prune(raw_xyz, VOXEL, raw_rgb)
    xyz, rgb = pr["xyz"], pr["rgb"]
    if not clear_of_ties(xyz):
        return None
    graph_nn, target2 = compute_graph_nn_2(xyz, K_ADJ, K_GEOF)
    # partition_S3DIS.py:108
    edge_weight = np.array(1. / (LAMBDA + graph_nn["distances"] / np.mean(graph_nn["distances"])), dtype='float32')
    mean = np.mean(graph_nn["distances"])
    assert graph_nn["source"].dtype == graph_nn["target"].dtype == target2.dtype == np.uint32
    assert graph_nn["distances"].dtype == edge_weight.dtype == mean.dtype == np.float32
    nbr, d2 = ref.knn(xyz, K_GEOF)
    assert np.array_equal(target2, nbr.flatten().astype(np.uint32)), "the reference's lists are the (d2, id) order"
    assert np.array_equal(graph_nn["distances"], np.sqrt(d2[:, :K_ADJ]).flatten().astype(np.float32))
    return {"seed": np.int64(seed), "xyz": xyz, "rgb": rgb, "source": graph_nn["source"], "target": graph_nn["target"],
            "distances": graph_nn["distances"], "target2": target2, "edge_weight": edge_weight, "mean": np.float32(mean)}


def save(path, arrays):
    """an .npz whose bytes depend on the arrays alone"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


def main():
    fn = reference_function(REF_GRAPHS, "compute_graph_nn_2")
    out, seed = {}, 0
    for tag, offset in ROOMS:
        res = None
        while res is None:
            res = run(fn, seed, offset)
            seed += 1
            assert seed < 200, "no seed clear of ties"
        out.update({f"{tag}_{k}": v for k, v in res.items()})
        d2 = ref.knn(res["xyz"], K_GEOF + 1)[1]
        gap = float((np.diff(d2, axis=1) / d2[:, 1:]).min())
        print(f"{tag}: seed {int(res['seed'])} V {len(res['xyz'])} E {len(res['source'])}  smallest relative gap between "
              f"consecutive d2 {gap:.3g}  reference mean {float(res['mean']):.9g}")
    path = os.path.join(HERE, "partition_golden.npz")
    save(path, out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
