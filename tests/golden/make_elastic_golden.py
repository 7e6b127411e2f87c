"""Generates tests/golden/elastic_golden.npz by running the REFERENCE's own ``ScanNetV2Inst_spg.elastic``
(modules/datasets/scannetv2_dataset.py:222-249) behind the stand-ins of make_dataset_golden.py: the method's source is
read from the reference checkout at generation time and bound to a bare object (it ignores ``self``); nothing of it is
stored here.  ``scipy.ndimage.filters``, which the method names and newer scipy no longer has, is aliased to
``scipy.ndimage`` there.  The reference draws from numpy's global state, so each case runs after ``np.random.seed(s)``;
``RandomState(s).randn`` is the same stream, which is what ``ScenePrep(seed=s).elastic`` must reproduce.

Stored per case k: ``in_k`` fp64 [N,3] (negative and positive coordinates), ``cfg_k`` = (gran, mag, seed), ``bb_k``
int32 [3], ``out_k`` fp64 [N,3].  Arrays only.  Needs the reference checkout and scipy; never run on the GPU machine.

    python tests/golden/make_elastic_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_dataset_golden import reference_object  # noqa: E402

CASES = ((6, 40.0, 61), (20, 160.0, 62))              # (gran, mag) of the two calls at scale 50, and the seed


def main():
    ref = reference_object()
    out = {"n_cases": np.int64(len(CASES))}
    for k, (gran, mag, seed) in enumerate(CASES):
        rs = np.random.RandomState(100 + k)
        xyz = (rs.rand(3000, 3) - np.array([0.6, 0.3, 0.1])) * np.array([260.0, 190.0, 120.0])
        np.random.seed(seed)
        got = ref.elastic(xyz.copy(), gran, mag)
        out[f"in_{k}"] = xyz
        out[f"cfg_{k}"] = np.asarray([gran, mag, seed], dtype=np.float64)
        out[f"bb_{k}"] = (np.abs(xyz).max(0).astype(np.int32) // gran + 3).astype(np.int32)
        out[f"out_{k}"] = got
        print(k, "gran", gran, "mag", mag, "bb", out[f"bb_{k}"], "largest displacement", float(np.abs(got - xyz).max()))
    path = os.path.join(HERE, "elastic_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
