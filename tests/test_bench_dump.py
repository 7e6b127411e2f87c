"""CPU: bench.py --dump-outputs -- what the last timed step returned, as <name>.npy in float32 / float64, within the
64 MB budget; an array too large for its share keeps the same seeded sample of rows in every run."""
import importlib.util
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("wsis_bench", os.path.join(ROOT, "bench.py"))
bench = importlib.util.module_from_spec(spec)
spec.loader.exec_module(bench)


def _ret(rows):
    g = torch.Generator().manual_seed(0)
    return {"semantic_scores": torch.randn(rows, 20, generator=g),
            "pred_sp_occupancy": torch.randn(50, generator=g, dtype=torch.float64),
            "edge_affinity": torch.randn(300, generator=g).half()}


def test_dump_small_outputs_whole(tmp_path):
    ret = _ret(1000)
    bench.dump_outputs(str(tmp_path), torch.tensor(1.5), ret)
    assert sorted(os.listdir(tmp_path)) == ["edge_affinity.npy", "loss.npy", "pred_sp_occupancy.npy",
                                            "semantic_scores.npy"]
    assert np.load(tmp_path / "loss.npy").dtype == np.float32 and float(np.load(tmp_path / "loss.npy")) == 1.5
    occ = np.load(tmp_path / "pred_sp_occupancy.npy")
    assert occ.dtype == np.float64 and np.array_equal(occ, ret["pred_sp_occupancy"].numpy())
    aff = np.load(tmp_path / "edge_affinity.npy")
    assert aff.dtype == np.float32 and np.array_equal(aff, ret["edge_affinity"].float().numpy())
    assert np.array_equal(np.load(tmp_path / "semantic_scores.npy"), ret["semantic_scores"].numpy())


def test_dump_large_output_sampled_within_budget(tmp_path):
    rows = bench.DUMP_BYTES // 80 + 1000            # [rows, 20] float32: just over the whole budget on its own
    ret = _ret(rows)
    ret["semantic_scores"][:, 0] = torch.arange(rows, dtype=torch.float32)      # exact row ids (rows < 2^24)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), torch.tensor(0.0), ret)
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 64 * 2 ** 20
    a, b = np.load(tmp_path / "a" / "semantic_scores.npy"), np.load(tmp_path / "b" / "semantic_scores.npy")
    assert a.shape[1] == 20 and rows // 2 < a.shape[0] < rows
    assert np.array_equal(a, b)                      # same shapes -> same rows
    ids = a[:, 0].astype(np.int64)
    assert np.all(np.diff(ids) > 0)                  # distinct rows, in their original order
    assert np.array_equal(ret["semantic_scores"].numpy()[ids], a)
