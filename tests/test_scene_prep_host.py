"""CPU: the device scene preparation (wsis_datasets.DeviceScenePrep, csrc/sceneprep.hip) is declared, exported and bound,
and refuses to run without the GPU.  The id tables (superpoint renumbering, instance re-compaction) are device code:
tests/test_gpu_scene_prep.py checks them against ``ScenePrep.get_cropped_inst_label`` and ``np.unique``."""
import ctypes
import os
import re

import numpy as np
import pytest

import wsis_native
from wsis_datasets import DeviceScenePrep, ScenePrep, collate_prepared, _ordered_to_double

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("wsis_sp_state_bytes", "wsis_sp_state_init", "wsis_sp_affine", "wsis_sp_crop_mask",
           "wsis_sp_emit_workspace_bytes", "wsis_sp_emit", "wsis_sp_tables", "wsis_sp_relabel", "wsis_sp_instance_info")


def test_entries_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "wsis_hip.h")).read()
    lib = ctypes.CDLL(os.path.join(ROOT, "3d-wsis_amd", "libwsis_hip.so"))
    _, bound = wsis_native.declared_symbols()
    for name in ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert hasattr(lib, name), name
        assert name in bound, name
    assert set(n for n in bound if n.startswith("wsis_sp_") and not n.startswith("wsis_sp_ce_")
               and not n.startswith("wsis_sp_regression_")) == set(ENTRIES)


def test_state_block_constants_agree_with_the_header():
    import wsis_datasets
    header = open(os.path.join(ROOT, "include", "wsis_hip.h")).read()
    rounds = int(re.search(r"#define WSIS_SP_ROUNDS (\d+)", header).group(1))
    assert re.search(r"#define WSIS_SP_STATE_WORDS \(16 \+ 4 \* WSIS_SP_ROUNDS\)", header)
    assert int(re.search(r"#define WSIS_SP_MAX_IDS (\d+)", header).group(1)) == wsis_datasets.SP_MAX_IDS
    assert (wsis_datasets._SP_ROUNDS, wsis_datasets._SP_ROUND0) == (rounds, 16)
    assert wsis_datasets._SP_STATE_WORDS == 16 + 4 * rounds
    lib = ctypes.CDLL(os.path.join(ROOT, "3d-wsis_amd", "libwsis_hip.so"))
    lib.wsis_sp_state_bytes.restype = ctypes.c_int64
    assert lib.wsis_sp_state_bytes() == 8 * wsis_datasets._SP_STATE_WORDS        # (no device needed: a constant)


def test_no_cpu_fallback():
    with pytest.raises(wsis_native.WsisError):
        DeviceScenePrep(device="cpu")
    with pytest.raises(wsis_native.WsisError):
        DeviceScenePrep(max_npoint=3000, seed=1, device="cpu")

    class Item(object):
        device = "cpu"
    with pytest.raises(wsis_native.WsisError):
        collate_prepared([Item()])
    assert issubclass(DeviceScenePrep, ScenePrep)


def test_ordered_keys_decode_to_the_doubles():
    """the state block keeps minima and maxima as ordered uint64 keys (include/wsis_hip.h): ~bits for a negative
    double, bits | 2^63 otherwise"""
    x = np.array([-1e300, -3.5, -1e-300, -0.0, 0.0, 1e-300, 7.25, 1e300])
    u = x.view(np.uint64)
    top = np.uint64(1) << np.uint64(63)
    keys = np.where(u & top, ~u, u | top)
    assert (np.diff(keys.astype(object)) > 0).all()                 # the keys order as the doubles do
    np.testing.assert_array_equal(_ordered_to_double(keys).view(np.uint64), u)
    np.testing.assert_array_equal(_ordered_to_double(keys.view(np.int64)).view(np.uint64), u)
