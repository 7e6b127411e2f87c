"""CPU: the C ABI and the host side of dynamic loss scaling (wsis_grad_nonfinite, wsis_adamw_step_scaled,
wsis_loss_scale_update; wsis_optim.LossScaler, FlatAdamW as a torch fused-protocol optimizer, harness.train_step(scaler=)).
Everything here returns before a kernel would be launched."""
import ctypes
import inspect
import os

import pytest
import torch

import wsis_native as _n

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("wsis_grad_nonfinite", "wsis_adamw_step_scaled", "wsis_loss_scale_update")
WSIS_ERR_ARG = -1


def test_err_arg_code_matches_header():
    import re
    text = open(os.path.join(ROOT, "include", "wsis_hip.h")).read()
    assert int(re.search(r"#define WSIS_ERR_ARG \((-?\d+)\)", text).group(1)) == WSIS_ERR_ARG


def test_symbols_exported_and_bound():
    raw = ctypes.CDLL(os.path.join(ROOT, "3d-wsis_amd", "libwsis_hip.so"))
    _, hip_names = _n.declared_symbols()
    lib = _n.hip()
    for name in NAMES:
        assert hasattr(raw, name), name
        assert name in hip_names, name
        assert getattr(lib, name).argtypes is not None and getattr(lib, name).restype is _n.I32, name
    assert len(lib.wsis_adamw_step_scaled.argtypes) == len(lib.wsis_adamw_step.argtypes) + 3


def _scaled(segments, blocks, n_blocks, skipped):
    return _n.hip().wsis_adamw_step_scaled(segments, blocks, n_blocks, 1e-3, 0.9, 0.999, 1e-8, 1e-4, None, None, skipped,
                                           None)


def test_step_scaled_argument_checks():
    seg = (ctypes.c_int64 * 7)()
    blk = (ctypes.c_int32 * 2)()
    skp = (ctypes.c_int32 * 1)()
    a, b, c = (ctypes.addressof(x) for x in (seg, blk, skp))
    assert _scaled(None, None, 0, None) == 0                 # nothing to do: nothing is touched, not even the pointers
    assert _scaled(a, b, 0, c) == 0
    assert _scaled(None, b, 1, c) == WSIS_ERR_ARG
    assert _scaled(a, None, 1, c) == WSIS_ERR_ARG
    assert _scaled(a, b, 1, None) == WSIS_ERR_ARG
    assert b"wsis_adamw_step_scaled" in _n.hip().wsis_last_error()
    assert _scaled(a, b, -1, c) == WSIS_ERR_ARG
    assert _scaled(a, b, 1 << 31, c) == WSIS_ERR_ARG


def test_check_and_update_argument_checks():
    lib = _n.hip()
    seg = (ctypes.c_int64 * 7)()
    blk = (ctypes.c_int32 * 2)()
    flag = (ctypes.c_float * 1)()
    a, b, f = (ctypes.addressof(x) for x in (seg, blk, flag))
    assert lib.wsis_grad_nonfinite(None, None, 0, None, None) == 0
    assert lib.wsis_grad_nonfinite(None, b, 1, f, None) == WSIS_ERR_ARG
    assert lib.wsis_grad_nonfinite(a, b, 1, None, None) == WSIS_ERR_ARG
    assert lib.wsis_grad_nonfinite(a, b, -1, f, None) == WSIS_ERR_ARG
    assert lib.wsis_loss_scale_update(None, f, f, 2.0, 0.5, 2000, None) == WSIS_ERR_ARG
    assert lib.wsis_loss_scale_update(f, None, f, 2.0, 0.5, 2000, None) == WSIS_ERR_ARG
    assert lib.wsis_loss_scale_update(f, f, None, 2.0, 0.5, 2000, None) == WSIS_ERR_ARG
    assert lib.wsis_loss_scale_update(f, f, f, 2.0, 0.5, 0, None) == WSIS_ERR_ARG


def test_loss_scaler_and_flat_adamw_refuse_cpu():
    import wsis_optim
    with pytest.raises(_n.WsisError):
        wsis_optim.LossScaler(device="cpu")
    with pytest.raises(_n.WsisError):
        wsis_optim.LossScaler(enabled=False, device="cpu")
    if not torch.cuda.is_available():
        with pytest.raises(_n.WsisError):
            wsis_optim.LossScaler()
    with pytest.raises(_n.WsisError):
        wsis_optim.FlatAdamW([torch.zeros(3, requires_grad=True)])


def test_loss_scaler_signature_is_grad_scalers():
    import wsis_optim
    sig = inspect.signature(wsis_optim.LossScaler.__init__).parameters
    ref = inspect.signature(torch.amp.GradScaler.__init__).parameters
    for k in ("init_scale", "growth_factor", "backoff_factor", "growth_interval", "enabled"):
        assert sig[k].default == ref[k].default, k
    for method in ("scale", "step", "update", "get_scale", "state_dict", "load_state_dict"):
        assert callable(getattr(wsis_optim.LossScaler, method))


def test_flat_adamw_declares_torchs_fused_protocol():
    import wsis_optim
    assert wsis_optim.FlatAdamW._step_supports_amp_scaling is True
    assert "grad_scaler" not in inspect.signature(wsis_optim.FlatAdamW.step).parameters    # the attribute form of it


def test_train_step_accepts_a_scaler():
    import harness
    p = inspect.signature(harness.train_step).parameters
    assert "scaler" in p and p["scaler"].default is None
