"""GPU: one weight gradient per kind of the launch plan (csrc/spconv_dw2.hip: dw_plan), each at the smallest shape that
reaches it: register gather and LDS ring (33 rows, 27 offsets, 32 -> 32; WSIS_DW3 = 1 / 0), the dense product without a
table (129 rows, 32 -> 4), the 6 -> 32 input convolution, the generic kernel (33 -> 200 channels), the own-rows form
(33 -> 65 rows, 32 -> 64) and an empty level.  The plan query says which kind the launch takes, and the test asserts it.

Each dW, computed into a workspace and an output full of NaN, equals an fp64 gather-GEMM within the bound of
tests/test_gpu_dw_hint.py (2e-6 of the largest element), repeats bit for bit, and -- where an X that is only 8-byte
aligned keeps the product on the same kind -- is bit-identical for such an X; where it moves the product to the generic
kernel the result is held to fp64 as well."""
import numpy as np
import pytest
import torch

import dw_plan_ref as plan
import wsis_native as _n

pytestmark = pytest.mark.gpu
DEV = "cuda"
BOUND = 2e-6

# name -> (M_in, M_out, K, Cin, Cout, table, WSIS_DW3, kind)
SHAPES = {
    "dw3": (33, 33, 27, 32, 32, True, "1", plan.DW3),
    "ring": (33, 33, 27, 32, 32, True, "0", plan.RING),
    "dense": (129, 129, 1, 32, 4, False, "1", plan.DW3),
    "in_conv": (33, 33, 27, 6, 32, True, "1", plan.IN_CONV),
    "generic": (33, 33, 27, 33, 200, True, "1", plan.GENERIC),
}


def _table(rng, rows, other_rows, K):
    """[K, rows] int32: offset 0 pairs every row, the others a random 60 % (a row of the other tensor, or -1)"""
    t = rng.integers(0, other_rows, (K, rows)).astype(np.int32)
    t[1:][rng.random((K - 1, rows)) >= 0.6] = -1
    return t


def _offset_by_8(t):
    """the same values in storage that is 8-byte but not 16-byte aligned"""
    store = torch.empty(t.numel() + 2, dtype=t.dtype, device=t.device)
    v = store[2:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 8
    return v


def _kind(X, dY, dW, ws, M_in, M_out, K, Cin, Cout, table, swapped=0):
    align = ((X.data_ptr() % 16 == 0) * plan.X16 | (X.data_ptr() % 8 == 0) * plan.X8 | (dY.data_ptr() % 16 == 0) * plan.DY16
             | (dW.data_ptr() % 16 == 0) * plan.DW16 | (ws.data_ptr() % 16 == 0) * plan.WS16)
    case = plan.Case("gpu", M_in, M_out, K, Cin, Cout, plan.TABLE if table else plan.NO_TABLE, int(align), swapped, 1, "")
    return plan.plan_lib(case)["kind"]


def _held_to_fp64(got, want, what):
    scale = float(want.abs().max())
    err = float((got.double() - want).abs().max())
    print(f"{what}: max err {err:.3e} of scale {scale:.3e} ({err / scale:.2e} <= {BOUND:.0e})")
    assert torch.isfinite(got).all() and err / scale < BOUND, what


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_one_weight_gradient_per_kind(monkeypatch, name):
    M_in, M_out, K, Cin, Cout, table, dw3, kind = SHAPES[name]
    monkeypatch.setenv("WSIS_DW3", dw3)
    lib = _n.hip()
    rng = np.random.default_rng(K * 100 + Cin)
    g = torch.Generator(device=DEV).manual_seed(Cin + Cout)
    X = torch.randn(M_in, Cin, device=DEV, generator=g)
    dY = torch.randn(M_out, Cout, device=DEV, generator=g)
    if table:
        nbr = torch.from_numpy(_table(rng, M_out, M_in, K)).to(DEV)
        order = torch.from_numpy(rng.permutation(M_out).astype(np.int32)).to(DEV)
        nbr_p = nbr[:, order.long()].contiguous()
    else:
        nbr, order, nbr_p = torch.arange(M_out, device=DEV, dtype=torch.int32)[None], None, None
    want = torch.stack([X[nbr[k][nbr[k] >= 0].long()].double().t() @ dY[nbr[k] >= 0].double() for k in range(K)])
    wsb = lib.wsis_spconv_dw_workspace_bytes(M_out, K, Cin, Cout)

    def run(x):
        ws = torch.full((wsb,), 255, dtype=torch.uint8, device=DEV)           # every float of it a NaN
        dW = torch.full((K, Cin, Cout), float("nan"), device=DEV)
        took = _kind(x, dY, dW, ws, M_in, M_out, K, Cin, Cout, table)
        _n.check(lib.wsis_spconv_dw(_n.ptr(x), _n.ptr(nbr_p), _n.ptr(order), _n.ptr(dY), _n.ptr(dW), M_in, M_out, K, Cin,
                                    Cout, _n.ptr(ws), wsb, _n.stream_ptr()), "spconv_dw")
        torch.cuda.synchronize()
        return dW, took

    got, took = run(X)
    assert took == kind, (plan.KIND_NAMES[took], plan.KIND_NAMES[kind])
    _held_to_fp64(got, want, name)
    again, _ = run(X)
    assert torch.equal(got, again), "repeat"
    got8, took8 = run(_offset_by_8(X))
    if took8 == kind:
        assert torch.equal(got, got8), "X at an 8-byte offset, same kind"
    else:
        assert took8 == plan.GENERIC
        _held_to_fp64(got8, want, name + " with X at an 8-byte offset (generic)")
    print(f"{name}: kind {plan.KIND_NAMES[took]}, X at an 8-byte offset: {plan.KIND_NAMES[took8]}")


def test_own_rows_form():
    """wsis_spconv_dw_bn without statistics: slices over the 33 input rows, dY gathered through the dIn table"""
    M_in, M_out, K, Cin, Cout = 33, 65, 8, 32, 64
    lib = _n.hip()
    rng = np.random.default_rng(5)
    g = torch.Generator(device=DEV).manual_seed(9)
    X = torch.randn(M_in, Cin, device=DEV, generator=g)
    dY = torch.randn(M_out, Cout, device=DEV, generator=g)
    nbr_b = torch.from_numpy(_table(rng, M_in, M_out, K)).to(DEV)             # [K, M_in]: the output row of input row i
    order_b = torch.from_numpy(rng.permutation(M_in).astype(np.int32)).to(DEV)
    nbr_bp = nbr_b[:, order_b.long()].contiguous()
    want = torch.stack([X[nbr_b[k] >= 0].double().t() @ dY[nbr_b[k][nbr_b[k] >= 0].long()].double() for k in range(K)])
    assert lib.wsis_spconv_dw_bn_supported(K, Cin, Cout)
    wsb = lib.wsis_spconv_dw_bn_workspace_bytes(M_in, K, Cin, Cout)

    def run():
        ws = torch.full((wsb,), 255, dtype=torch.uint8, device=DEV)
        dW = torch.full((K, Cin, Cout), float("nan"), device=DEV)
        assert _kind(X, dY, dW, ws, M_in, M_out, K, Cin, Cout, True, swapped=1) == plan.SWAPPED
        _n.check(lib.wsis_spconv_dw_bn(_n.ptr(X), None, None, None, None, 1e-4, 0, _n.ptr(nbr_bp), _n.ptr(order_b), 0,
                                       _n.ptr(dY), _n.ptr(dW), M_in, M_out, K, Cin, Cout, _n.ptr(ws), wsb,
                                       _n.stream_ptr()), "dw_bn")
        torch.cuda.synchronize()
        return dW

    got = run()
    _held_to_fp64(got, want, "own rows")
    assert torch.equal(got, run()), "repeat"
    # (the own-rows form has no kernel for an X that is not 16-byte aligned: the entry point refuses it)
    x8, ws = _offset_by_8(X), torch.empty(wsb, dtype=torch.uint8, device=DEV)
    dW = torch.empty(K, Cin, Cout, device=DEV)
    assert lib.wsis_spconv_dw_bn(_n.ptr(x8), None, None, None, None, 1e-4, 0, _n.ptr(nbr_bp), _n.ptr(order_b), 0,
                                 _n.ptr(dY), _n.ptr(dW), M_in, M_out, K, Cin, Cout, _n.ptr(ws), wsb, _n.stream_ptr()) != 0
    assert b"alignment" in lib.wsis_last_error()


def test_empty_level():
    """no output rows: both forms zero-fill dW and touch nothing else"""
    lib = _n.hip()
    K, Cin, Cout = 27, 32, 64
    dY = torch.empty(0, Cout, device=DEV)
    X = torch.randn(40, Cin, device=DEV)
    for swapped in (0, 1):
        for _ in range(2):
            dW = torch.full((K, Cin, Cout), float("nan"), device=DEV)
            assert _kind(X, dY, dW, dW, 40, 0, K, Cin, Cout, True, swapped) == plan.EMPTY
            if swapped:
                rc = lib.wsis_spconv_dw_bn(_n.ptr(X), None, None, None, None, 1e-4, 0, None, None, 1, None, _n.ptr(dW), 40,
                                           0, K, Cin, Cout, None, 0, _n.stream_ptr())
            else:
                rc = lib.wsis_spconv_dw(_n.ptr(X), None, None, None, _n.ptr(dW), 40, 0, K, Cin, Cout, None, 0,
                                        _n.stream_ptr())
            _n.check(rc, "empty level")
            torch.cuda.synchronize()
            assert torch.equal(dW, torch.zeros_like(dW))
