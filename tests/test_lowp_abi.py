"""CPU: the 16-bit sparse-convolution entry points (include/wsis_hip.h, csrc/spconv_lp.hip) are exported and bound, their
domain predicate covers every UNet layer shape and not the 6-channel input convolution, the workspace queries are
positive and never shrink as the row count grows, and the launch plan (wsis_spconv_lp_plan) keeps its rules over the whole
domain."""
import ctypes
import itertools
import os

import pytest

import wsis_native
from lowp_exact import PLAN_KEYS, lp_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LP_SYMBOLS = ("wsis_spconv_lp_supported", "wsis_spconv_fwd_lp", "wsis_spconv_fwd_lp_workspace_bytes",
              "wsis_spconv_dw_lp", "wsis_spconv_dw_lp_workspace_bytes", "wsis_weight_cast_lp", "wsis_spconv_lp_plan")
PLANES = (32, 64, 96, 128, 160)


def _unet_shapes():
    """(K, Cin, Cout) of every sparse product of the 5-level UNet, forward and dIn"""
    shapes = set()
    for l, c in enumerate(PLANES):
        shapes |= {(27, c, c), (27, 2 * c, c), (1, 2 * c, c)} if l < len(PLANES) - 1 else {(27, c, c)}
        if l + 1 < len(PLANES):
            shapes |= {(8, c, PLANES[l + 1]), (8, PLANES[l + 1], c)}
    return shapes | {(K, co, ci) for K, ci, co in shapes}


def test_lp_symbols_exported_and_bound():
    lib = ctypes.CDLL(os.path.join(ROOT, "3d-wsis_amd", "libwsis_hip.so"))
    _, hip_names = wsis_native.declared_symbols()
    for name in LP_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in hip_names, name


def test_lp_domain_covers_the_unet_and_not_the_input_conv():
    lib = wsis_native.hip()
    for K, ci, co in sorted(_unet_shapes()):
        assert lib.wsis_spconv_lp_supported(K, ci, co) == 1, (K, ci, co)
    for K, ci, co in ((27, 6, 32), (27, 32, 6), (27, 48, 32), (27, 32, 16), (0, 32, 32)):
        assert lib.wsis_spconv_lp_supported(K, ci, co) == 0, (K, ci, co)


def test_lp_workspace_queries_positive_and_monotone():
    lib = wsis_native.hip()
    rows = (0, 1, 31, 32, 1000, 4096, 70_000, 150_000, 1_000_000)
    for K, ci, co in ((27, 32, 32), (27, 160, 160), (8, 64, 96), (1, 256, 128), (125, 64, 32)):
        for query in (lib.wsis_spconv_fwd_lp_workspace_bytes, lib.wsis_spconv_dw_lp_workspace_bytes):
            got = [query(M, K, ci, co) for M in rows]
            assert all(v > 0 for v in got), (query.__name__, K, ci, co, got)
            assert got == sorted(got), (query.__name__, K, ci, co, got)
        assert lib.wsis_spconv_dw_lp_workspace_bytes(-1, K, ci, co) < 0


DW_WS_CAP = 256 << 20           # the slabs of one weight-gradient product stay below this
DW_MAX_CHUNKS, DW_CHUNK_ROWS = 64, 2048


def _cdiv(a, b):
    return -(-a // b)


def _check_plan(M, K, Cin, Cout):
    lib = wsis_native.hip()
    p = lp_plan(M, K, Cin, Cout)
    what = (M, K, Cin, Cout, p)
    two = (Cout // 32) % 2 == 0 and _cdiv(M, 32) * (Cout // 64) >= 4096
    assert p["nt"] == (2 if two else 1), what
    assert p["ncg"] * p["nt"] * 32 == Cout, what
    assert p["fwd_blocks"] == _cdiv(_cdiv(M, 32), 4) * p["ncg"], what
    c, rpc = p["chunks"], p["rows_per_chunk"]
    assert c * rpc >= M and rpc % 32 == 0 and rpc > 0, what
    assert 1 <= c <= DW_MAX_CHUNKS and c <= max(1, _cdiv(M, DW_CHUNK_ROWS)), what
    slabs = K * Cin * Cout * 4
    ws = lib.wsis_spconv_dw_lp_workspace_bytes(M, K, Cin, Cout)
    if c == 1:
        assert ws == 256, what
    else:
        assert c * slabs <= DW_WS_CAP and ws == c * slabs + 256, what
    # as many chunks as the three limits allow: the row count, the chunk cap and the workspace cap
    assert c == max(1, min(_cdiv(M, DW_CHUNK_ROWS), DW_MAX_CHUNKS, DW_WS_CAP // slabs)), what
    ntiles = (Cin // 32) * (Cout // 32)
    assert p["nw"] == min(4, ntiles), what
    per_group = p["nw"] * 4
    assert p["groups"] * per_group >= ntiles > (p["groups"] - 1) * per_group, what
    assert p["lds"] == (Cin + Cout) * 80 <= 160 * 1024, what
    return p


ROWS = (1, 31, 32, 33, 2048, 2049, 16352, 16353, 65504, 65505, 131040, 131041, 129025, 200_000, 1_000_000,
        (1 << 31) - 33)


@pytest.mark.parametrize("K", (1, 8, 27, 125))
def test_lp_plan_rules_over_the_domain(K):
    chans = range(32, 513, 32)
    for Cin, Cout in itertools.product(chans, chans):
        for M in ROWS:
            _check_plan(M, K, Cin, Cout)


def test_lp_plan_thresholds_and_named_cases():
    # NT = 2 from ceil(M / 32) * Cout / 64 >= 4096 on: the pairs on both sides at Cout 64, 128 and 512
    for M, Cout in ((131040, 64), (65504, 128), (16352, 512)):
        assert _check_plan(M, 27, 64, Cout)["nt"] == 1, (M, Cout)
        assert _check_plan(M + 1, 27, 64, Cout)["nt"] == 2, (M + 1, Cout)
    assert _check_plan(10 ** 6, 27, 64, 96)["nt"] == 1            # an odd number of 32-column tiles: never two
    # weight-gradient chunks: 1 / 2 around one chunk of rows, 64 with a one-row last chunk, the cap, the workspace cap
    assert _check_plan(2048, 8, 32, 32)["chunks"] == 1
    assert _check_plan(2049, 8, 64, 32)["chunks"] == 2
    p = _check_plan(129025, 2, 96, 32)
    assert (p["chunks"], p["rows_per_chunk"], 129025 - 63 * p["rows_per_chunk"]) == (64, 2048, 1), p
    assert _check_plan(200_000, 1, 160, 96)["chunks"] == 64
    assert _check_plan(20_000, 27, 512, 512)["chunks"] == 9
    assert _check_plan(5000, 125, 512, 512)["chunks"] == 2
    # waves and tile groups: 1-3 waves below 4 tiles, 2 groups (the last partial) at 20 tiles, 16 at 256
    assert [_check_plan(100, 1, ci, co)["nw"] for ci, co in ((32, 32), (64, 32), (96, 32), (32, 128))] == [1, 2, 3, 4]
    assert _check_plan(100, 1, 160, 96)["groups"] == 1              # 15 tiles
    assert _check_plan(100, 1, 160, 128)["groups"] == 2             # 20 tiles
    assert _check_plan(100, 1, 512, 512)["groups"] == 16            # 256 tiles
    # the LDS stage above 64 KiB
    assert _check_plan(100, 1, 512, 512)["lds"] == 80 * 1024
    assert _check_plan(100, 1, 512, 320)["lds"] > 64 * 1024


def test_lp_plan_refuses_outside_the_domain():
    lib = wsis_native.hip()
    out = (ctypes.c_int32 * len(PLAN_KEYS))()
    for M, K, ci, co in ((0, 27, 32, 32), (-1, 27, 32, 32), (1 << 31, 27, 32, 32), (100, 27, 6, 32),
                         (100, 27, 32, 544), (100, 0, 32, 32)):
        assert lib.wsis_spconv_lp_plan(M, K, ci, co, out) != 0, (M, K, ci, co)
    assert lib.wsis_spconv_lp_plan(100, 27, 32, 32, None) != 0
