"""The launch plan of the fp32 weight gradient (csrc/spconv_dw2.hip: dw_plan, what wsis_spconv_dw / wsis_spconv_dw_bn /
the size queries / wsis_debug_dw2_diag all call) restated in plain Python with the default build's constants, and the
shape table that reaches every branch of it.  Nothing here calls the library except ``plan_lib`` (the library's own
host-only plan query wsis_debug_dw_plan); tests/test_dw_plan_host.py holds the two to each other and to the figures
tests/golden/dw_plan_golden.json recorded before the plan had one definition.

The rule:
  empty      M_out == 0 (own-rows form: M_in == 0 or M_out == 0): dW is zero-filled
  dw2 family K <= 32, Cin % 32 == 0, Cout % 4 == 0; X, dY and the table below 2 GiB; table AND order, or no table with
             K == 1 and M_in == M_out; X, dY, dW and the workspace 16-byte aligned.  Register gather (dw3) where WSIS_DW3
             != 0 and the row ids fit (dw3_fits), else the LDS ring (its XCD deal: an EXPERIMENTAL knob)
  input conv a table, 27 x 6 -> 32, X 8-byte aligned, dW and workspace 16-byte aligned
  generic    everything else
  own rows   (wsis_spconv_dw_bn) always the LDS ring with the roles of the two tensors exchanged
"""
import collections
import ctypes
import os

import numpy as np

EMPTY, DW3, RING, RING_XCD, SWAPPED, IN_CONV, GENERIC = range(7)
KIND_NAMES = ("empty", "dw3", "ring", "ring_xcd", "swapped", "in_conv", "generic")
NO_TABLE, TABLE, TABLE_NO_ORDER = 0, 1, 2
# alignment bits of the plan query: X 16 bytes, X 8 bytes, dY 16, dW 16, workspace 16
X16, X8, DY16, DW16, WS16 = 1, 2, 4, 8, 16
ALIGNED = 31
HINTS = (0, 249999, 250000, 625000)
WIDE_ROWS = 250000

GS, WGW = 8, 4
TILE = 32 * 128
HDR = (GS * 32 + 64) * 4
WAVE_LDS = 2 * HDR + TILE + 3 * TILE + 256      # two headers, dY tile, three X tiles, a row of -1
WAVE_LDS3 = 2 * HDR + TILE
P_CLAUSES = ("hint", "slices", "floor", "dense", "cap", "mult8")

Plan = collections.namedtuple("Plan", "kind P gx gy lds total4")


def p_plan(rows, K, cg, co, wide, hit=None):
    """dw2_P_plan: slabs (workgroups per combination) over ``rows`` sliced rows, ``cg`` gathered and ``co`` own channels;
    ``hit`` collects the clauses that changed the outcome"""
    hit = set() if hit is None else hit
    n_slices = (rows + 31) // 32
    by_slices = n_slices >= 8192
    if by_slices:
        hit.add("slices")
    elif wide:
        hit.add("hint")
    target = 2048 if (wide or by_slices) else 1024
    nog = (K + GS - 1) // GS
    combos = nog * (cg // 32) * ((co + 31) // 32)
    P = (target // WGW + combos - 1) // combos
    if K != 1 and P * combos > target // WGW and P > 1:
        P -= 1
        hit.add("floor")
    if K == 1:
        widened = min(n_slices // (4 * WGW), 32)
        if widened > P:
            P = widened
            hit.add("dense")
    cap = (n_slices + WGW - 1) // WGW
    if P > cap:
        P = cap
        hit.add("cap")
    if P >= 8:
        if P & 7:
            hit.add("mult8")
        P &= ~7
    return max(P, 1)


def dw2_supported(K, Cin, Cout):
    return 1 <= K <= 32 and Cin >= 32 and Cin % 32 == 0 and Cout >= 4 and Cout % 4 == 0


def dw2_fits(M_in, M_out, K, Cin, Cout):
    lim = 1 << 31
    return M_in * Cin * 4 < lim and M_out * Cout * 4 < lim and K * M_out * 4 < lim and M_in >= 1 and M_out >= 1


def dw3_fits(M_in, Cin):
    p = Cin * 4
    w = (0xFFFFFF * p) & 0xFFFFFFFF
    return M_in < (1 << 24) - 1 and w >= M_in * p and w <= 0xFFFFFF00


def bn_supported(K, Cin, Cout):
    return dw2_supported(K, Cout, Cin) and Cin % 32 == 0 and Cout % 32 == 0


def plan_ref(M_in, M_out, K, Cin, Cout, table, align, swapped, hint_rows=0, dw3=1, in_conv=1, xcd_rows=0, hit=None):
    """the Plan of a launch, or None where the entry point refuses the arguments"""
    wide = hint_rows >= WIDE_ROWS
    if M_in < 0 or M_out < 0 or K < 1 or Cin < 1 or Cout < 1:
        return None
    nog = (K + GS - 1) // GS
    total4 = K * Cin * Cout // 4
    if swapped:
        if not bn_supported(K, Cin, Cout):
            return None
        if M_in == 0 or M_out == 0:
            return Plan(EMPTY, 0, 0, 0, 0, 0)
        if table != TABLE or not dw2_fits(M_out, M_in, K, Cout, Cin) or align & (X16 | DY16 | DW16 | WS16) != X16 | DY16 | DW16 | WS16:
            return None
        P = p_plan(M_in, K, Cout, Cin, wide, hit)
        return Plan(SWAPPED, P, P, nog * (Cout // 32) * ((Cin + 31) // 32), WAVE_LDS * WGW, total4)
    if M_out == 0:
        return Plan(EMPTY, 0, 0, 0, 0, 0)
    if table == NO_TABLE and not (K == 1 and M_in == M_out):
        return None
    if K > 128 or M_in * Cin * 4 >= 1 << 32 or M_out * Cout * 4 >= 1 << 32:
        return None
    paired = table == TABLE or (table == NO_TABLE and K == 1 and M_in == M_out)
    all16 = align & (X16 | DY16 | DW16 | WS16) == X16 | DY16 | DW16 | WS16
    if dw2_supported(K, Cin, Cout) and dw2_fits(M_in, M_out, K, Cin, Cout) and paired and all16:
        P = p_plan(M_out, K, Cin, Cout, wide, hit)
        gy = nog * (Cin // 32) * ((Cout + 31) // 32)
        if dw3 and dw3_fits(M_in, Cin):
            return Plan(DW3, P, P, gy, WAVE_LDS3 * WGW, total4)
        xcd = xcd_rows > 0 and M_out >= xcd_rows and P % 8 == 0
        return Plan(RING_XCD if xcd else RING, P, P, gy, WAVE_LDS * WGW, total4)
    if table != NO_TABLE and in_conv and (K, Cin, Cout) == (27, 6, 32) and align & X8 and align & DW16 and align & WS16:
        return Plan(IN_CONV, 0, 0, 0, 0, 0)      # (grid and slabs: the launcher's own, csrc/spconv_in.hip)
    return Plan(GENERIC, 0, 0, 0, 0, 0)          # (csrc/spconv.hip)


# ---------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "name M_in M_out K Cin Cout table align swapped dw3 why")


def _cases():
    out = []

    def add(name, M_in, M_out, K, Cin, Cout, why, table=TABLE, align=ALIGNED, swapped=0, dw3=1):
        out.append(Case(name, M_in, M_out, K, Cin, Cout, table, align, swapped, dw3, why))

    # row counts x channel widths: one partial slice ... the 8,192-slice switch (262,112 | 262,113) ... four scenes
    rows = (1, 31, 32, 33, 127, 129, 4095, 26819, 153685, 262112, 262113, 625000)
    for K, Cin, Cout in ((27, 32, 32), (27, 64, 64), (27, 96, 96), (27, 64, 32), (8, 32, 64), (8, 64, 32)):
        for M in rows:
            # submanifold: M_in == M_out; strided 32 -> 64: four fine rows per coarse one; inverse 64 -> 32: the other way
            M_in = M if K == 27 else 4 * M if Cin < Cout else (M + 3) // 4
            add("k%d_%d_%d_m%d" % (K, Cin, Cout, M), M_in, M, K, Cin, Cout, "row count x width, cap / floor / slice switch")
    add("dense_2080_few", 1000, 1000, 1, 32, 2080, "dense, too few slices for the widening", table=NO_TABLE)
    add("dense_2080_wide", 20000, 20000, 1, 32, 2080, "dense widening to 32 workgroups", table=NO_TABLE)
    add("dense_2080_mid", 6000, 6000, 1, 32, 2080, "dense widening to 11, rounded to 8", table=NO_TABLE)
    add("dense_64_64", 153685, 153685, 1, 64, 64, "dense point-level Linear", table=NO_TABLE)
    add("dense_32_4", 129, 129, 1, 32, 4, "dense, partial output block", table=NO_TABLE)
    add("k1_table", 129, 129, 1, 32, 32, "K = 1 with an identity table")
    add("dense_ring", 129, 129, 1, 32, 4, "dense on the LDS ring", table=NO_TABLE, dw3=0)
    # outside the dw2 family
    add("in_conv_l0", 153685, 153685, 27, 6, 32, "input convolution")
    add("in_conv_33", 33, 33, 27, 6, 32, "input convolution, smallest")
    add("in_conv_x8", 33, 33, 27, 6, 32, "input convolution, X 8-byte aligned", align=X8 | DY16 | DW16 | WS16)
    add("in_conv_x4", 33, 33, 27, 6, 32, "6 -> 32 with an unaligned X: generic", align=DY16 | DW16 | WS16)
    add("in_conv_dw4", 33, 33, 27, 6, 32, "6 -> 32 with an unaligned dW: generic", align=X16 | X8 | DY16 | WS16)
    add("generic_33_200", 33, 33, 27, 33, 200, "Cin not a multiple of 32")
    add("generic_32_6", 33, 33, 27, 32, 6, "Cout not a multiple of 4")
    add("generic_k125", 4095, 4095, 125, 32, 32, "more than 32 offsets")
    add("refused_k129", 33, 33, 129, 32, 32, "more than 128 offsets: refused")
    add("no_order", 33, 33, 27, 32, 32, "a table without its order: generic", table=TABLE_NO_ORDER)
    add("no_table_k27", 33, 33, 27, 32, 32, "no table and K != 1: refused", table=NO_TABLE)
    add("no_table_rows_differ", 33, 65, 1, 32, 32, "no table and M_in != M_out: refused", table=NO_TABLE)
    # alignment of a dw2-family shape
    add("align_16", 33, 33, 27, 32, 32, "all four 16-byte aligned")
    add("align_x8", 33, 33, 27, 32, 32, "X 8-byte aligned only: generic", align=X8 | DY16 | DW16 | WS16)
    add("align_none", 33, 33, 27, 32, 32, "nothing aligned: generic", align=0)
    add("align_ws", 33, 33, 27, 32, 32, "workspace unaligned: generic", align=X16 | X8 | DY16 | DW16)
    # dw3_fits: the pitch edge (a missing pair must land beyond the tensor) and the 24-bit row-id edge
    add("dw3_pitch_in", 5592404, 5592404, 27, 96, 96, "96 channels, last M_in of the register gather")
    add("dw3_pitch_out", 5592405, 5592405, 27, 96, 96, "96 channels, first M_in of the LDS ring")
    add("dw3_rowid_in", (1 << 24) - 2, 1 << 22, 8, 32, 64, "row ids fit 24 bits")
    add("dw3_rowid_out", (1 << 24) - 1, 1 << 22, 8, 32, 64, "row id 2^24 - 1 is the missing pair's")
    # dw2_fits: X just below and at 2 GiB
    add("fits_in", (1 << 23) - 1, 1 << 21, 8, 64, 32, "X just below 2 GiB")
    add("fits_out", 1 << 23, 1 << 21, 8, 64, 32, "X of 2 GiB: generic")
    add("too_large", 1 << 24, 1 << 22, 8, 64, 32, "X of 4 GiB: refused")
    # WSIS_DW3=0: the LDS ring
    for M in (33, 26819, 262113):
        add("ring_k27_64_m%d" % M, M, M, 27, 64, 64, "WSIS_DW3=0", dw3=0)
    add("ring_k8_m4095", 4 * 4095, 4095, 8, 32, 64, "WSIS_DW3=0, strided", dw3=0)
    # empty levels
    add("empty", 0, 0, 27, 32, 32, "M_out == 0")
    add("empty_out", 40, 0, 8, 32, 64, "M_out == 0 below rows")
    # the own-rows form: slices over M_in, channel roles exchanged
    for M in (33, 4095, 26819, 262113, 625000):
        add("swapped_subm_m%d" % M, M, M, 27, 64, 64, "own rows, submanifold", swapped=1)
    add("swapped_96_32", 26819, 26819, 27, 96, 32, "own rows, 96 -> 32", swapped=1)
    add("swapped_down", 4 * 26819, 26819, 8, 32, 64, "own rows, strided", swapped=1)
    add("swapped_inverse", 26819, 4 * 26819, 8, 64, 32, "own rows, inverse", swapped=1)
    add("swapped_33_65", 33, 65, 8, 32, 64, "own rows, smallest", swapped=1)
    add("swapped_empty_in", 0, 65, 8, 32, 64, "own rows, no input rows", swapped=1)
    add("swapped_empty_out", 33, 0, 8, 32, 64, "own rows, no output rows", swapped=1)
    add("swapped_cout_36", 33, 33, 27, 32, 36, "own rows need Cout % 32 == 0: refused", swapped=1)
    add("swapped_unaligned", 33, 33, 27, 32, 32, "own rows need 16-byte alignment: refused", swapped=1, align=X8)
    add("swapped_too_large", 1 << 22, 1 << 24, 8, 64, 32, "own rows, gathered dY of 2 GiB: refused", swapped=1)
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


CASES = _cases()


def reference(case, hint_rows, hit=None):
    return plan_ref(case.M_in, case.M_out, case.K, case.Cin, case.Cout, case.table, case.align, bool(case.swapped),
                    hint_rows=hint_rows, dw3=case.dw3, hit=hit)


# ---------------------------------------------------------------------------------------------------------------------
_LIB = []


def lib():
    """libwsis_hip.so by path, as tests/fwd2_ref.py loads it (host arithmetic: no device needed)"""
    if not _LIB:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        so = ctypes.CDLL(os.path.join(root, "3d-wsis_amd", "libwsis_hip.so"))
        so.wsis_spconv_dw_workspace_bytes.restype = ctypes.c_int64
        so.wsis_spconv_dw_workspace_bytes.argtypes = [ctypes.c_int64] + [ctypes.c_int32] * 3
        so.wsis_spconv_dw_bn_workspace_bytes.restype = ctypes.c_int64
        so.wsis_spconv_dw_bn_workspace_bytes.argtypes = [ctypes.c_int64] + [ctypes.c_int32] * 3
        so.wsis_spconv_dw_bn_supported.restype = ctypes.c_int32
        so.wsis_spconv_dw_bn_supported.argtypes = [ctypes.c_int32] * 3
        so.wsis_hint_batch_rows.restype = ctypes.c_int32
        so.wsis_hint_batch_rows.argtypes = [ctypes.c_int64]
        _LIB.append(so)
    return _LIB[0]


PLAN_FIELDS = ("kind", "P", "gx", "gy", "lds", "total4", "flags", "ws_bytes")


def plan_lib(case):
    """{field: value} of wsis_debug_dw_plan under the present hint and environment, or None where it refuses"""
    fn = lib().wsis_debug_dw_plan
    fn.restype = ctypes.c_int32
    fn.argtypes = [ctypes.c_int64, ctypes.c_int64] + [ctypes.c_int32] * 6 + [ctypes.c_void_p]
    out = np.full(len(PLAN_FIELDS), -7, dtype=np.int64)
    rc = fn(case.M_in, case.M_out, case.K, case.Cin, case.Cout, case.table, case.align, case.swapped, out.ctypes.data)
    return dict(zip(PLAN_FIELDS, out.tolist())) if rc == 0 else None
