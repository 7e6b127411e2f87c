"""CPU: the workspace layout of a pass of the op-list executor (csrc/executor.hip: plan_pass) without a GPU.  The op byte
arrays of tests/golden/unet_program_golden.npz are complete forward and backward programs; the size query and the
diagnostic export of the plan run on them without a device.

* the sizes are those tests/golden/executor_layout_golden.json recorded at the revision before the layout got one
  definition (tests/golden/make_executor_layout_golden.py), per build flavour and under every switch that changes them;
* the plan itself: aligned, ordered, disjoint regions that add up to the size query's answer; a weight slot for exactly
  the ops that read one, each large enough, in op order; refused lists refused by both entry points."""
import ctypes

import numpy as np
import pytest

import unet_native as un
import wsis_native
from tests.golden import make_executor_layout_golden as gen
from tests.golden import make_unet_program_golden as prog

# (the 15 programs whose sizes executor_layout_golden.json recorded at its revision: the 16-bit training programs were
# added to unet_program_golden.npz later)
CASES = sorted(n for n, spec in prog.CASES.items() if spec[0] != "lp_train")
ALIGN = 256
N_REGIONS = 5      # 16-bit weights | transposed fp32 weights | weight-gradient slabs | resident deep-level run | per-op


@pytest.fixture(scope="module")
def programs():
    return gen.programs()


@pytest.fixture(scope="module")
def golden():
    return gen.load()


def _expected(golden, name):
    if wsis_native.experimental() and gen.needs_experimental(name):
        return golden["experimental"][name]
    return golden["default"][name]


def _layout(ops):
    """(status, regions [(offset, bytes)] * 5, total, lp_off, wt_off) of the plan of ``ops`` under the present environment"""
    fn = wsis_native.hip().wsis_debug_run_ops_layout
    fn.restype = ctypes.c_int32
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]
    n = len(ops)
    out = np.full(11 + 2 * n, -7, dtype=np.int64)
    rc = fn(ops.ctypes.data, n, out.ctypes.data)
    regions = [(int(out[2 * k]), int(out[2 * k + 1])) for k in range(N_REGIONS)]
    return rc, regions, int(out[10]), out[11:11 + n], out[11 + n:]


def test_fixture_holds_every_program_of_both_flavours(golden):
    assert len(CASES) == 15 and set(golden["default"]) == set(CASES)
    assert set(golden["experimental"]) == {n for n in CASES if gen.needs_experimental(n)} and len(golden["experimental"]) == 3
    for table in (golden["default"], golden["experimental"]):
        for sides in table.values():
            assert set(sides) == set(gen.SIDES) and all(set(v) == set(gen.ENVS) for v in sides.values())
    # one revision for both flavours, and an unmodified one
    assert golden["commit"]["default"] == golden["commit"]["experimental"] and not golden["commit"]["default"].endswith("+")


def test_fixture_agrees_with_the_figures_noted_when_it_was_made(golden):
    d = golden["default"]
    assert d["train_dx1"]["fwd"]["default"] == 60_426_752 and d["train_dx1"]["bwd"]["default"] == 11_988_992
    assert d["train_dx1"]["bwd"]["batch_reduce"] == 140_021_760
    assert d["train_dx1"]["fwd"]["no_fwd2"] == 16_640_512 and d["train_dx1"]["bwd"]["no_fwd2"] == 69_295_104
    assert d["train_dx0"]["bwd"]["default"] == 11_059_968
    for name in CASES:
        if name.startswith("lp_"):
            assert d[name]["fwd"]["default"] == 38_533_632 and d[name]["bwd"]["default"] == 512, name
    assert d["train_bn_in"]["fwd"]["default"] == -1 and d["train_stat_fin"]["fwd"]["default"] == -1


@pytest.mark.parametrize("name", CASES)
def test_sizes_are_those_recorded_before_the_layout_had_one_definition(name, programs, golden):
    want = _expected(golden, name)
    for side in gen.SIDES:
        assert gen.sizes(wsis_native.hip(), programs[name][side]) == want[side], side


def _reads_transposed_weight(op, fwd2_on):
    """forward convolutions on the wave-autonomous kernel (channel counts multiples of 32, WSIS_FWD2 on) read B^T; the
    dIn products that are NOT on it read W^T"""
    if op["flags"] & un.F_LP:
        return False
    on_t = fwd2_on and op["Cin"] >= 32 and op["Cin"] % 32 == 0 and op["Cout"] >= 32 and op["Cout"] % 32 == 0
    if op["kind"] == un.OP_CONV:
        return bool(on_t)
    return bool(op["kind"] == un.OP_CONV_BWD and op["out"][0] != 0 and not on_t)


def _check_slots(ops, off, wanted, word, region):
    """a slot for exactly the ops of ``wanted``, in op order, each of K * Cin * Cout words rounded up to ALIGN, inside"""
    at, size = region
    end = 0
    for i, op in enumerate(ops):
        if not wanted[i]:
            assert off[i] == -1, i
            continue
        need = -(-int(op["K"]) * int(op["Cin"]) * int(op["Cout"]) * word // ALIGN) * ALIGN
        assert off[i] == end and off[i] % ALIGN == 0, (i, off[i], end)      # increasing, no gaps, no overlap
        end = int(off[i]) + need
    assert end == size, (end, size)


@pytest.mark.parametrize("env_name", sorted(gen.ENVS))
@pytest.mark.parametrize("name", CASES)
def test_plan_of_the_pass(name, env_name, programs, golden):
    lib = wsis_native.hip()
    want = _expected(golden, name)
    for side in gen.SIDES:
        ops = programs[name][side]
        with gen.environment(gen.ENVS[env_name]):
            rc, regions, total, lp_off, wt_off = _layout(ops)
            size = lib.wsis_run_ops_workspace_bytes(ops.ctypes.data, len(ops))
        if want[side][env_name] < 0:      # a refused list: both entry points say so
            assert rc != 0 and size == -1
            continue
        assert rc == 0 and size == total == want[side][env_name]
        end = 0
        for at, nbytes in regions:       # aligned, in order, disjoint, nothing between them
            assert at % ALIGN == 0 and nbytes % ALIGN == 0 and nbytes >= 0 and at == end
            end = at + nbytes
        assert end == total
        assert regions[-1][1] >= 2 * ALIGN, "the per-op region is never empty"
        fwd2_on = gen.ENVS[env_name].get("WSIS_FWD2", "1") != "0"
        _check_slots(ops, wt_off, [_reads_transposed_weight(op, fwd2_on) for op in ops], 4, regions[1])
        _check_slots(ops, lp_off, [op["kind"] == un.OP_CONV and bool(op["flags"] & un.F_LP) for op in ops], 2, regions[0])
        if not wanted_dw(ops):
            assert regions[2][1] == 0
        if not wsis_native.experimental():
            assert regions[3][1] == 0, "no resident deep-level run in the default build"


def wanted_dw(ops):
    return any(op["kind"] == un.OP_CONV_BWD and op["out"][1] != 0 for op in ops)


def test_deferred_slab_sums_reserve_every_product_its_own_slabs(programs):
    ops = programs["train_dx1"]["bwd"]
    with gen.environment({}):
        _, shared, _, _, _ = _layout(ops)
    with gen.environment({"WSIS_DW_BATCH_REDUCE": "1"}):
        _, each, _, _, _ = _layout(ops)
    assert 0 < shared[2][1] < each[2][1]
    assert [r[1] for r in shared[:2] + shared[3:]] == [r[1] for r in each[:2] + each[3:]], "the other regions keep their size"


def test_refused_lists_have_no_plan():
    lib = wsis_native.hip()
    op = np.zeros(1, dtype=un.OP_DTYPE)
    op["kind"], op["flags"], op["M_in"], op["M_out"], op["K"], op["Cin"], op["Cout"] = un.OP_CONV_BWD, un.F_LP, 100, 100, 27, 64, 64
    rc, _, _, _, _ = _layout(op)
    assert rc != 0 and "op 0" in lib.wsis_last_error().decode()
    assert lib.wsis_run_ops_workspace_bytes(op.ctypes.data, 1) == -1
    # a convolution on the transposed-weight path without weights: refused by the plan, before anything is enqueued
    conv = np.zeros(1, dtype=un.OP_DTYPE)
    conv["kind"], conv["M_in"], conv["M_out"], conv["K"], conv["Cin"], conv["Cout"] = un.OP_CONV, 100, 100, 27, 64, 64
    with gen.environment({}):
        rc, _, _, _, _ = _layout(conv)
        assert rc != 0 and "without weights" in lib.wsis_last_error().decode()
        assert lib.wsis_run_ops(conv.ctypes.data, 1, None, 0, None, None) != 0
    # an empty list: only the (minimum) per-op region
    rc, regions, total, _, _ = _layout(np.zeros(0, dtype=un.OP_DTYPE))
    assert rc == 0 and total == 2 * ALIGN and [r[1] for r in regions] == [0, 0, 0, 0, 2 * ALIGN]
