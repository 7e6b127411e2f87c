"""CPU: the launch plan of the fp32 weight gradient (csrc/spconv_dw2.hip: dw_plan) without a GPU.

* the three size queries answer what tests/golden/dw_plan_golden.json recorded at the revision before the plan had one
  definition (tests/golden/make_dw_plan_golden.py), for every shape of tests/dw_plan_ref.py;
* the wave count of the plan query wsis_debug_dw_plan -- dw_plan(), the function the launch itself calls -- is the one
  that revision's diagnostic reported, under each hint;
* the plan query agrees field by field with the Python restatement of the rule (dw_plan_ref.plan_ref);
* a plan never needs more workspace than the size query promised, at any alignment and either hint;
* the shape table reaches every kind and every clause of the slab-count rule (the reference says which case reaches what).

All comparisons are exact: sizes, grids and kinds are integers."""
import contextlib
import os

import pytest

import dw_plan_ref as ref
import wsis_native
from tests.golden import make_dw_plan_golden as gen

CASES = {c.name: c for c in ref.CASES}
FAMILY = (ref.DW3, ref.RING, ref.RING_XCD)


@pytest.fixture(scope="module")
def golden():
    return gen.load()


@contextlib.contextmanager
def launch_state(case, rows):
    """the hint and the switches a launch of ``case`` reads"""
    saved = {k: os.environ.pop(k, None) for k in ("WSIS_DW3", "WSIS_IN_CONV")}
    os.environ["WSIS_DW3"] = str(case.dw3)
    assert ref.lib().wsis_hint_batch_rows(rows) == 0
    try:
        yield
    finally:
        assert ref.lib().wsis_hint_batch_rows(0) == 0
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def test_fixture_holds_every_shape_at_an_unmodified_revision(golden):
    assert set(golden["cases"]) == set(CASES)
    assert len(golden["commit"]) == 40 and not golden["commit"].endswith("+")
    # figures noted when it was made: level 1 of the benchmark scene at 64 -> 64, one and two workgroups per CU
    g = golden["cases"]["k27_64_64_m26819"]
    assert g["ws"] == 27_934_976 and g["bn_ws"] == 14_156_032 and g["waves"] == {
        "0": 1024, "249999": 1024, "250000": 2048, "625000": 2048}
    assert golden["cases"]["refused_k129"]["ws"] == -1


@pytest.mark.parametrize("name", sorted(CASES))
def test_size_queries_are_those_recorded_before_the_plan_had_one_definition(name, golden):
    with launch_state(CASES[name], 0):
        now = gen.sizes(ref.lib(), CASES[name])
    want = golden["cases"][name]
    assert now == {k: want[k] for k in ("ws", "bn_supported", "bn_ws")}


@pytest.mark.parametrize("name", sorted(CASES))
def test_wave_count_is_the_one_the_diagnostic_reported(name, golden):
    """(the recorded diagnostic knew the plain form only, took any alignment and any row counts without a table: a case
    the plan puts on the wave-autonomous kernels must have a recorded count, and a shape without one is never put there)"""
    case, want = CASES[name], golden["cases"][name]["waves"]
    if case.swapped:
        return
    for rows in ref.HINTS:
        with launch_state(case, rows):
            p = ref.plan_lib(case)
        if p is not None and p["kind"] in FAMILY:
            assert want is not None and p["gx"] * p["gy"] * ref.WGW == want[str(rows)], rows
        else:
            assert want is None or case.align != ref.ALIGNED or (case.table == ref.NO_TABLE and case.M_in != case.M_out), rows


@pytest.mark.parametrize("name", sorted(CASES))
def test_plan_query_agrees_with_the_restated_rule(name):
    case = CASES[name]
    for rows in ref.HINTS:
        want = ref.reference(case, rows)
        with launch_state(case, rows):
            got = ref.plan_lib(case)
        if want is None:
            assert got is None, rows
            continue
        assert got is not None, rows
        assert ref.Plan(*(got[f] for f in ref.Plan._fields)) == want, rows


@pytest.mark.parametrize("name", sorted(CASES))
def test_a_plan_never_needs_more_workspace_than_the_size_query_promised(name, golden):
    case = CASES[name]
    aligns = (ref.ALIGNED, ref.X8 | ref.DY16 | ref.DW16 | ref.WS16, ref.DY16 | ref.DW16 | ref.WS16, ref.X16 | ref.X8, 0)
    g = golden["cases"][name]
    promised = g["bn_ws"] if case.swapped else g["ws"]
    largest = -1
    for align in aligns:
        for dw3 in (0, 1):
            for rows in ref.HINTS:
                c = case._replace(align=align, dw3=dw3)
                with launch_state(c, rows):
                    p = ref.plan_lib(c)
                if p is None:
                    continue
                assert 0 <= p["ws_bytes"] <= promised, (align, dw3, rows, p)
                largest = max(largest, p["ws_bytes"])
                if p["kind"] in FAMILY + (ref.SWAPPED,):      # P slabs of dW and a spare line
                    assert p["ws_bytes"] == p["P"] * case.K * case.Cin * case.Cout * 4 + 256
    if case.swapped and largest > 0:
        assert largest == promised, "the own-rows form has one kind: the query is its larger hint plan"


def test_the_table_reaches_every_kind_and_every_clause_of_the_slab_count_rule():
    kinds, clauses = {}, {}
    for case in ref.CASES:
        for rows in ref.HINTS:
            hit = set()
            p = ref.reference(case, rows, hit)
            if p is None:
                kinds.setdefault("refused", case.name)
                continue
            kinds.setdefault(ref.KIND_NAMES[p.kind], case.name)
            for c in hit:
                clauses.setdefault(c, case.name)
    # (the XCD deal of the LDS ring is behind a knob of the EXPERIMENTAL build: below)
    assert set(kinds) == set(ref.KIND_NAMES) - {"ring_xcd"} | {"refused"}, kinds
    assert set(clauses) == set(ref.P_CLAUSES), clauses
    # the cases the issue names for a branch reach it
    P = lambda name, rows=0: ref.reference(CASES[name], rows).P
    assert P("k27_96_96_m26819") == 7                                          # round-down: 7 x 36 = 252 workgroups
    assert P("k27_64_64_m262112") == 16 and P("k27_64_64_m262113") == 32       # the 8,192-slice switch
    assert P("k27_64_64_m26819", 249999) == 16 and P("k27_64_64_m26819", 250000) == 32      # the hint threshold
    assert P("dense_2080_few") == 4 and P("dense_2080_wide") == 32 and P("dense_2080_mid") == 8
    assert P("k27_32_32_m33") == 1 and P("k27_32_32_m4095") == 32              # the cap by slices
    kind = lambda name: ref.reference(CASES[name], 0).kind
    assert (kind("dw3_pitch_in"), kind("dw3_pitch_out")) == (ref.DW3, ref.RING)
    assert (kind("dw3_rowid_in"), kind("dw3_rowid_out")) == (ref.DW3, ref.RING)
    assert (kind("fits_in"), kind("fits_out")) == (ref.DW3, ref.GENERIC) and ref.reference(CASES["too_large"], 0) is None
    assert (kind("in_conv_x8"), kind("in_conv_x4"), kind("align_x8")) == (ref.IN_CONV, ref.GENERIC, ref.GENERIC)


def test_the_xcd_deal_follows_its_knob(monkeypatch):
    """rows >= WSIS_DW2_XCD and a slab count that is a multiple of 8: restated always, asked of the library where the knob
    is live"""
    big, small = CASES["ring_k27_64_m26819"], CASES["ring_k27_64_m33"]
    args = lambda c: (c.M_in, c.M_out, c.K, c.Cin, c.Cout, c.table, c.align, False)
    assert ref.plan_ref(*args(big), dw3=0, xcd_rows=1000).kind == ref.RING_XCD
    assert ref.plan_ref(*args(big), dw3=0, xcd_rows=30000).kind == ref.RING
    assert ref.plan_ref(*args(small), dw3=0, xcd_rows=1).kind == ref.RING          # one slab: no multiple of 8
    assert ref.plan_ref(*args(big), dw3=1, xcd_rows=1000).kind == ref.DW3
    if wsis_native.experimental():
        monkeypatch.setenv("WSIS_DW2_XCD", "1000")
        with launch_state(big, 0):
            assert ref.plan_lib(big)["kind"] == ref.RING_XCD
        with launch_state(small, 0):
            assert ref.plan_lib(small)["kind"] == ref.RING
