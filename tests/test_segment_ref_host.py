"""Host: the numpy reference of tests/segment_ref.py against Python loops (ties, empty segments, +-inf), against
oracle.scatter_ref.scatter with fp64 autograd on tie-free data, and its error bound against numpy's own fp32 sums on every
float input tests/test_gpu_segment_edges.py runs -- which shows that an honest fp32 summation passes there.  No GPU."""
import numpy as np
import pytest
import torch

import segment_ref as ref
from oracle import scatter_ref

INF = float("inf")


# ---- brute force ------------------------------------------------------------------------------------------------------

def loops_csr(index, S):
    perm = [p for s in range(S) for p in range(len(index)) if index[p] == s]
    offsets = [sum(1 for v in index if v < s) for s in range(S + 1)]
    return perm, offsets


def loops_reduce(src, index, S, kind):
    N, C = src.shape
    out = [[0.0] * C for _ in range(S)]
    arg = [[N] * C for _ in range(S)]
    for s in range(S):
        rows = [p for p in range(N) if index[p] == s]
        for c in range(C):
            if not rows:
                continue
            vals = [float(src[p, c]) for p in rows]
            if kind == "sum":
                out[s][c] = sum(vals)
            elif kind == "mean":
                out[s][c] = sum(vals) / len(vals)
            else:
                best = max(vals) if kind == "max" else min(vals)
                out[s][c] = best
                arg[s][c] = rows[vals.index(best)]          # the first row that attains it
    return np.array(out, np.float64).reshape(S, C), np.array(arg, np.int64).reshape(S, C)


def loops_bwd(dout, index, S, kind, arg):
    N, C = len(index), dout.shape[1]
    d = np.zeros((N, C))
    for p in range(N):
        s = index[p]
        n = sum(1 for v in index if v == s)
        for c in range(C):
            if kind == "sum":
                d[p, c] = dout[s, c]
            elif kind == "mean":
                d[p, c] = dout[s, c] / n
            elif arg[s, c] == p:
                d[p, c] = dout[s, c]
    return d


def small_cases():
    rng = np.random.default_rng(5)
    ties = ref.tie_rows(rng, (40, 3))
    idx = rng.integers(1, 7, 40)                              # segments 0 and 7, 8 stay empty
    idx[idx == 4] = 5                                         # and 4
    infs = ties.copy()
    infs[idx == 2] = -INF                                     # a segment of -inf only
    infs[idx == 3] = INF                                      # and one of +inf only
    infs[np.flatnonzero(idx == 5)[1], 0] = INF                # single infinities among finite rows
    infs[np.flatnonzero(idx == 5)[2], 1] = -INF
    return [("ties", ties, idx, 9), ("inf", infs, idx, 9), ("one_row", ties[:1], np.array([0]), 1),
            ("one_segment", ties, np.zeros(40, np.int64), 1), ("no_rows", ties[:0], np.zeros(0, np.int64), 5),
            ("no_segments", ties[:0], np.zeros(0, np.int64), 0),
            ("descending", ties[:9], np.arange(8, -1, -1), 9)]


@pytest.mark.parametrize("name,src,index,S", small_cases(), ids=[c[0] for c in small_cases()])
def test_reference_equals_python_loops(name, src, index, S):
    perm, offsets = ref.csr(index, S)
    lp, lo = loops_csr(index, S)
    assert perm.tolist() == lp and offsets.tolist() == lo
    rng = np.random.default_rng(6)
    dout = rng.integers(-8, 9, (S, src.shape[1])).astype(np.float64)
    for kind in ref.KINDS:
        if name == "inf" and kind in ("sum", "mean"):
            continue                                          # inf - inf: outside the contract
        val, arg = ref.reduce(src, index, S, kind)
        lv, la = loops_reduce(src, index, S, kind)
        assert np.array_equal(val, lv), (name, kind)
        assert not np.signbit(val[val == 0]).any()
        if kind in ("max", "min"):
            assert np.array_equal(arg, la), (name, kind)
        assert np.array_equal(ref.reduce_bwd(dout, index, S, kind, arg), loops_bwd(dout, index, S, kind, la)), (name, kind)


def test_reference_arg_is_the_first_row_of_a_tie():
    src = np.array([[1.0], [2.0], [2.0], [-3.0], [-3.0], [2.0]])
    index = np.array([0, 0, 0, 2, 2, 0])
    val, arg = ref.reduce(src, index, 4, "max")
    assert val[:, 0].tolist() == [2.0, 0.0, -3.0, 0.0] and arg[:, 0].tolist() == [1, 6, 3, 6]
    val, arg = ref.reduce(src, index, 4, "min")
    assert val[:, 0].tolist() == [1.0, 0.0, -3.0, 0.0] and arg[:, 0].tolist() == [0, 6, 3, 6]
    d = ref.reduce_bwd(np.array([[10.0], [20.0], [30.0], [40.0]]), index, 4, "max", ref.reduce(src, index, 4, "max")[1])
    assert d[:, 0].tolist() == [0.0, 10.0, 0.0, 30.0, 0.0, 0.0]          # the whole gradient to one row, no split


# ---- the oracle (tie-free data: its max backward splits a tie) -----------------------------------------------------------

@pytest.mark.parametrize("kind", ref.KINDS)
@pytest.mark.parametrize("shape", [(300,), (300, 7), (120, 2, 5)])
def test_reference_equals_the_oracle_scatter_on_tie_free_data(shape, kind):
    g = torch.Generator().manual_seed(len(shape))
    src = torch.randn(shape, generator=g, dtype=torch.float64)
    index = torch.randint(0, 23, (shape[0],), generator=g)
    index[index == 9] = 10                                    # an empty segment
    S = 25                                                    # and two trailing ones
    xr = src.clone().requires_grad_(True)
    want = scatter_ref.scatter(xr, index, 0, S, kind)
    dout = torch.randn(want.shape, generator=g, dtype=torch.float64)
    want.backward(dout)
    val, arg = ref.reduce(src.numpy(), index.numpy(), S, kind)
    d = ref.reduce_bwd(dout.numpy(), index.numpy(), S, kind, arg)
    # both are fp64; the two sums differ in order only: 2^-52 per addition
    mag = np.abs(ref.reduce(np.abs(src.numpy()), index.numpy(), S, "sum")[0])
    tol = 0.0 if kind in ("max", "min") else 64 * 2.0 ** -52 * mag
    assert (np.abs(val - want.detach().numpy()) <= tol).all()
    assert (np.abs(d - xr.grad.numpy()) <= 2.0 ** -52 * np.abs(d)).all()


# ---- the inputs of the device tests ----------------------------------------------------------------------------------

def test_geometry_index_has_the_stated_segment_sizes():
    for C in ref.GEOMETRY_C:
        G = 64 // ref.cp_of(C)
        index, S = ref.geometry_index(C)
        n = ref.counts(index, S)
        assert S == 16 and n.tolist() == [0, 0] + ref.geometry_sizes(C) + [0, 0, 0]
        assert n.max() == 16 * G + 3 and {7 * G, 7 * G + 1, 8 * G - 1, 8 * G, 8 * G + 1, G - 1, G, G + 1} <= set(n.tolist())
        assert (np.diff(index) < 0).any()                     # shuffled
    assert ref.counts(*ref.geometry_index(1)).max() == 1027
    assert sorted({ref.cp_of(C) for C in ref.GEOMETRY_C}) == [1, 2, 4, 8, 16, 32, 64]


def test_narrow_index_sits_on_both_sides_of_the_switch():
    for pad, N in (("below", 70), ("edge", 159), ("at", 160)):
        index, S = ref.narrow_index(pad)
        n = ref.counts(index, S)
        assert S == 40 and len(index) == N and n[:10].tolist() == list(ref.NARROW_SIZES) and (n[30:] == 0).all()
        assert (N < 4 * S) == (pad != "at")
    for which, blocks_per in (("wave", 4), ("narrow", 32)):
        index, S, C = ref.cap_case(which)
        assert S > 256 * 16 * blocks_per and index.max() == S - 1 and index.min() == 0
        assert (ref.counts(index, S) == 0).any()
    assert len(ref.cap_case("narrow")[0]) < 4 * ref.cap_case("narrow")[1] and ref.cp_of(20) == 32


def float_inputs():
    for C in ref.GEOMETRY_C:
        index, S = ref.geometry_index(C)
        yield f"geometry-{C}", ref.case_rows("wide", 2000 + C, (len(index), C)), index, S
    for C in ref.NARROW_C + (16, 36):
        for pad in ("below", "edge", "at"):
            index, S = ref.narrow_index(pad)
            yield f"narrow-{C}-{pad}", ref.case_rows("wide", 3000 + C, (len(index), C)), index, S
    index, S = ref.narrow_index("below")
    for C in (20, 32):                                        # the misaligned views
        yield f"misaligned-{C}", ref.case_rows("wide", 7000 + C, (len(index), C)), index, S
    index, S = ref.geometry_index(8)
    yield "3-D", ref.case_rows("wide", 13, (len(index), 2, 5)), index, S
    for C in (1, 20, 70):
        yield f"one-row-{C}", ref.case_rows("wide", 21, (1, C)), np.array([2], np.int64), 4


@pytest.mark.parametrize("kind", ["sum", "mean"])
def test_sum_bound_holds_for_numpys_fp32_sum_on_the_device_inputs(kind):
    worst = 0.0
    for name, src, index, S in float_inputs():
        val, _ = ref.reduce(src, index, S, kind)
        bound = ref.sum_bound(src, index, S, kind)
        err = np.abs(ref.fp32_reduceat(src, index, S, kind).astype(np.float64) - val)
        assert (err <= bound).all(), (name, float((err - bound).max()))
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        assert (bound[ref.counts(index, S) == 0] == 0).all()  # an empty segment must be exactly 0
    print(f"{kind}: numpy's fp32 reduceat uses at most {worst:.3g} of the bound")
    assert worst > 0.0                                        # the inputs do round: the bound is not vacuous


@pytest.mark.parametrize("kind", ["sum", "mean"])
def test_integer_rows_sum_exactly_in_fp32(kind):
    """every partial sum of the integer rows stays below 2^24, so fp32 sums them exactly in any order; the mean is then
    one fp32 division of two exact numbers"""
    for C in (1, 8, 33):
        index, S = ref.geometry_index(C)
        src = ref.case_rows("int", 4000 + C, (len(index), C))
        assert np.abs(src).max() <= 8 and (src == np.round(src)).all() and 8 * ref.counts(index, S).max() < 2 ** 24
        val, _ = ref.reduce(src, index, S, "sum")
        got = ref.fp32_reduceat(src, index, S, kind)
        if kind == "sum":
            assert np.array_equal(got.astype(np.float64), val)
        else:
            n = np.maximum(ref.counts(index, S), 1).astype(np.float32)[:, None]
            assert np.array_equal(got, val.astype(np.float32) / n)
