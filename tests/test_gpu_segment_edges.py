"""GPU: the segment reductions, the CSR builds (csrc/segment.hip, torch_scatter/__init__.py) and the row gather
(gather_rows of csrc/core.hip, wsis_ops.gather_rows) against the numpy fp64 reference of tests/segment_ref.py at every
launch branch.

Two kinds of data.  Integer-valued fp32 rows in [-8, 8]: every partial sum is exact in fp32, so sum, max, min, arg and
every gradient must equal the reference bit for bit, and mean must equal the one fp32 division np.float32(sum) /
np.float32(n) -- this catches a dropped, doubled or misplaced row.  Floats with six decades of dynamic range: sum and mean
within segment_ref.sum_bound, the bound of any fp32 summation order ((n + 1) 2^-24 sum|x|); max, min (a selection) and
every gradient (a copy or one division) still bit for bit.  No comparison here uses a tuned tolerance.

Branches, read from the launch conditions of wsis_segment_reduce_fwd / _bwd, wsis_segment_csr_batch and wsis_gather_rows:

* CP = 1, 2, 4, 8, 16, 32, 64: test_channel_geometry at C = 1, 2, 3 | 4, 7 | 8, 12 | 16, 20 | 32, 33 | 64; C = 65, 70, 128,
  130 take two or three passes of 64 channels, the last one partly idle;
* the eight-rows-per-trip loop (entered by group g of G = 64 / CP when the segment has more than 7 G + g rows): segments
  of 7 G + 1 (group 0 alone), 8 G (every group, no tail) and 16 G + 3 rows (two trips); the row-by-row tail: all others;
* grid caps of 4096 blocks: test_grid_caps[wave] (S = 20000 > 16384), test_grid_caps[narrow] (S = 140000 > 131072);
* narrow kernel (sum / mean, CP == 32, C % 4 == 0, N < 4 S, 16-byte src and out): test_narrow_kernel_* at C = 20, 24, 28,
  32 with N < 4 S and N = 4 S - 1, test_one_row[20]; wave kernel instead: the same at N = 4 S, C = 16 and 36,
  WSIS_SEGMENT_NARROW=0, and test_misaligned_* (pointer 4 bytes past a 16-byte boundary);
* segment_bwd_kernel<4> (C % 4 == 0, 16-byte dout and dsrc): C = 4, 8, 12, 16, 20, 32, 64, 128; <1>: every other C and
  test_misaligned_* at C = 20, 32; segment_max_bwd_kernel: every max / min case;
* max tie rule: inside a row group test_ties_go_to_the_first_row (C = 1: 64 groups walk 600 equal rows; C = 33, 70: one
  group), across the butterfly the same at C = 1, 2, 8, 32 and test_ties_that_straddle_the_two_row_groups;
* counting CSR (WSIS_CSR_COUNTING=1) orderings: segments of 0 or 1 rows skipped, 2 .. 64 ranked in registers, 65 .. 2048
  by the network in LDS (about 200 rows per segment), more by the network in memory (3000 rows); the sort otherwise;
* table number 7 (key bits 32 .. 34): test_batched_csr_*[full]; empty tables first, middle, last and S = 0: [gaps];
* gather_rows_kernel<int32 | int64, float4>: C = 4, 20, 32; <., scalar>: C = 1, 3, 6, 130 and test_gather_rows_misaligned_*.

NaN inputs are outside the contract of these kernels (max compares with ``>``) and are not tested.  Ids outside [0, S)
are a caller error (SegmentCSR's docstring) and are not tested either."""
import ctypes

import numpy as np
import pytest
import torch

import segment_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 0x5a5a5a5a
GUARD = 64
_REF = {}


def ts():
    import torch_scatter
    return torch_scatter


def native():
    import wsis_native
    return wsis_native


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def assert_bits(what, got, want):
    """same shape, same type, same bytes"""
    got = host(got) if torch.is_tensor(got) else np.asarray(got)
    want = np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.tobytes() != want.tobytes():
        g, w = got.reshape(-1), want.reshape(-1)
        bad = np.flatnonzero(g.view(np.uint32 if g.itemsize == 4 else np.uint64) !=
                             w.view(np.uint32 if w.itemsize == 4 else np.uint64))
        raise AssertionError(f"{what}: {bad.size} of {g.size} words differ, first at {bad[0]}: got {g[bad[0]]!r}, "
                             f"want {w[bad[0]]!r}")


def assert_bound(what, got, want, bound):
    err = np.abs(host(got).astype(np.float64) - want)
    worst = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    print(f"{what}: largest error {float(err.max()) if err.size else 0.0:.3g}, largest error / bound {worst:.3g}")
    assert (err <= bound).all(), what


def misaligned(a):
    """a contiguous device view of ``a`` that starts at element 1 of a flat buffer: its pointer is 4 bytes past a
    16-byte boundary, and contiguous() does not copy it"""
    a = np.ascontiguousarray(a)
    buf = torch.zeros(a.size + 1, dtype=torch.from_numpy(a).dtype, device=DEV)
    view = buf[1:1 + a.size].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.is_contiguous() and view.data_ptr() % 16 == 4 and view.contiguous().data_ptr() == view.data_ptr()
    return view


def reference(src, index, S, kind):
    """(value fp64, arg, counts) of one case, computed once per (array, kind)"""
    key = (id(src), id(index), S, kind)
    if key not in _REF:
        _REF[key] = (src, index) + ref.reduce(src, index, S, kind) + (ref.counts(index, S),)      # (keeps the arrays alive)
    return _REF[key][2:]


def expected_forward(src, index, S, kind):
    """(fp32 array the device must reproduce bit for bit, or None where only the bound holds; value fp64; arg)"""
    val, arg, n = reference(src, index, S, kind)
    exact_data = bool((src == np.round(src)).all()) and np.isfinite(src).all()
    if kind in ("max", "min"):
        return val.astype(np.float32), val, arg
    if not exact_data:
        return None, val, arg
    if kind == "sum":
        return val.astype(np.float32), val, arg
    total = reference(src, index, S, "sum")[0].astype(np.float32)
    div = np.maximum(n, 1).astype(np.float32).reshape((S,) + (1,) * (total.ndim - 1))
    return total / div, val, arg


def expected_backward(dout, index, S, kind, arg):
    """fp32 gradient, bit for bit: a copy (sum), one fp32 division (mean), the arg row alone (max / min)"""
    if kind == "mean":
        n = np.maximum(ref.counts(index, S), 1).astype(np.float32)[index]
        return (dout[index] / n.reshape((len(index),) + (1,) * (dout.ndim - 1))).astype(np.float32)
    return ref.reduce_bwd(dout, index, S, kind, arg).astype(np.float32)


def run(src_t, index_t, kind, dout_t, **kw):
    x = src_t.detach().requires_grad_(True)
    out = ts().scatter(x, index_t, reduce=kind, **kw)
    out.backward(dout_t)
    return out.detach(), x.grad


def check_case(what, src, index, S, kinds=ref.KINDS, seed=0, with_arg=True, dim_size="S", src_t=None, dout_wrap=dev, **kw):
    """all of ``kinds`` forward and backward through torch_scatter.scatter against the reference; returns the device
    results {kind: (out, grad)} for comparisons between launches"""
    index_t = dev(index)
    src_t = dev(src) if src_t is None else src_t
    exact_data = bool((src == np.round(src)).all())
    dout = ref.case_rows("int" if exact_data else "wide", 9000 + seed, (S,) + src.shape[1:])
    if dim_size == "S":
        kw["dim_size"] = S
    elif dim_size is not None:
        kw["dim_size"] = dim_size
    results = {}
    for kind in kinds:
        want32, val, arg = expected_forward(src, index, S, kind)
        out, grad = run(src_t, index_t, kind, dout_wrap(dout), **kw)
        if want32 is not None:
            assert_bits(f"{what} {kind} forward", out, want32)
        else:
            assert out.shape == val.shape
            assert_bound(f"{what} {kind} forward", out, val, ref.sum_bound(src, index, S, kind))
            assert_bits(f"{what} {kind} empty segments", out[dev(ref.counts(index, S) == 0)],
                        np.zeros((int((ref.counts(index, S) == 0).sum()),) + src.shape[1:], np.float32))
        assert_bits(f"{what} {kind} backward", grad, expected_backward(dout, index, S, kind, arg))
        if with_arg and kind in ("max", "min"):
            fn = ts().scatter_max if kind == "max" else ts().scatter_min
            v2, a2 = fn(src_t, index_t, dim_size=kw.get("dim_size"))
            assert_bits(f"{what} scatter_{kind} value", v2, want32)
            assert_bits(f"{what} scatter_{kind} arg", a2, arg)
        results[kind] = (out, grad)
    return results


# ---- channel geometry ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("data", ["int", "wide"])
@pytest.mark.parametrize("C", ref.GEOMETRY_C)
def test_channel_geometry(C, data):
    """every CP = 1 .. 64 (and two passes over the channels at C > 64), with segments of 0, 1, G - 1, G, G + 1 rows
    (some row groups idle), 7 G (the last size that stays in the row-by-row tail), 7 G + 1 (group 0 alone takes one
    eight-row trip), 8 G - 1, 8 G (every group one trip, no tail), 8 G + 1 and 16 G + 3 (two trips and a tail); rows
    shuffled, two leading and three trailing empty segments.  N >= 4 S where CP = 32: the wave-per-segment kernel throughout."""
    index, S = ref.geometry_index(C)
    src = ref.case_rows(data, 2000 + C, (len(index), C))
    assert ref.cp_of(C) != 32 or len(index) >= 4 * S
    check_case(f"C={C} {data}", src, index, S, seed=C)


def test_src_shapes_dims_and_dim_size():
    """a 1-D src (with dim=0 and dim=-1), a 3-D src of shape (N, 2, 5), dim_size=None (S = max + 1) and a dim_size
    beyond max + 1"""
    index, S = ref.geometry_index(8)
    top = int(index.max()) + 1
    assert top < S
    one_d = ref.case_rows("int", 11, (len(index),))
    three_d = ref.case_rows("int", 12, (len(index), 2, 5))
    check_case("1-D", one_d, index, S, seed=1)
    check_case("1-D dim=-1", one_d, index, S, seed=1, with_arg=False, dim=-1)
    check_case("3-D", three_d, index, S, seed=2)
    check_case("3-D wide", ref.case_rows("wide", 13, (len(index), 2, 5)), index, S, seed=3)
    check_case("dim_size=None", three_d, index, top, seed=4, dim_size=None)
    check_case("dim_size=S+9", one_d, index, S + 9, seed=5, dim_size=S + 9)
    v, a = ts().scatter_max(dev(one_d), dev(index), dim=-1, dim_size=S)
    assert_bits("scatter_max dim=-1", a, reference(one_d, index, S, "max")[1])


@pytest.mark.parametrize("shape", [(0,), (0, 7), (0, 2, 5)], ids=["1-D", "2-D", "3-D"])
def test_no_rows(shape):
    """N = 0 with dim_size = 5 (every segment empty: zeros, arg 0 = N) and S = 0 (dim_size 0 and None: empty results);
    the gradient is an empty tensor of src's shape"""
    src = np.zeros(shape, np.float32)
    index = np.zeros(0, np.int64)
    check_case("N=0 S=5", src, index, 5)
    check_case("N=0 S=0", src, index, 0)
    check_case("N=0 dim_size=None", src, index, 0, dim_size=None, with_arg=False)


@pytest.mark.parametrize("C", [1, 20, 70])
def test_one_row(C):
    src = ref.case_rows("wide", 21, (1, C))
    check_case("N=1 S=1", src, np.array([0], np.int64), 1)
    check_case("N=1 S=4", src, np.array([2], np.int64), 4)
    check_case("N=1 dim_size=None", src, np.array([2], np.int64), 3, dim_size=None)


# ---- narrow kernel ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("data", ["int", "wide"])
@pytest.mark.parametrize("C", ref.NARROW_C + (16, 36))
def test_narrow_kernel_on_both_sides_of_its_switch(monkeypatch, C, data):
    """segments of 0, 1, 2, 3, 4 (one four-row trip), 5, 7, 8 (two trips), 9 and 11 rows among one-row and empty ones at
    N < 4 S and N = 4 S - 1 (the narrow kernel for C = 20 .. 32) and at N = 4 S (the wave kernel); C = 16 (CP = 16) and
    C = 36 (CP = 64) take the wave kernel at every N.  Each launch is bit-identical to the wave kernel's
    (WSIS_SEGMENT_NARROW=0), as the narrow kernel's comment promises."""
    for pad in ("below", "edge", "at"):
        index, S = ref.narrow_index(pad)
        src = ref.case_rows(data, 3000 + C, (len(index), C))
        monkeypatch.delenv("WSIS_SEGMENT_NARROW", raising=False)
        got = check_case(f"C={C} {pad} {data}", src, index, S, seed=C, with_arg=False)
        monkeypatch.setenv("WSIS_SEGMENT_NARROW", "0")
        wave = check_case(f"C={C} {pad} {data} wave", src, index, S, kinds=("sum", "mean"), seed=C)
        for kind in ("sum", "mean"):
            assert torch.equal(got[kind][0], wave[kind][0]) and torch.equal(got[kind][1], wave[kind][1]), (pad, kind)


@pytest.mark.parametrize("which", ["wave", "narrow"])
def test_grid_caps(which):
    """S = 20000 at C = 8: 5000 blocks of four waves wanted, 4096 launched -- the wave-per-segment kernel strides;
    S = 140000, N = 150000 at C = 20: 4375 blocks of 32 segments wanted -- the narrow kernel strides"""
    index, S, C = ref.cap_case(which)
    assert len(index) < 4 * S and (which == "wave") == (ref.cp_of(C) != 32)
    src = ref.case_rows("int", 5000 + C, (len(index), C))
    check_case(which, src, index, S, kinds=("sum", "mean"))


# ---- ties and infinities ------------------------------------------------------------------------------------------------

def tie_case(C):
    """values from {-2 .. 2} on the sizes of the channel geometry, plus a segment of 600 equal rows"""
    rng = np.random.default_rng(6000 + C)
    index, S = ref.index_of_sizes(rng, ref.geometry_sizes(C) + [600], lead=1, trail=1)
    src = ref.case_rows("tie", 6100 + C, (len(index), C))
    src[index == S - 2] = 1.0
    return src, index, S


@pytest.mark.parametrize("C", [1, 2, 8, 32, 33, 70])
def test_ties_go_to_the_first_row(C):
    """most segments tie: the first row of a row group wins inside the group (C = 1: 64 groups walk the 600 equal rows;
    C = 33, 70: one group), the smaller original row wins across the butterfly (C = 32: two groups); the whole gradient
    goes to that row, as the value and arg of scatter_max / scatter_min say"""
    src, index, S = tie_case(C)
    check_case(f"ties C={C}", src, index, S, kinds=("max", "min"), seed=C)
    arg = reference(src, index, S, "max")[1]
    assert (arg[S - 2] == np.flatnonzero(index == S - 2)[0]).all()


def test_ties_that_straddle_the_two_row_groups():
    """C = 32, two row groups (even and odd positions of a segment): the extreme sits in both groups, first in the odd
    one (rows 1, 2, 4 of segment 0), first in the even one (rows 0, 1 of segment 1), and only in the odd one"""
    C = 32
    col = np.array([0, 2, 2, 1, 2, 0,   2, 2, 0, 1, 2,   -1, 1, -1, 1], np.float32)
    index = np.array([0] * 6 + [1] * 5 + [2] * 4, np.int64)
    src = np.repeat(col[:, None], C, axis=1)
    src[:, 1::2] *= -1                                         # odd channels: the same pattern under min
    src += 0.0                                                 # (no negative zero among the inputs)
    check_case("straddle", src, index, 3, kinds=("max", "min"))
    assert reference(src, index, 3, "max")[1][:, 0].tolist() == [1, 6, 12]
    perm = np.random.default_rng(3).permutation(len(index))    # and with the rows out of order
    check_case("straddle shuffled", src[perm], index[perm], 3, kinds=("max", "min"))


@pytest.mark.parametrize("C", [1, 32, 70])
def test_infinite_segments(C):
    """a segment of -inf only under max, of +inf only under min: the value stays infinite, arg is the segment's first
    row and the gradient goes there; single infinities among finite rows win or lose as numbers do"""
    src, index, S = tie_case(C)
    n = ref.counts(index, S)
    big, small = S - 3, 2                                      # the segments of 16 G + 3 rows and of one row
    assert n[big] == n[:S - 2].max() and n[small] == 1
    for kind, inf in (("max", -np.inf), ("min", np.inf)):
        x = src.copy()
        x[index == big] = inf
        x[index == small] = inf
        x[np.flatnonzero(index == S - 2)[5]] = inf             # among the 600 equal rows: one row that loses,
        x[np.flatnonzero(index == S - 2)[7], 0] = -inf         # and one value that wins
        res = check_case(f"inf C={C}", x, index, S, kinds=(kind,), seed=C)
        assert torch.isinf(res[kind][0][big]).all() and torch.isinf(res[kind][0][small]).all()
        arg = reference(x, index, S, kind)[1]
        assert (arg[big] == np.flatnonzero(index == big)[0]).all() and (arg[small] == np.flatnonzero(index == small)[0]).all()


# ---- misaligned views ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("data", ["int", "wide"])
@pytest.mark.parametrize("C", [20, 32])
def test_misaligned_src_and_gradient_views(C, data):
    """src and the incoming gradient as contiguous views that start at element 1 of a flat buffer (4 bytes past a
    16-byte boundary; contiguous() does not copy them): the narrow forward and the float4 backward must fall back to the
    scalar kernels -- same bits as from aligned clones, and the reference's"""
    index, S = ref.narrow_index("below")
    src = ref.case_rows(data, 7000 + C, (len(index), C))
    aligned = check_case(f"aligned C={C}", src, index, S, seed=C, with_arg=False)
    for what, src_t, wrap in (("src", misaligned(src), dev), ("dout", None, misaligned), ("both", misaligned(src), misaligned)):
        got = check_case(f"misaligned {what} C={C}", src, index, S, seed=C, with_arg=what == "both", src_t=src_t, dout_wrap=wrap)
        for kind in ref.KINDS:
            assert torch.equal(got[kind][0], aligned[kind][0]) and torch.equal(got[kind][1], aligned[kind][1]), (what, kind)


# ---- straight through the C ABI: every word written, no word beyond ---------------------------------------------------------

def guarded(n, dtype, fill=None):
    """n words and a 64-word tail, all sentinel (NaN for floats); ``fill`` then presets the n words"""
    if dtype == torch.float32:
        buf = torch.full((n + GUARD,), float("nan"), dtype=dtype, device=DEV)
    else:
        buf = torch.full((n + GUARD,), SENTINEL, dtype=dtype, device=DEV)
    if fill is not None:
        buf[:n] = fill
    return buf


def check_guard(what, buf, n):
    tail = host(buf[n:])
    assert tail.size == GUARD
    if tail.dtype == np.float32:
        assert np.isnan(tail).all(), f"{what}: a word behind the buffer was written"
        assert not np.isnan(host(buf[:n])).any(), f"{what}: a word of the buffer was not written"
    else:
        assert (tail == SENTINEL).all(), f"{what}: a word behind the buffer was written"
        assert not (host(buf[:n]) == SENTINEL).any(), f"{what}: a word of the buffer was not written"


def abi_cases():
    for C in (1, 3, 20, 64, 70):
        index, S = ref.geometry_index(C)
        yield f"geometry-{C}", index, S, C
    for C in (20, 32):
        index, S = ref.narrow_index("below")
        yield f"narrow-{C}", index, S, C


@pytest.mark.parametrize("name,index,S,C", list(abi_cases()), ids=[c[0] for c in abi_cases()])
def test_abi_reduce_writes_every_word_and_no_other(name, index, S, C):
    """wsis_segment_reduce_fwd / _bwd on buffers pre-filled with NaN / 0x5a5a5a5a and a 64-word guard tail, with the
    reference's own perm and offsets: out, argmax and dsrc are overwritten in [0, S C) / [0, N C) and equal the
    reference, the tails are untouched; dsrc of the max backward starts at zero, as the wrapper passes it"""
    n = native()
    lib = n.hip()
    N = len(index)
    src = ref.case_rows("int", 8000 + C, (N, C))
    dout = ref.case_rows("int", 8100 + C, (S, C))
    perm, offsets = ref.csr(index, S)
    src_t, dout_t, index_t = dev(src), dev(dout), dev(index)
    perm_t, off_t = dev(perm.astype(np.int32)), dev(offsets.astype(np.int32))
    for code, kind in ((0, "sum"), (1, "mean"), (2, "max")):
        want32, _, arg = expected_forward(src, index, S, kind)
        out = guarded(S * C, torch.float32)
        am = guarded(S * C, torch.int32)
        n.check(lib.wsis_segment_reduce_fwd(src_t.data_ptr(), perm_t.data_ptr(), off_t.data_ptr(), out.data_ptr(),
                                            am.data_ptr(), N, S, C, code, n.stream_ptr()), "fwd")
        check_guard(f"{name} {kind} out", out, S * C)
        assert_bits(f"{name} {kind} out", out[:S * C].view(S, C), want32)
        if kind == "max":
            check_guard(f"{name} argmax", am, S * C)
            assert_bits(f"{name} argmax", am[:S * C].view(S, C), np.where(arg == N, -1, arg).astype(np.int32))
        else:
            assert (host(am) == SENTINEL).all(), "argmax belongs to max alone"
        dsrc = guarded(N * C, torch.float32, fill=0.0 if kind == "max" else None)
        n.check(lib.wsis_segment_reduce_bwd(dout_t.data_ptr(), index_t.data_ptr(), off_t.data_ptr(),
                                            am.data_ptr() if kind == "max" else None, dsrc.data_ptr(), N, S, C, code,
                                            n.stream_ptr()), "bwd")
        check_guard(f"{name} {kind} dsrc", dsrc, N * C)
        assert_bits(f"{name} {kind} dsrc", dsrc[:N * C].view(N, C), expected_backward(dout, index, S, kind, arg))


def csr_tables(layout):
    """index vectors (int64 arrays) and their S for the batched build.  'gaps': eight tables with an empty one first, in
    the middle and last, one with S = 0, and S from 2 to 20000; 'full': eight tables with rows, so the last one carries
    table number 7 (key bits 32 .. 34 all set).  Segments of one row, of 2 .. 64 rows (ranked in registers by the
    counting form), of 65 .. 2048 (its network in LDS) and of 3000 (its network in memory)."""
    rng = np.random.default_rng(31)
    wide = rng.integers(0, 20000, 30000)
    wide[0] = 19999
    mid = rng.integers(0, 20, 4000)                              # ~200 rows per segment
    one = np.concatenate([np.ones(3000, np.int64), np.zeros(3, np.int64)])
    rng.shuffle(one)
    small = rng.integers(0, 64, 50)
    small[3] = 63
    none = np.zeros(0, np.int64)
    if layout == "gaps":
        return [(none, 5), (wide, 20000), (mid, 20), (none, 3), (none, 0), (one, 2), (small, 64), (none, 7)]
    return [(small, 64), (wide, 20000), (mid, 20), (one, 2), (np.arange(299, -1, -1), 300), (np.zeros(1, np.int64), 1),
            (rng.integers(0, 255, 700), 255), (rng.integers(1, 9, 100), 9)]


@pytest.mark.parametrize("counting", ["0", "1"])
@pytest.mark.parametrize("layout", ["gaps", "full"])
def test_batched_csr_build_equals_the_reference(monkeypatch, layout, counting):
    """wsis_segment_csr_batch (the sort, and the counting form under WSIS_CSR_COUNTING=1) straight through the C ABI:
    perm and offsets of all eight tables equal segment_ref.csr, every word of both is written (an empty table's
    offsets, the single offset of a table with S = 0) and the guard tails are untouched; then the same through
    torch_scatter.segment_csr_batch"""
    monkeypatch.setenv("WSIS_CSR_COUNTING", counting)
    n = native()
    lib = n.hip()
    tables = csr_tables(layout)
    assert len(tables) == 8
    idx = [dev(np.asarray(i, np.int64)) for i, _ in tables]
    Ns, Ss = [len(i) for i, _ in tables], [S for _, S in tables]
    perm = guarded(sum(Ns), torch.int32)
    off = guarded(sum(Ss) + 8, torch.int32)
    ws_bytes = lib.wsis_segment_csr_batch_workspace_bytes(sum(Ns))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    n.check(lib.wsis_segment_csr_batch(8, (ctypes.c_void_p * 8)(*[t.data_ptr() if t.numel() else None for t in idx]),
                                       (ctypes.c_int64 * 8)(*Ns), (ctypes.c_int64 * 8)(*Ss), perm.data_ptr(),
                                       off.data_ptr(), ws.data_ptr(), ws_bytes, n.stream_ptr()), "csr_batch")
    check_guard("perm", perm, sum(Ns))
    check_guard("offsets", off, sum(Ss) + 8)
    want = [ref.csr(i, S) for i, S in tables]
    assert_bits("perm", perm[:sum(Ns)], np.concatenate([p for p, _ in want]).astype(np.int32))
    assert_bits("offsets", off[:sum(Ss) + 8], np.concatenate([o for _, o in want]).astype(np.int32))
    got = ts().segment_csr_batch([(t, S) for t, S in zip(idx, Ss)])
    for c, (p, o), N, S in zip(got, want, Ns, Ss):
        assert (c.N, c.S) == (N, S)
        assert_bits("offsets", c.offsets, o.astype(np.int32))
        assert_bits("perm", c.perm[:N], p.astype(np.int32))


def test_nine_tables_are_refused():
    pair = (torch.zeros(3, dtype=torch.int64, device=DEV), 1)
    with pytest.raises(AssertionError):
        ts().segment_csr_batch([pair] * 9)
    assert len(ts().segment_csr_batch([pair] * 8)) == 8


def single_csr_cases():
    rng = np.random.default_rng(41)
    for S in (1, 2, 3, 4, 255, 256, 257):                        # S + 1 = 2, 4, 256: a power of two exactly
        index = rng.integers(0, S, 3 * S + 5)
        index[1] = S - 1
        yield f"S={S}", index, S, torch.int64, S
    yield "N=1", np.array([3]), 6, torch.int64, 6
    yield "N=1 S=1", np.array([0]), 1, torch.int64, 1
    yield "descending", np.arange(499, -1, -1), 500, torch.int64, 500
    yield "one segment", np.full(700, 4), 5, torch.int64, 5
    yield "empty ends", rng.integers(3, 6, 50), 9, torch.int64, 9
    yield "int32", rng.integers(0, 40, 300), 40, torch.int32, 40
    yield "dim_size=None", np.concatenate([rng.integers(0, 31, 200), [30]]), 31, torch.int64, None


@pytest.mark.parametrize("name,index,S,dtype,dim_size", list(single_csr_cases()), ids=[c[0] for c in single_csr_cases()])
def test_single_csr_build_equals_the_reference(name, index, S, dtype, dim_size):
    """SegmentCSR against segment_ref.csr, and wsis_segment_csr on guarded buffers: all of perm [N] and offsets [S + 1]
    written, nothing behind them"""
    n = native()
    lib = n.hip()
    perm, offsets = ref.csr(index, S)
    c = ts().SegmentCSR(dev(index).to(dtype), dim_size)
    assert (c.N, c.S) == (len(index), S) and c.index.dtype == torch.int64
    assert_bits("offsets", c.offsets, offsets.astype(np.int32))
    assert_bits("perm", c.perm[:c.N], perm.astype(np.int32))
    N = len(index)
    p, o = guarded(N, torch.int32), guarded(S + 1, torch.int32)
    ws_bytes = lib.wsis_segment_csr_workspace_bytes(N, S)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    index_t = dev(np.asarray(index, np.int64))
    n.check(lib.wsis_segment_csr(index_t.data_ptr(), N, S, p.data_ptr(), o.data_ptr(), ws.data_ptr(),
                                 ws_bytes, n.stream_ptr()), "csr")
    torch.cuda.synchronize()
    check_guard("perm", p, N)
    check_guard("offsets", o, S + 1)
    assert_bits("perm", p[:N], perm.astype(np.int32))
    assert_bits("offsets", o[:S + 1], offsets.astype(np.int32))


def test_csr_without_rows():
    """N = 0: offsets [S + 1] all zero (S = 5, and S = 0: one word), nothing behind them"""
    n = native()
    lib = n.hip()
    for S in (5, 0):
        o = guarded(S + 1, torch.int32)
        ws = torch.empty(256, dtype=torch.uint8, device=DEV)
        n.check(lib.wsis_segment_csr(None, 0, S, None, o.data_ptr(), ws.data_ptr(), 256, n.stream_ptr()), "csr")
        check_guard("offsets", o, S + 1)
        assert_bits("offsets", o[:S + 1], np.zeros(S + 1, np.int32))
        c = ts().SegmentCSR(torch.zeros(0, dtype=torch.int64, device=DEV), S if S else None)
        assert (c.N, c.S) == (0, S)
        assert_bits("offsets", c.offsets, np.zeros(S + 1, np.int32))


# ---- row gather -----------------------------------------------------------------------------------------------------------

def gather_case(C, data="int"):
    """50 source rows; 900 picks that never name rows 0, 7 and 49 and name row 13 six hundred times"""
    rng = np.random.default_rng(50 + C)
    M = 50
    pool = np.setdiff1d(np.arange(M), [0, 7, 13, 49])
    idx = np.concatenate([rng.choice(pool, 300), np.full(600, 13)])
    rng.shuffle(idx)
    return ref.case_rows(data, 5100 + C, (M, C)), idx.astype(np.int64), M


def check_gather(what, src, idx, idx_dtype, src_t=None, dout_wrap=dev):
    import wsis_ops
    M, C = src.shape
    dout = ref.case_rows("int", 5200 + C, (len(idx), C))
    x = (dev(src) if src_t is None else src_t).detach().requires_grad_(True)
    out = wsis_ops.gather_rows(x, dev(idx).to(idx_dtype))
    assert_bits(f"{what} forward", out, src[idx])
    out.backward(dout_wrap(dout))
    want = ref.reduce(dout, idx, M, "sum")[0].astype(np.float32)
    assert_bits(f"{what} backward", x.grad, want)
    unused = np.setdiff1d(np.arange(M), idx)
    assert_bits(f"{what} unused rows", x.grad[dev(unused)], np.zeros((len(unused), C), np.float32))
    return out.detach(), x.grad


@pytest.mark.parametrize("idx_dtype", [torch.int32, torch.int64], ids=["int32", "int64"])
@pytest.mark.parametrize("C", [1, 3, 4, 6, 20, 32, 130])
def test_gather_rows_both_forms_both_index_types(C, idx_dtype):
    """float4 form (C % 4 == 0) and scalar form with int32 and int64 indexes: the forward is src[idx] bit for bit (wide
    data too), the backward the exact segmented sum of integer gradients -- 600 rows into row 13, exactly 0 for the rows
    that idx never names; and N = 1"""
    src, idx, M = gather_case(C)
    check_gather(f"C={C}", src, idx, idx_dtype)
    wide = gather_case(C, "wide")[0]
    check_gather(f"C={C} wide", wide, idx, idx_dtype)
    check_gather(f"C={C} N=1", src, idx[:1], idx_dtype)


@pytest.mark.parametrize("idx_dtype", [torch.int32, torch.int64], ids=["int32", "int64"])
@pytest.mark.parametrize("C", [20, 32])
def test_gather_rows_misaligned_views(C, idx_dtype):
    """src (and the incoming gradient) 4 bytes past a 16-byte boundary with C % 4 == 0: wsis_gather_rows must take the
    scalar form, its backward the wave kernel -- same bits as from aligned clones"""
    src, idx, M = gather_case(C, "wide")
    aligned = check_gather(f"C={C} aligned", src, idx, idx_dtype)
    got = check_gather(f"C={C} misaligned", src, idx, idx_dtype, src_t=misaligned(src), dout_wrap=misaligned)
    assert torch.equal(got[0], aligned[0]) and torch.equal(got[1], aligned[1])
    # and a misaligned destination, straight through the C ABI
    n = native()
    out = guarded(len(idx) * C + 1, torch.float32)
    idx_t, src_t = dev(idx).to(idx_dtype), dev(src)
    n.check(n.hip().wsis_gather_rows(src_t.data_ptr(), idx_t.data_ptr(), int(idx_dtype == torch.int64),
                                     out.data_ptr() + 4, len(idx), C, n.stream_ptr()), "gather_rows")
    assert np.isnan(host(out[:1])).all() and np.isnan(host(out[1 + len(idx) * C:])).all()
    assert_bits("misaligned out", out[1:1 + len(idx) * C].view(len(idx), C), src[idx])
