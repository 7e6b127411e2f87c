"""Plain numpy fp64 reference of the segment family (csrc/segment.hip, gather_rows of csrc/core.hip) and the input
generators of tests/test_gpu_segment_edges.py.  It shares no code with the product: a stable argsort and a searchsorted
for the CSR, np.add.at / np.maximum.at for the reductions.  tests/test_segment_ref_host.py checks it against Python loops
and against oracle.scatter_ref.

Conventions (those of torch_scatter 2.0.x for a 1-D index over dim 0): an empty segment has value 0, and under max / min
``arg = N``; under max / min ``arg`` is the smallest original row that attains the extreme.  NaN inputs are outside the
contract."""
import numpy as np

U24 = 2.0 ** -24          # unit roundoff of fp32 (round to nearest)
KINDS = ("sum", "mean", "max", "min")


def _rows(src):
    src = np.asarray(src)
    width = int(np.prod(src.shape[1:], dtype=np.int64))          # (not -1: undefined for an array without rows)
    return src.reshape(src.shape[0], width).astype(np.float64), src.shape[1:]


def csr(index, S):
    """perm = stable argsort of index, offsets[s] = number of rows with an id below s (s = 0 .. S); ids lie in [0, S)"""
    index = np.asarray(index).astype(np.int64)
    assert index.ndim == 1 and (index.size == 0 or (index.min() >= 0 and index.max() < S))
    perm = np.argsort(index, kind="stable").astype(np.int64)
    offsets = np.searchsorted(index[perm], np.arange(S + 1), side="left").astype(np.int64)
    return perm, offsets


def counts(index, S):
    return np.bincount(np.asarray(index).astype(np.int64), minlength=S)[:S].astype(np.int64) if S else np.zeros(0, np.int64)


def reduce(src, index, S, kind):
    """fp64 values [S, ...]; for max / min also arg [S, ...] int64 (None otherwise)"""
    x, tail = _rows(src)
    index = np.asarray(index).astype(np.int64)
    N, C = x.shape
    assert index.shape == (N,) and kind in KINDS
    if kind in ("sum", "mean"):
        out = np.zeros((S, C))
        np.add.at(out, index, x)
        if kind == "mean":
            out = out / np.maximum(counts(index, S), 1)[:, None]
        return out.reshape((S,) + tail), None
    y = x if kind == "max" else -x
    best = np.full((S, C), -np.inf)
    np.maximum.at(best, index, y)
    # the smallest row that attains the extreme: its own number where a row attains it, N elsewhere, then the minimum
    arg = np.full((S, C), N, np.int64)
    rows = np.where(y == best[index], np.arange(N)[:, None], N)
    np.minimum.at(arg, index, rows)
    n = counts(index, S)
    out = np.where(n[:, None] > 0, best if kind == "max" else -best, 0.0) + 0.0          # (+ 0.0: no negative zero)
    return out.reshape((S,) + tail), arg.reshape((S,) + tail)


def reduce_bwd(dout, index, S, kind, arg=None):
    """fp64 gradient [N, ...] of ``reduce`` for the incoming gradient dout [S, ...]"""
    g, tail = _rows(dout)
    index = np.asarray(index).astype(np.int64)
    N, C = index.size, g.shape[1]
    assert g.shape[0] == S and kind in KINDS
    if kind == "sum":
        d = g[index] if N else np.zeros((0, C))
    elif kind == "mean":
        d = g[index] / np.maximum(counts(index, S), 1)[index][:, None] if N else np.zeros((0, C))
    else:
        a = np.asarray(arg).reshape(S, C)
        d = np.zeros((N, C))
        s_i, c_i = np.nonzero(a < N)
        d[a[s_i, c_i], c_i] = g[s_i, c_i]
    return d.reshape((N,) + tail)


def sum_bound(src, index, S, kind):
    """Per-element bound [S, ...] on |fp32 result - exact result| that holds for EVERY order of an fp32 summation of the
    n_s rows of a segment: n_s - 1 additions, each with a relative error of at most u = 2^-24, give
    |err| <= ((1 + u)^(n_s - 1) - 1) sum|x| <= n_s u sum|x| while n_s < 16384 (then (n_s - 1)(1 + n_s u) <= n_s); one
    more u sum|x| covers the fp64 reference's own rounding and, under mean, the second-order term of the quotient -- so
    (n_s + 1) u sum|x|.  Mean divides that by n_s (exact in fp32 below 2^24) and adds one rounding of the quotient,
    u |result|.  Derived, not measured."""
    x, tail = _rows(src)
    index = np.asarray(index).astype(np.int64)
    assert kind in ("sum", "mean")
    n = counts(index, S).astype(np.float64)[:, None]
    mag = np.zeros((S, x.shape[1]))
    np.add.at(mag, index, np.abs(x))
    b = (n + 1.0) * U24 * mag
    if kind == "mean":
        val, _ = reduce(src, index, S, "mean")
        b = b / np.maximum(n, 1.0) + U24 * np.abs(val.reshape(S, -1))
    return b.reshape((S,) + tail)


# ---- inputs of the device tests (also run on the host: test_segment_ref_host.py) ---------------------------------------

def int_rows(rng, shape):
    """integer-valued fp32 in [-8, 8]: a segment of fewer than 2^20 rows sums exactly in fp32 in any order"""
    return rng.integers(-8, 9, size=shape).astype(np.float32)


def wide_rows(rng, shape):
    """randn * 10^U(-3, 3): six decades of dynamic range"""
    return (rng.standard_normal(shape) * 10.0 ** rng.uniform(-3, 3, shape)).astype(np.float32)


def tie_rows(rng, shape):
    return rng.integers(-2, 3, size=shape).astype(np.float32)


def index_of_sizes(rng, sizes, lead=0, trail=0, shuffle=True):
    """an index vector whose segment ``lead + k`` has sizes[k] rows, with ``lead`` / ``trail`` empty segments around;
    returns (index int64 [N], S)"""
    sizes = np.asarray(sizes, np.int64)
    index = np.repeat(np.arange(len(sizes), dtype=np.int64) + lead, sizes)
    if shuffle:
        rng.shuffle(index)
    return index, lead + len(sizes) + trail


def cp_of(C):
    """channels per pass of segment_reduce_kernel (power of two, at most 64); 64 / CP row groups"""
    cp = 1
    while cp < C and cp < 64:
        cp <<= 1
    return cp


GEOMETRY_C = (1, 2, 3, 4, 7, 8, 12, 16, 20, 32, 33, 64, 65, 70, 128, 130)


def geometry_sizes(C):
    """segment sizes around the row-group count G and around the eight-rows-per-trip loop, which group 0 enters at
    7 G + 1 rows"""
    G = 64 // cp_of(C)
    return [0, 1, G - 1, G, G + 1, 7 * G, 7 * G + 1, 8 * G - 1, 8 * G, 8 * G + 1, 16 * G + 3]


def geometry_index(C):
    rng = np.random.default_rng(1000 + C)
    return index_of_sizes(rng, geometry_sizes(C), lead=2, trail=3)


NARROW_C = (20, 24, 28, 32)
NARROW_SIZES = (0, 1, 2, 3, 4, 5, 7, 8, 9, 11)


def narrow_index(pad_to):
    """the sizes of NARROW_SIZES (50 rows in 10 segments), then 20 one-row and 10 empty segments: S = 40, N = 70
    (``pad_to`` = 'below': N < 4 S).  'edge' grows the one-row segments until N = 4 S - 1 = 159, the last N of the narrow
    kernel; 'at' until N = 4 S = 160, the first N of the wave kernel.  Returns (index, S)"""
    rng = np.random.default_rng(77)
    S = 40
    N = {"below": 70, "edge": 4 * S - 1, "at": 4 * S}[pad_to]
    sizes = list(NARROW_SIZES) + [1] * 20 + [0] * 10
    extra = N - sum(sizes)
    k = len(NARROW_SIZES)
    while extra > 0:                                     # spread over the one-row segments: they stay small
        sizes[k] += 1
        k = k + 1 if k + 1 < len(NARROW_SIZES) + 20 else len(NARROW_SIZES)
        extra -= 1
    assert sum(sizes) == N and len(sizes) == S
    return index_of_sizes(rng, sizes)


def cap_case(which):
    """(index, S, C) past a grid cap of 256 * 16 blocks: 'wave' -- four segments per block, S > 16384; 'narrow' -- 32
    segments per block, S > 131072 and N < 4 S"""
    S, N, C = {"wave": (20000, 30000, 8), "narrow": (140000, 150000, 20)}[which]
    rng = np.random.default_rng(S)
    index = rng.integers(0, S, N)
    index[0], index[1] = S - 1, 0
    return index.astype(np.int64), S, C


def case_rows(kind, seed, shape):
    """'int' | 'wide' | 'tie' rows from a seed of their own, so host and device tests see the same numbers"""
    return {"int": int_rows, "wide": wide_rows, "tie": tie_rows}[kind](np.random.default_rng(seed), shape)


def fp32_reduceat(src, index, S, kind):
    """numpy's own fp32 segment sum / mean (np.add.reduceat over the rows in CSR order): an honest fp32 summation whose
    order is not the device's"""
    x = _rows(src)[0].astype(np.float32)
    perm, offsets = csr(index, S)
    n = np.diff(offsets)
    out = np.zeros((S, x.shape[1]), np.float32)
    if len(index):
        full = np.flatnonzero(n > 0)                       # (reduceat returns a row, not 0, for an empty slice)
        out[full] = np.add.reduceat(x[perm], offsets[full], axis=0, dtype=np.float32)
    if kind == "mean":
        out = out / np.maximum(n, 1).astype(np.float32)[:, None]
    return out.reshape((S,) + np.shape(src)[1:])
