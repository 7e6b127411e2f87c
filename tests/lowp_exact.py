"""Exact-arithmetic oracle of the 16-bit sparse convolutions (csrc/spconv_lp.hip) for the GPU tests.

Every operand is an integer times a power of two (its grain), and every output element keeps sum |x||w| (+ |bias|)
below 2^24 units of the output grain (the product of the operand grains).  Then each partial sum of the kernels' fp32
accumulation is exact, whatever the order of additions or the MFMA blocking, and the right answer is unique:

  forward / dIn   round-to-nearest-even of the fp64 reference, fp64 -> fp32 (exact) -> bf16 / fp16
  dW              the fp64 reference cast to fp32 (exact)

so the tests compare with torch.equal on all elements, with no tolerance.  The references are the fp64 gather-GEMMs of
tests/conv_ref.py over pair lists.  Each helper asserts its own precondition (the 2^24 bound, element by element) and
that the case is not vacuous: enough outputs needed rounding, some were exact ties (only ties separate round-to-nearest-
even from round-half-away), and, with a bias, some outputs come out differently when the bias is rounded to 16 bits
before the add."""
import ctypes

import torch

import conv_ref
import wsis_native

LIMIT = 2.0 ** 24
BITS = {torch.bfloat16: 8, torch.float16: 11}          # significand bits, the implicit one included
EMIN = {torch.bfloat16: -126, torch.float16: -14}      # exponent of the smallest normal


PLAN_KEYS = ("nt", "ncg", "fwd_blocks", "chunks", "rows_per_chunk", "nw", "groups", "lds")


def lp_plan(M_out, K, Cin, Cout):
    """wsis_spconv_lp_plan as a dict: the launch branch a product of this shape runs (host-only query)"""
    out = (ctypes.c_int32 * len(PLAN_KEYS))()
    wsis_native.check(wsis_native.hip().wsis_spconv_lp_plan(M_out, K, Cin, Cout, out), "spconv_lp_plan")
    return dict(zip(PLAN_KEYS, out))


def ints(shape, R, exp, gen, dev="cuda"):
    """fp32 tensor of integers uniform in [-R, R] times 2^exp"""
    return torch.randint(-R, R + 1, shape, generator=gen, device=dev).float() * 2.0 ** exp


def rounding(want, dt):
    """(inexact, tie) masks of the fp64 values ``want`` rounded to ``dt`` (normal and subnormal range)"""
    v = want.abs()
    _, e = torch.frexp(v)                               # v = m 2^e, m in [0.5, 1)
    ulp = torch.pow(2.0, (torch.clamp(e - 1, min=EMIN[dt]) - (BITS[dt] - 1)).double())
    r = torch.fmod(v, ulp)
    return r != 0, r == ulp / 2


def _round(want, grain, absref, dt, min_round, min_ties, what):
    """the RNE 16-bit form of ``want`` (fp64), after the precondition and non-vacuity checks"""
    units = absref / grain
    assert float(units.max()) < LIMIT, f"{what}: sum |x||w| reaches {float(units.max()):.0f} >= 2^24 grains"
    q = want / grain
    assert torch.equal(q, torch.round(q)), f"{what}: an output is off the grain"
    f = want.float()
    assert torch.equal(f.double(), want), f"{what}: an output is not exact in fp32"
    inexact, tie = rounding(want, dt)
    n = want.numel()
    frac = float(inexact.sum()) / max(n, 1)
    assert frac >= min_round, f"{what}: only {frac:.3f} of the outputs needed rounding (< {min_round})"
    assert int(tie.sum()) >= min_ties, f"{what}: {int(tie.sum())} ties (< {min_ties})"
    return f.to(dt)


def expect_rows(X, W, pairs, M_out, dt, grain, bias=None, min_round=0.1, min_ties=1, what=""):
    """[M_out, Cout] 16-bit result of sum_k X[pi] @ W[k] scattered to po (+ fp32 bias, added before the one rounding).
    X 16-bit (or fp32 holding 16-bit values), W [K, Cin, Cout], pairs on the device."""
    sel = torch.arange(M_out, device=X.device)
    want = conv_ref.rows(X, W, pairs, M_out, sel)
    absref = conv_ref.rows(X.abs(), W.abs(), pairs, M_out, sel)
    if bias is not None:
        b = bias.double()
        want = want + b
        absref = absref + b.abs()
    exp = _round(want, grain, absref, dt, min_round, min_ties, what)
    if bias is not None:
        b16 = bias.to(dt).double()
        assert bool((b16 != bias.double()).any()), f"{what}: every bias value is exact in 16 bits"
        early = (want - bias.double() + b16).float().to(dt)
        assert not torch.equal(early, exp), f"{what}: a bias rounded to 16 bits before the add would pass"
    return exp


def expect_dw(X, dY, pairs, grain, what=""):
    """fp32 [K, Cin, Cout] dW[k] = X[pi]^T @ dY[po], exact"""
    want = conv_ref.dw(X, dY, pairs)
    absref = conv_ref.dw(X.abs(), dY.abs(), pairs)
    units = absref / grain
    assert float(units.max()) < LIMIT, f"{what}: sum |x||dy| reaches {float(units.max()):.0f} >= 2^24 grains"
    f = want.float()
    assert torch.equal(f.double(), want), f"{what}: dW is not exact in fp32"
    assert bool((want != 0).any()), f"{what}: dW is zero everywhere"
    return f
