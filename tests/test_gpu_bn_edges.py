"""GPU: the fp32 BatchNorm(+ReLU) kernels of csrc/bn.hip against the fp64 reference of tests/bn_ref.py on every launch branch,
with inputs where var = E[x^2] - mean^2 cancels (|mean| up to 1000 sigma), a pivot up to 8 sigma off the mean, degenerate
channels and gradient rows of scales 1e-3 .. 1e3 (generators and their ReLU margin: tests/bn_ref.py, checked by
tests/test_bn_ref_host.py).

Measured on an MI355X, all 83 cases passing (kernel error | fp32-torch error | bound applied, each at the element closest to
its bound; last column: cases inside the project bound alone):
                                          var                      y                        dx                       dgamma
  stand-alone offset(100)                 1.6e-07|2.4e-06|2.9e-04  4.2e-06|2.3e-05|9.0e-05  1.3e-06|4.0e-06|1.0e-03  9.1e-05|3.3e-04|7.2e-03   2/2
  stand-alone offset(300)                 1.1e-07|7.9e-06|1.5e-04  2.2e-05|2.2e-05|8.7e-05  2.6e-06|4.7e-06|7.7e-04  6.5e-04|   -   |1.6e-02  34/34
  stand-alone offset(1000)                7.4e-07|8.0e-06|7.2e-05  7.1e-05|7.1e-05|2.8e-04  1.5e-04|1.5e-04|6.1e-04  1.2e-04|1.2e-04|4.9e-04  46/68
  stand-alone offset(1000), scaled dy     2.0e-07|1.9e-05|4.0e-04  4.0e-05|1.5e-04|6.2e-04  1.5e-03|1.5e-02|5.2e-01  8.0e-01|3.1e+00|1.4e+01   2/2
  stand-alone displaced_pivot(1)          3.7e-07|8.2e-07|4.0e-04  1.8e-06|1.7e-05|6.8e-05  7.3e-07|1.2e-06|1.1e-03  6.7e-05|1.3e-04|1.0e-02   2/2
  stand-alone displaced_pivot(4)          2.2e-06|9.7e-07|1.8e-04  3.9e-06|8.7e-06|6.9e-05  3.7e-06|1.6e-06|4.5e-03  4.3e-05|9.1e-05|7.7e-03   2/2
  stand-alone displaced_pivot(8)          1.8e-05|5.6e-07|3.4e-04  2.3e-05|1.2e-05|8.1e-04  1.3e-05|2.4e-06|3.9e-03  2.0e-04|9.1e-04|2.1e-02   2/2
  stand-alone displaced_pivot(8), scaled  1.8e-05|5.6e-07|3.4e-04  2.3e-05|1.2e-05|8.1e-04  7.2e-03|1.5e-03|1.8e+00  1.2e-02|1.4e-02|2.4e+00   2/2
  stand-alone degenerate                  7.5e-04|7.1e-03|2.4e+00  4.9e-06|7.0e-05|3.0e-04  5.1e-05|5.1e-05|1.9e-01  9.2e-05|1.9e-03|9.1e-03   2/2
  stand-alone degenerate, scaled dy       7.5e-04|7.1e-03|2.4e+00  4.9e-06|7.0e-05|3.0e-04  2.0e-02|2.0e-02|1.2e+02  3.4e-02|5.8e-01|2.3e+00   2/2
  centred offset(100)                     2.9e-07|9.7e-07|1.3e-04  5.7e-06|9.1e-06|4.7e-05  1.2e-06|6.7e-06|8.7e-04  3.1e-06|2.8e-04|7.1e-03   2/2
  centred offset(300)                     1.6e-06|1.6e-05|2.5e-04  2.3e-05|2.2e-05|8.7e-05  2.7e-06|3.9e-06|8.1e-04  1.8e-06|2.6e-04|9.5e-03   2/2
  centred offset(1000)                    3.8e-05|7.6e-05|3.7e-04  8.7e-05|6.3e-05|2.5e-04  1.5e-05|5.6e-05|4.8e-04  6.1e-06|5.4e-03|2.1e-02  10/18
  centred offset(1000), scaled dy         6.6e-06|2.4e-05|1.9e-04  5.6e-05|8.7e-05|3.5e-04  3.4e-03|1.0e-02|2.3e+00  4.5e-04|3.9e-01|1.8e+00   2/2
  centred displaced_pivot(1)              1.7e-07|2.7e-07|1.5e-04  1.5e-06|4.2e-06|5.2e-05  1.1e-06|3.2e-06|1.1e-03  2.0e-06|5.5e-05|5.6e-03   2/2
  centred displaced_pivot(4)              4.6e-07|9.2e-07|1.5e-04  2.0e-06|2.1e-05|8.6e-05  1.2e-06|2.1e-06|1.0e-03  2.0e-06|1.3e-04|5.9e-03   2/2
  centred displaced_pivot(8)              3.8e-07|1.3e-06|8.1e-05  2.2e-06|3.8e-06|1.3e-04  8.5e-07|1.9e-06|1.0e-03  2.9e-06|1.6e-04|5.6e-03   2/2
  centred displaced_pivot(8), scaled dy   3.8e-07|1.3e-06|8.1e-05  2.2e-06|3.8e-06|1.3e-04  3.5e-04|8.0e-04|1.7e+00  8.5e-04|2.7e-01|4.3e+00   2/2
  centred degenerate                      2.7e-03|1.3e-02|1.1e+01  5.8e-06|3.7e-05|2.9e-04  6.2e-05|6.2e-05|2.0e-01  1.8e-06|2.2e-04|6.8e-03   2/2
  centred degenerate, scaled dy           2.7e-03|1.3e-02|1.1e+01  5.8e-06|3.7e-05|2.9e-04  3.2e-02|3.2e-02|1.1e+02  2.3e-04|2.9e-01|1.5e+00   2/2
The largest |mean| / sigma at which the kernels sit inside the project bound alone is 300 (every case); at 1000 the fp32
rounding of the mean itself (half an ulp of 1000 sigma = 3e-5 .. 6e-5 sigma) reaches y, as it does in fp32 torch, and 22 of 68
stand-alone and 8 of 18 centred cases need the 4 x fp32-torch bound.  A pivot 8 sigma off costs the stand-alone variance a
factor ~50 (3.7e-7 -> 1.8e-5), still a fifth of the project bound.  The finish kernels were within 0.5 ulp of the exact
result for mean, var, both running statistics, dgamma and dbeta in every case: correctly rounded.

Branches -> cases (the id of a parametrised case names its branch).
  stand-alone path (wsis_ops.batch_norm_relu; wsis_bn_stats / wsis_bn_apply / wsis_bn_bwd directly for one row, without
  affine parameters and with an addend)
    test_rows_around_the_one_launch_kernels[M]  M = 1, 2 (the n > 1 guard, n / (n - 1)), 7 (short pivot), 8, 9, 1023, 1024,
                                    1025 (the 1024-thread walk), 4095, 4096 (last one-launch size), 4097 (two launches)
    test_channel_layouts[C-M]       M = 4101 (two launches; no multiple of any bn_rows_per_wg), and 333 (one launch) for
                                    the scalar layouts:
                                    C = 4 (one group, 2,048 rows per workgroup), 32, 96 / 160 (10 / 6 row lanes, 16 idle
                                    threads), 260 (65 groups, 3 lanes, 61 idle), 516 (one lane, rl = 1 idle), 1024, and
                                    1, 3, 5, 21, 33, 70 (masked tail channels, scalar loads).  4101 x 1024 is 16 MB: the
                                    smallest input that reaches that layout, everything else stays below 8 MB
    test_more_than_1024_channels_are_refused    C = 1028: WSIS_ERR_ARG, outputs untouched
    test_block_counts_of_the_final_kernels[nblk]  17, 64, 65, 129 partial rows for the 64 lanes (C = 32)
    test_modes[M-C]                 relu x training / evaluation x affine / NULL gamma and beta x addend / NULL
    test_generators_standalone[...] offset 100 / 300 / 1000 (channels at 0 and 30 in each), displaced pivot 1 / 4 / 8
                                    sigma, degenerate; scaled dy on the extreme of each
    test_isolation_standalone[...]  one +inf / one NaN: every other channel bit for bit
  centred-partials path (wsis_bn_stats_finalize, wsis_bn_stats_finalize_apply, wsis_bn_bwd_from_partials)
    test_chunk_edges[n_part]        n_part = 1, 2, 127 (G = 1), 128, 129, 191 (G = 2, uneven last chunk), 192 (G = 3), 4095
                                    (G = 63), 4096 (64 reached), 4097 (held), C = 32, 33, 96, 4; M % 32 = 0, 1, 31 each at
                                    n_part = 1, 2, 128, one of them elsewhere; with the sync block (ticket) and without
                                    (second launch), WSIS_BN_SMALL_FUSED = 0 and WSIS_BN_SMALL_G = 1 against the default: bit
                                    for bit; the sync slots zero afterwards
    test_generators_centred[...]    the generators of the stand-alone path, G = 1 (C = 33) and G = 2 (C = 32)
    test_isolation_centred[...]

Bounds.  Against bn_ref (the true fp64 values): the project bound of tests/test_gpu_ops.py::test_fused_batchnorm_relu --
forward and running statistics rtol 1e-4, atol 1e-5 max(1, max |want|); gradients 1e-3 / 1e-4 -- or, where larger, 4 x the
error that torch.nn.functional.batch_norm (+ relu) in fp32 on the GPU with autograd makes on the same input against fp64 (4:
a different but legitimate order of additions).  Every case prints kernel error | fp32-torch error | applied bound.
Before any gradient is compared the forward error must be below half the ReLU margin (5e-4): no mask can have flipped.
Against bn_ref.finish_from_partials / sum_partials (the finish kernels alone, exact on the fp32 partials they are given):
one ulp of fp32 at the wanted value, plus the fp64 arithmetic of the kernel itself: K x 2^-53 x (the size of the terms that
cancel), K = the number of fp64 roundings between a partial and the result (_roundings).  Derived, not measured; the
second term is below 0.01 ulp wherever the variance does not cancel to nothing (it matters for a constant channel, whose
exact result is ~1e-17 of mean^2).  Repeats, the launch forms among themselves, isolation, the zero variance of a constant
channel and dx = 0 under gamma = 0 are exact."""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bn_ref
import wsis_native as _n
import wsis_ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = bn_ref.EPS
MOM = float(np.float32(0.1))          # the momentum as the C ABI receives it
FWD = (1e-4, 1e-5)                    # rtol, atol x max(1, max |want|): tests/test_gpu_ops.py::test_fused_batchnorm_relu
GRAD = (1e-3, 1e-4)
HALF_MARGIN = 0.5 * bn_ref.MARGIN
ERR_ARG = -1                          # WSIS_ERR_ARG of include/wsis_hip.h


# ---------------------------------------------------------------- shared inputs and references (built once)

@functools.lru_cache(maxsize=None)
def _dy(M, C, scaled):
    if scaled:
        return bn_ref.dy_scaled(M, C, 17 * M + C)
    return torch.randn(M, C, generator=torch.Generator().manual_seed(31 * M + C))


@functools.lru_cache(maxsize=None)
def _addend(M, C):
    return torch.randn(M, C, generator=torch.Generator().manual_seed(5 * M + C + 1))


def _running0(c, training):
    """running statistics a case starts from: fixed values (training), the case's own (evaluation)"""
    if not training:
        return c.rm, c.rv
    return torch.full((c.C,), 0.25), torch.full((c.C,), 1.5)


@functools.lru_cache(maxsize=None)
def _reference(key, relu, training, scaled, addend):
    """fp64: everything the kernels produce for one case"""
    c = bn_ref.case(*key)
    dy = _dy(c.M, c.C, scaled)
    rm0, rv0 = _running0(c, training)
    mean, var, _ = bn_ref.stats(c.x)
    out = {}
    if training:
        out["mean"], out["var"] = mean, var
        out["running_mean"], out["running_var"] = bn_ref.running(rm0, rv0, c.x, MOM)
    else:
        mean, var = rm0.double(), rv0.double()
    out["y"] = bn_ref.forward(c.x, mean, var, c.gamma, c.beta, EPS, relu)
    out["dx"], out["dgamma"], out["dbeta"] = bn_ref.backward(
        c.x, dy, c.gamma, c.beta, EPS, relu, training, addend=_addend(c.M, c.C) if addend else None, mean=mean, var=var)
    return out


def _torch32(c, relu, training, scaled, addend):
    """the unfused formulation in fp32 on the GPU with autograd; None where torch refuses (one row in training mode)"""
    if training and c.M == 1:
        return None
    x = c.x.to(DEV).requires_grad_(True)
    g = None if c.gamma is None else c.gamma.to(DEV).requires_grad_(True)
    b = None if c.beta is None else c.beta.to(DEV).requires_grad_(True)
    rm, rv = (t.clone().to(DEV) for t in _running0(c, training))
    y = F.batch_norm(x, rm, rv, g, b, training, MOM, EPS)
    if relu:
        y = torch.relu(y)
    y.backward(_dy(c.M, c.C, scaled).to(DEV))
    out = {"y": y.detach(), "dx": x.grad + (_addend(c.M, c.C).to(DEV) if addend else 0)}
    if training:
        out.update(mean=x.detach().mean(0), var=x.detach().var(0, unbiased=False), running_mean=rm, running_var=rv)
    if g is not None:
        out.update(dgamma=g.grad, dbeta=b.grad)
    return out


# ---------------------------------------------------------------- the kernels

def _dev(t):
    return None if t is None else t.to(DEV).contiguous()


def _native(c, relu, training, scaled=False, addend=False, x=None):
    """wsis_bn_stats + wsis_bn_apply + wsis_bn_bwd"""
    lib, st = _n.hip(), _n.stream_ptr()
    M, C = c.M, c.C
    x = _dev(c.x) if x is None else x
    g, b, dy = _dev(c.gamma), _dev(c.beta), _dev(_dy(M, C, scaled))
    add = _dev(_addend(M, C)) if addend else None
    rm0, rv0 = _running0(c, training)
    wsb = lib.wsis_bn_workspace_bytes(M, C)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    out = {}
    if training:
        mean, var = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
        rm, rv = _dev(rm0.clone()), _dev(rv0.clone())
        _n.check(lib.wsis_bn_stats(_n.ptr(x), M, C, _n.ptr(mean), _n.ptr(var), _n.ptr(rm), _n.ptr(rv), MOM, _n.ptr(ws),
                                   wsb, st), "bn_stats")
        out.update(mean=mean, var=var, running_mean=rm, running_var=rv)
    else:
        mean, var = _dev(rm0), _dev(rv0)
    y, dx = torch.empty_like(x), torch.empty_like(x)
    dg, db = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    _n.check(lib.wsis_bn_apply(_n.ptr(x), _n.ptr(mean), _n.ptr(var), _n.ptr(g), _n.ptr(b), EPS, int(relu), _n.ptr(y), M, C,
                               st), "bn_apply")
    _n.check(lib.wsis_bn_bwd(_n.ptr(x), _n.ptr(dy), _n.ptr(mean), _n.ptr(var), _n.ptr(g), _n.ptr(b), EPS, int(relu),
                             int(training), _n.ptr(dx), _n.ptr(dg), _n.ptr(db), _n.ptr(add), M, C, _n.ptr(ws), wsb, st),
             "bn_bwd")
    torch.cuda.synchronize()
    out.update(y=y, dx=dx, dgamma=dg, dbeta=db)
    return out


def _module(c, relu, training, scaled=False):
    """wsis_ops.batch_norm_relu on an nn.BatchNorm1d; mean / var of a training pass from a wsis_bn_stats call of their own"""
    M, C = c.M, c.C
    bn = torch.nn.BatchNorm1d(C, eps=EPS, momentum=MOM)
    rm0, rv0 = _running0(c, training)
    with torch.no_grad():
        bn.weight.copy_(c.gamma)
        bn.bias.copy_(c.beta)
        bn.running_mean.copy_(rm0)
        bn.running_var.copy_(rv0)
    bn = bn.to(DEV).train(training)
    x = _dev(c.x).requires_grad_(True)
    y = wsis_ops.batch_norm_relu(x, bn, relu=relu)
    y.backward(_dev(_dy(M, C, scaled)))
    out = {"y": y.detach(), "dx": x.grad, "dgamma": bn.weight.grad, "dbeta": bn.bias.grad}
    if training:
        lib = _n.hip()
        wsb = lib.wsis_bn_workspace_bytes(M, C)
        ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
        mean, var = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
        _n.check(lib.wsis_bn_stats(_n.ptr(x.detach()), M, C, _n.ptr(mean), _n.ptr(var), None, None, MOM, _n.ptr(ws), wsb,
                                   _n.stream_ptr()), "bn_stats")
        out.update(mean=mean, var=var, running_mean=bn.running_mean.detach(), running_var=bn.running_var.detach())
    torch.cuda.synchronize()
    return out


# ---------------------------------------------------------------- comparisons

ORDER = ("mean", "var", "running_mean", "running_var", "y", "dx", "dgamma", "dbeta")


def _compare(what, got, want, t32):
    """every tensor of ``got`` against fp64 under the project bound, or 4 x the fp32-torch error where that is larger;
    the forward error is asserted below half the ReLU margin before any gradient is looked at.  Prints one line."""
    parts, failed, alone = [], [], True
    for name in ORDER:
        if name not in got:
            continue
        g, w = got[name].detach().double().cpu(), want[name]
        assert g.shape == w.shape and bool(torch.isfinite(g).all()), (what, name)
        rtol, atol = FWD if name in ORDER[:5] else GRAD
        err = (g - w).abs()
        project = rtol * w.abs() + atol * max(1.0, float(w.abs().max()))
        bound, terr = project, float("nan")
        if t32 is not None and name in t32:
            terr = float((t32[name].detach().double().cpu() - w).abs().max())
            bound = torch.clamp_min(project, 4.0 * terr)
        worst = int(torch.argmax(err / bound))
        alone &= bool((err <= project).all())
        parts.append(f"{name} {float(err.max()):.2e}|{terr:.2e}|{float(bound.flatten()[worst]):.2e}")
        if name == "y":
            assert float(err.max()) < HALF_MARGIN, (what, "forward error above half the ReLU margin", float(err.max()))
        if not bool((err <= bound).all()):
            failed.append((name, float(err.flatten()[worst]), float(bound.flatten()[worst])))
    print(f"[bn-edges] {what}: " + "  ".join(parts) + f"  project-bound-alone={'yes' if alone else 'no'}")
    assert not failed, (what, failed)
    return alone


def _same(a, b, what, skip=None):
    """two result dicts bit for bit (NaN equal to NaN); ``skip``: a channel left out"""
    assert a.keys() == b.keys(), what
    for name in a:
        u, v = a[name], b[name]
        if skip is not None:
            keep = torch.arange(u.shape[-1], device=u.device) != skip
            u, v = u[..., keep], v[..., keep]
        assert torch.equal(u.view(torch.int32), v.view(torch.int32)), (what, name)


def _standalone(key, relu=True, training=True, scaled=False, addend=False, native=None, bound32=True):
    c = bn_ref.case(*key)
    if native is None:
        native = c.M == 1 or c.gamma is None or addend
    run = (lambda: _native(c, relu, training, scaled, addend)) if native else (lambda: _module(c, relu, training, scaled))
    got = run()
    what = (f"{key[0]}({key[3]}) {c.M}x{c.C} {'native' if native else 'module'} relu={int(relu)} train={int(training)}"
            f"{'' if c.gamma is not None else ' no-affine'}{' addend' if addend else ''}{' dy-scaled' if scaled else ''}")
    alone = _compare(what, got, _reference(key, relu, training, scaled, addend),
                     _torch32(c, relu, training, scaled, addend) if bound32 else None)
    _same(got, run(), what + ": repeat")
    return c, got, alone


# ---------------------------------------------------------------- stand-alone path

@pytest.mark.parametrize("M", bn_ref.ROWS)
def test_rows_around_the_one_launch_kernels(M):
    """|mean| up to 1000 sigma at every row count around the 1024-thread walk and the 4,096-row switch; one and two rows:
    the running variance keeps v for n = 1 and takes n / (n - 1) = 2 for n = 2 (bn_ref.running)"""
    for relu in (True, False):
        _standalone(("offset", M, 32, 1000, True, False), relu=relu)
    if M > 1:                                      # (one row runs through the direct calls anyway)
        _standalone(("offset", M, 32, 1000, True, False), native=True)
    _standalone(("offset", M, 32, 1000, True, True), training=False)


@pytest.mark.parametrize("C,M", bn_ref.layout_shapes())
def test_channel_layouts(C, M):
    _standalone(("offset", M, C, 1000, True, False))


def test_more_than_1024_channels_are_refused():
    lib, st = _n.hip(), _n.stream_ptr()
    M, C = 10, 1028
    x, dy = torch.randn(M, C, device=DEV), torch.randn(M, C, device=DEV)
    wsb = lib.wsis_bn_workspace_bytes(M, C)
    assert wsb > 0
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    outs = [torch.full((C,), 7.0, device=DEV) for _ in range(6)] + [torch.full((M, C), 7.0, device=DEV)]
    mean, var, rm, rv, dg, db, dx = outs
    assert lib.wsis_bn_stats(_n.ptr(x), M, C, _n.ptr(mean), _n.ptr(var), _n.ptr(rm), _n.ptr(rv), MOM, _n.ptr(ws), wsb,
                             st) == ERR_ARG
    assert b"1024" in lib.wsis_last_error()
    assert lib.wsis_bn_bwd(_n.ptr(x), _n.ptr(dy), _n.ptr(mean), _n.ptr(var), None, None, EPS, 1, 1, _n.ptr(dx), _n.ptr(dg),
                           _n.ptr(db), None, M, C, _n.ptr(ws), wsb, st) == ERR_ARG
    torch.cuda.synchronize()
    for t in outs:
        assert bool((t == 7.0).all())


@pytest.mark.parametrize("nblk", sorted(bn_ref.NBLK_M))
def test_block_counts_of_the_final_kernels(nblk):
    M = bn_ref.NBLK_M[nblk]
    assert -(-M // 256) == nblk
    _standalone(("offset", M, 32, 1000, True, False))


@pytest.mark.parametrize("M,C", bn_ref.MODE_SHAPES)
def test_modes(M, C):
    for affine in (True, False):
        for training in (True, False):
            for relu in (True, False):
                for addend in (False, True):
                    _standalone(("offset", M, C, 300, affine, not training), relu=relu, training=training, addend=addend,
                                native=True)


def _generator_keys(shapes):
    keys = []
    for M, C in shapes:
        keys += [("offset", M, C, r, True, False) for r in bn_ref.RATIOS]
        keys += [("displaced_pivot", M, C, d, True, False) for d in bn_ref.DISPLACEMENTS]
        keys += [("degenerate", M, C, None, True, False)]
    return keys


def _extreme(key):
    return key[3] in (None, 1000, 8)


def _id(key):
    return f"{key[0]}{'' if key[3] is None else key[3]}-{key[1]}x{key[2]}"


def _check_degenerate(c, got, standalone, addend=False):
    for ch, kind in enumerate(c.kinds):
        if kind == "const_short" and standalone and "var" in got:
            assert float(got["var"][ch]) == 0.0 and float(got["mean"][ch]) == float(c.x[0, ch])
        if kind in ("gamma0", "gamma0_beta0"):      # dx = 0 exactly (+ the addend as it is)
            rest = _dev(_addend(c.M, c.C))[:, ch] if addend else torch.zeros(c.M, device=DEV)
            assert torch.equal(got["dx"][:, ch], rest), kind
        if kind == "gamma0_beta0":
            assert not bool(got["y"][:, ch].any()) and float(got["dgamma"][ch]) == 0.0 and float(got["dbeta"][ch]) == 0.0


@pytest.mark.parametrize("key", _generator_keys(bn_ref.GEN_SHAPES), ids=_id)
def test_generators_standalone(key):
    """every input class with plain dy, the extreme of each class with scaled dy as well; the line of a case ends in
    project-bound-alone=yes/no"""
    for scaled in (False, True)[:1 + _extreme(key)]:
        c, got, _ = _standalone(key, scaled=scaled, native=scaled)
        if key[0] == "degenerate":
            _check_degenerate(c, got, True)


def _poisoned(c, value):
    """device x with ``value`` at one element of channel 1 (row 9: behind the pivot rows), and that channel"""
    x = c.x.clone()
    x[9, 1] = value
    return _dev(x), 1


@pytest.mark.parametrize("value", [float("inf"), float("nan")], ids=["inf", "nan"])
@pytest.mark.parametrize("M,C", bn_ref.ISOLATION_SHAPES)
def test_isolation_standalone(M, C, value):
    c = bn_ref.case("offset", M, C, 30, True, False)
    clean = _native(c, True, True)
    x, ch = _poisoned(c, value)
    dirty = _native(c, True, True, x=x)
    _same(clean, dirty, "isolation", skip=ch)
    assert not bool(torch.isfinite(dirty["var"][ch]))


# ---------------------------------------------------------------- centred-partials path

def _roundings(n_part):
    """fp64 roundings between a partial and the result: the lane walk of a chunk, its 8 lane sums, the walk and the lane
    sums (or the 6 butterfly steps) over the chunks, and the finish (S / n, n mu, mu, W -, Q +, / n)"""
    G = max(1, min(64, n_part // 64))
    per = -(-n_part // G)
    return -(-per // 8) + 8 + -(-G // 8) + 8 + 6


def _centred_forward(c, part, sync, apply, relu=True):
    lib, st = _n.hip(), _n.stream_ptr()
    M, C = c.M, c.C
    n_part = part.shape[0]
    x, g, b = _dev(c.x), _dev(c.gamma), _dev(c.beta)
    wsb = lib.wsis_bn_stats_finalize_workspace_bytes(n_part, C)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    mean, var = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    rm0, rv0 = _running0(c, True)
    rm, rv = _dev(rm0.clone()), _dev(rv0.clone())
    y = torch.empty_like(x)
    sp = _n.ptr(_n.sync_block()) if sync else None
    if apply:
        _n.check(lib.wsis_bn_stats_finalize_apply(_n.ptr(part), n_part, M, C, _n.ptr(mean), _n.ptr(var), _n.ptr(rm),
                                                  _n.ptr(rv), MOM, _n.ptr(x), _n.ptr(g), _n.ptr(b), EPS, int(relu),
                                                  _n.ptr(y), _n.ptr(ws), wsb, sp, st), "finalize_apply")
    else:
        _n.check(lib.wsis_bn_stats_finalize(_n.ptr(part), n_part, M, C, _n.ptr(mean), _n.ptr(var), _n.ptr(rm), _n.ptr(rv),
                                            MOM, _n.ptr(ws), wsb, sp, st), "finalize")
        _n.check(lib.wsis_bn_apply(_n.ptr(x), _n.ptr(mean), _n.ptr(var), _n.ptr(g), _n.ptr(b), EPS, int(relu), _n.ptr(y),
                                   M, C, st), "bn_apply")
    torch.cuda.synchronize()
    if sync:
        assert not bool(_n.sync_block()[:64 * 4096].any()), "a launch left its sync slot dirty"
        assert _n.sync_errors() == []
    return dict(mean=mean, var=var, running_mean=rm, running_var=rv, y=y)


def _centred_backward(c, bpart, stats, sync, scaled, addend, relu=True):
    lib, st = _n.hip(), _n.stream_ptr()
    M, C = c.M, c.C
    n_part = bpart.shape[0]
    x, g, b, dy = _dev(c.x), _dev(c.gamma), _dev(c.beta), _dev(_dy(M, C, scaled))
    add = _dev(_addend(M, C)) if addend else None
    wsb = lib.wsis_bn_stats_finalize_workspace_bytes(n_part, C)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    dx = torch.empty_like(x)
    dg, db = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    sp = _n.ptr(_n.sync_block()) if sync else None
    _n.check(lib.wsis_bn_bwd_from_partials(_n.ptr(bpart), n_part, _n.ptr(x), _n.ptr(dy), _n.ptr(stats["mean"]),
                                           _n.ptr(stats["var"]), _n.ptr(g), _n.ptr(b), EPS, int(relu), _n.ptr(dx),
                                           _n.ptr(dg), _n.ptr(db), _n.ptr(add), M, C, _n.ptr(ws), wsb, sp, st),
             "bn_bwd_from_partials")
    torch.cuda.synchronize()
    if sync:
        assert not bool(_n.sync_block()[:64 * 4096].any()), "a launch left its sync slot dirty"
        assert _n.sync_errors() == []
    return dict(dx=dx, dgamma=dg, dbeta=db)


def _within_one_ulp(what, got, want, fp64_term):
    got, want = got.detach().double().cpu(), want.double()
    err = (got - want).abs()
    bound = bn_ref.ulp32(want) + fp64_term
    worst = int(torch.argmax(err / bound))
    print(f"[bn-edges] {what}: finish err {float(err[worst]):.3e} = {float(err[worst] / bn_ref.ulp32(want)[worst]):.2f} ulp, "
          f"fp64 term {float(fp64_term[worst]):.1e}")
    assert bool((err <= bound).all()), (what, worst, float(err[worst]), float(bound[worst]))


def _centred(key, monkeypatch, scaled=False, addend=True, forms=True, finite=True):
    """forward and backward finish of one case in every launch form; returns (case, results of the default form)"""
    c = bn_ref.case(*key)
    M, C = c.M, c.C
    n_part = (M + 31) // 32
    what = f"centred {key[0]}({key[3]}) {M}x{C} n_part={n_part}{' dy-scaled' if scaled else ''}"
    mean64, var64, _ = bn_ref.stats(c.x)
    part_h = bn_ref.slice_partials(c.x)
    bpart_h = bn_ref.bwd_slice_partials(c.x, _dy(M, C, scaled), mean64, var64, c.gamma, c.beta, EPS, True)
    part, bpart = _dev(part_h), _dev(bpart_h)

    def run(sync=True, apply=True):
        f = _centred_forward(c, part, sync, apply)
        f.update(_centred_backward(c, bpart, f, sync, scaled, addend))
        return f

    got = run()
    _same(got, run(), what + ": repeat")
    if forms:
        _same(got, run(apply=False), what + ": finalize + apply")
        _same(got, run(sync=False), what + ": without a sync block (second launch)")
        _same(got, run(sync=False, apply=False), what + ": finalize without a sync block")
        monkeypatch.setenv("WSIS_BN_SMALL_FUSED", "0")
        _same(got, run(), what + ": WSIS_BN_SMALL_FUSED=0")
        monkeypatch.delenv("WSIS_BN_SMALL_FUSED")
        monkeypatch.setenv("WSIS_BN_SMALL_G", "1")
        _same(got, run(), what + ": WSIS_BN_SMALL_G=1")
        monkeypatch.delenv("WSIS_BN_SMALL_G")
    # the finish kernels alone: exact results on the partials they were given
    k = _roundings(n_part) * 2.0 ** -53
    mu, var, unb, mass = bn_ref.finish_from_partials(part_h, M)
    s_abs = part_h[:, 0].double().abs().sum(0) / M
    rm0, rv0 = (t.double() for t in _running0(c, True))
    _within_one_ulp(what + " mean", got["mean"], mu, k * s_abs)
    _within_one_ulp(what + " var", got["var"], var, k * mass)
    _within_one_ulp(what + " running_mean", got["running_mean"], (1.0 - MOM) * rm0 + MOM * mu, k * (s_abs + rm0.abs()))
    _within_one_ulp(what + " running_var", got["running_var"], (1.0 - MOM) * rv0 + MOM * unb,
                    k * (mass * (M / max(M - 1, 1)) + rv0.abs()))
    a, b, a_abs, b_abs = bn_ref.sum_partials(bpart_h)
    _within_one_ulp(what + " dbeta", got["dbeta"], a, k * a_abs)
    _within_one_ulp(what + " dgamma", got["dgamma"], b, k * b_abs)
    # and the true values
    _compare(what, got, _reference(key, True, True, scaled, addend), _torch32(c, True, True, scaled, addend))
    return c, got


def _edge_id(n_part):
    return f"n_part{n_part}-G{max(1, min(64, n_part // 64))}"


@pytest.mark.parametrize("n_part", sorted(bn_ref.CENTRED_EDGES), ids=_edge_id)
def test_chunk_edges(n_part, monkeypatch):
    C, rems = bn_ref.CENTRED_EDGES[n_part]
    assert _n.hip().wsis_bn_stats_finalize_workspace_bytes(n_part, C) == max(1, min(64, n_part // 64)) * 3 * C * 8 + 256
    for rem in rems:
        M = bn_ref.centred_rows(n_part, rem)
        assert (M + 31) // 32 == n_part and M % 32 == rem
        _centred(("offset", M, C, 1000, True, False), monkeypatch)


@pytest.mark.parametrize("key", _generator_keys(bn_ref.CENTRED_GEN_SHAPES), ids=_id)
def test_generators_centred(key, monkeypatch):
    for scaled in (False, True)[:1 + _extreme(key)]:
        c, got = _centred(key, monkeypatch, scaled=scaled, addend=not scaled, forms=False)
        if key[0] == "degenerate":
            _check_degenerate(c, got, False, addend=not scaled)


@pytest.mark.parametrize("value", [float("inf"), float("nan")], ids=["inf", "nan"])
@pytest.mark.parametrize("M,C", bn_ref.ISOLATION_SHAPES)
def test_isolation_centred(M, C, value):
    """the partials of the poisoned channel are what a convolution epilogue would write there: not finite"""
    c = bn_ref.case("offset", M, C, 30, True, False)
    mean64, var64, _ = bn_ref.stats(c.x)
    part = _dev(bn_ref.slice_partials(c.x))
    bpart = _dev(bn_ref.bwd_slice_partials(c.x, _dy(M, C, False), mean64, var64, c.gamma, c.beta, EPS, True))

    def run(part, bpart, x):
        cc = bn_ref.Case(x, c.gamma, c.beta)
        f = _centred_forward(cc, part, True, True)
        f.update(_centred_backward(cc, bpart, f, True, False, True))
        return f

    clean = run(part, bpart, c.x)
    x = c.x.clone()
    x[9, 1] = value
    part2, bpart2 = part.clone(), bpart.clone()
    part2[0, :, 1] = value if math.isnan(value) else torch.tensor([value, float("nan")], device=DEV)
    bpart2[0, :, 1] = float("nan")
    dirty = run(part2, bpart2, x)
    _same(clean, dirty, "isolation", skip=1)
    assert not bool(torch.isfinite(dirty["var"][1]))
