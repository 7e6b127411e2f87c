"""Host: the fp64 BatchNorm reference of tests/bn_ref.py against torch.nn.BatchNorm1d in float64 with autograd, the
exact finish of the centred slice partials against the direct statistics, and every input generator against the condition
it states -- for every parameter set tests/test_gpu_bn_edges.py runs.  No GPU."""
import copy

import numpy as np
import pytest
import torch

import bn_ref

RTOL = 1e-12


def _close(got, want, what):
    got, want = bn_ref.f64(got), bn_ref.f64(want)
    scale = max(1.0, float(want.abs().max())) if want.numel() else 1.0
    err = float((got - want).abs().max()) if want.numel() else 0.0
    assert torch.allclose(got, want, rtol=RTOL, atol=RTOL * scale), (what, err)


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("M,C", [(2, 5), (77, 33), (1025, 8)])
def test_reference_equals_torch_batchnorm_in_fp64(M, C, affine, relu, training):
    g = torch.Generator().manual_seed(M + C)
    x = (torch.randn(M, C, generator=g) * 2 + 0.5).float()
    dy = torch.randn(M, C, generator=g).float()
    addend = torch.randn(M, C, generator=g).float()
    bn = torch.nn.BatchNorm1d(C, eps=bn_ref.EPS, momentum=0.1, affine=affine).double()
    with torch.no_grad():
        if affine:
            bn.weight.copy_(torch.rand(C, generator=g) + 0.5)
            bn.bias.copy_(torch.randn(C, generator=g) * 0.3)
        bn.running_mean.copy_(torch.randn(C, generator=g) * 0.1 + 0.5)
        bn.running_var.copy_(torch.rand(C, generator=g) * 4 + 2)
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    bn.train(training)
    xr = x.double().requires_grad_(True)
    y = bn(xr)
    if relu:
        y = torch.relu(y)
    y.backward(dy.double())
    gamma, beta = (bn.weight.detach(), bn.bias.detach()) if affine else (None, None)
    mean, var, unb = bn_ref.stats(x)
    _close(mean, x.double().mean(0), "mean")
    _close(var, x.double().var(0, unbiased=False), "var")
    _close(unb, x.double().var(0, unbiased=True), "unbiased var")
    if training:
        rm, rv = bn_ref.running(rm0, rv0, x, 0.1)
        _close(rm, bn.running_mean, "running mean")
        _close(rv, bn.running_var, "running var")
    else:
        mean, var = rm0, rv0
    _close(bn_ref.forward(x, mean, var, gamma, beta, bn_ref.EPS, relu), y, "y")
    dx, dgamma, dbeta = bn_ref.backward(x, dy, gamma, beta, bn_ref.EPS, relu, training, mean=mean, var=var)
    _close(dx, xr.grad, "dx")
    if affine:
        _close(dgamma, bn.weight.grad, "dgamma")
        _close(dbeta, bn.bias.grad, "dbeta")
    dx2 = bn_ref.backward(x, dy, gamma, beta, bn_ref.EPS, relu, training, addend=addend, mean=mean, var=var)[0]
    _close(dx2, xr.grad + addend.double(), "dx + addend")


def test_one_row_has_zero_variance_and_keeps_it_unbiased():
    x = torch.tensor([[3.0, -1.5]])
    mean, var, unb = bn_ref.stats(x)
    assert torch.equal(mean, x[0].double()) and not var.any() and not unb.any()
    dx = bn_ref.backward(x, torch.ones(1, 2), None, None, bn_ref.EPS, False, True)[0]
    assert not dx.any()


@pytest.mark.parametrize("M,C,ratio", [(1, 4, 30), (31, 5, 1000), (32, 4, 1000), (33, 4, 0), (4799, 8, 1000), (6111, 3, 300)])
def test_finish_of_the_slice_partials_equals_the_direct_statistics(M, C, ratio):
    """finish_from_partials is exact on the fp32 partials, so it differs from stats(x) by the rounding of the partials
    alone: S_i by e_i, Q_i by f_i with |e_i| <= ulp(S_i) / 2, |f_i| <= ulp(Q_i) / 2 move
      mean by sum e_i / M
      var  by (sum f_i + 2 sum e_i (S_i / n_i - mean) + sum e_i^2 / n_i - M dmean^2) / M,   M dmean^2 <= sum e_i^2 / n_i"""
    x = bn_ref.offset(M, C, ratio, seed=M + C).x
    part = bn_ref.slice_partials(x)
    assert part.dtype == torch.float32 and part.shape == ((M + 31) // 32, 2, C)
    mean, var, unb, mass = bn_ref.finish_from_partials(part, M)
    want_mean, want_var, want_unb = bn_ref.stats(x)
    n_i = torch.tensor([min(32, M - 32 * i) for i in range(part.shape[0])], dtype=torch.float64).unsqueeze(1)
    e, f = 0.5 * bn_ref.ulp32(part[:, 0]), 0.5 * bn_ref.ulp32(part[:, 1])
    slice_dev = (part[:, 0].double() / n_i - want_mean).abs()
    b_mean = e.sum(0) / M
    b_var = (f.sum(0) + 2 * (e * slice_dev).sum(0) + 2 * (e * e / n_i).sum(0)) / M
    fp64 = 64 * 2.0 ** -53 * (mass + want_mean.abs())              # the reference's own fp64 arithmetic (pairwise sums)
    print(f"[bn-ref] M={M} C={C} ratio={ratio}: mean err {float((mean - want_mean).abs().max()):.3e} bound "
          f"{float(b_mean.max()):.3e}, var err {float((var - want_var).abs().max()):.3e} bound {float(b_var.max()):.3e}")
    assert bool(((mean - want_mean).abs() <= b_mean + fp64).all())
    assert bool(((var - want_var).abs() <= b_var + fp64).all())
    assert bool(((unb - want_unb).abs() <= (b_var + fp64) * (M / max(M - 1, 1))).all())
    assert bool((mass >= var).all())


def test_backward_slice_partials_add_up_to_the_gradients():
    M, C = 1025, 7
    c = bn_ref.offset(M, C, 30, seed=3)
    dy = bn_ref.dy_scaled(M, C, 4)
    mean, var, _ = bn_ref.stats(c.x)
    part = bn_ref.bwd_slice_partials(c.x, dy, mean, var, c.gamma, c.beta, c.eps, True)
    assert part.dtype == torch.float32 and part.shape == (33, 2, C)
    _, dgamma, dbeta = bn_ref.backward(c.x, dy, c.gamma, c.beta, c.eps, True, True)
    a, b, abs_a, abs_b = bn_ref.sum_partials(part)
    assert bool(((a - dbeta).abs() <= 33 * 2.0 ** -24 * abs_a.clamp_min(1e-30)).all())
    assert bool(((b - dgamma).abs() <= 33 * 2.0 ** -24 * abs_b.clamp_min(1e-30)).all())


def test_ulp32():
    t = torch.tensor([1.0, 1.5, 2.0, 1000.0, 0.0, -3.0], dtype=torch.float64)
    want = [float(np.spacing(np.float32(abs(v)))) for v in t.tolist()]
    want[4] = 2.0 ** -149
    assert bn_ref.ulp32(t).tolist() == want


def _margin_holds(c, mean, var):
    z = bn_ref.pre_activation(c.x, mean, var, c.gamma, c.beta, c.eps)
    inside = (z.abs() < bn_ref.MARGIN) & (z != 0)
    assert not bool(inside.any()), int(inside.sum())
    zero = (z == 0)
    if bool(zero.any()):        # exactly 0 only where the construction makes it so: gamma = beta = 0, or one row and beta = 0
        by_construction = c.exact_zero.clone()
        if c.M == 1 and c.beta is not None and not hasattr(c, "rm"):
            by_construction |= (c.beta == 0)
        assert not bool(zero[:, ~by_construction].any())
    return z


@pytest.mark.parametrize("key", bn_ref.gpu_cases(), ids=lambda k: "-".join(str(v) for v in k))
def test_generator_meets_its_conditions(key):
    kind, M, C, p, affine, evaluation = key
    c = bn_ref.case(*key)
    assert c.x.dtype == torch.float32 and c.x.shape == (M, C) and bool(torch.isfinite(c.x).all())
    assert (c.gamma is None) == (not affine) and (c.beta is None) == (not affine)
    mean, var, _ = bn_ref.stats(c.x)
    z = _margin_holds(c, *((c.rm.double(), c.rv.double()) if evaluation else (mean, var)))
    sd = torch.sqrt(var)
    if kind != "degenerate" and M >= 2:
        got = mean.abs() / sd
        assert bool(((got - c.ratio).abs() <= 0.01 * c.ratio + 0.01).all()), (got, c.ratio)
        # both sides of the mask in every channel (two rows or more, affine or not)
        assert bool(((z > 0).any(0) & (z <= 0).any(0)).all())
        assert c.nudged <= 0.02 * M * C + 2
    if kind == "displaced_pivot":
        disp = (c.x[:8].double().mean(0) - mean).abs() / sd
        assert bool((disp <= p).all()) and bool((disp >= 0.99 * p).all()) and p <= bn_ref.PIVOT_LIMIT, disp
        assert bool((c.displacement <= p).all())
    if kind == "degenerate":
        k = c.kinds
        assert set(k) == set(bn_ref.KINDS)
        for ch, kind_c in enumerate(k):
            col = c.x[:, ch]
            if kind_c == "const_short":
                assert float(var[ch]) == 0.0 and (col.view(torch.int32)[0].item() & 0xFFFFF) == 0
            elif kind_c == "const_full":
                assert float(var[ch]) == 0.0 and (col.view(torch.int32)[0].item() & 1) == 1
            elif kind_c == "tiny_sigma":
                assert 0.25e-8 < float(var[ch]) < 4e-8 and abs(float(mean[ch]) - 1) < 1e-4
            elif kind_c == "spike":
                assert int((col != 0).sum()) == 1 and float(col.max()) == 1e4
            elif kind_c == "gamma0":
                assert float(c.gamma[ch]) == 0.0 and float(c.beta[ch]) != 0.0
            elif kind_c == "gamma0_beta0":
                assert float(c.gamma[ch]) == 0.0 and float(c.beta[ch]) == 0.0 and not bool(z[:, ch].any())
            elif kind_c == "beta_masks":
                share = float((z[:, ch] > 0).double().mean())
                assert 0.002 <= share <= 0.03, share
            else:
                assert bool((z[:, ch] > 0).any()) and bool((z[:, ch] <= 0).any())


def test_dy_scales_span_six_decades():
    dy = bn_ref.dy_scaled(1025, 33, 1)
    rms = dy.double().pow(2).mean(1).sqrt()
    assert dy.dtype == torch.float32 and float(rms.min()) < 3e-3 and float(rms.max()) > 3e2
    assert torch.equal(dy, bn_ref.dy_scaled(1025, 33, 1))
