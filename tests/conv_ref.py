"""fp64 references of the sparse convolutions for the GPU value tests: gather-GEMMs over ORACLE pair lists
(oracle/spconv_ref: subm_pairs_fast / down_pairs_fast / inverse_pairs, numpy, independent of csrc/rulebook.hip), computed
on the device in float64.  ``pairs`` is a list over kernel offsets k of (pi, po): input row pi[j] feeds output row po[j].

  forward   y[po] += X[pi] @ W[k]              rows(X, W, pairs, rows)
  dIn       dX[pi] += dY[po] @ W[k]^T          rows(dY, W^T, swap(pairs), rows)
  dW        dW[k] = X[pi]^T @ dY[po]           dw(X, dY, pairs), checked by check_dw

check_dw states its tolerance as a fraction of the reference's max-abs and proves the fraction tight: the same comparison
against the reference with ONE pair of one offset removed must fail (a kernel that drops a row cannot pass)."""
import numpy as np
import torch


def device_pairs(pairs, dev):
    return [(torch.as_tensor(np.asarray(pi), dtype=torch.long, device=dev),
             torch.as_tensor(np.asarray(po), dtype=torch.long, device=dev)) for pi, po in pairs]


def swap(pairs):
    """the pairs of the adjoint product (dIn of a convolution, or the inverse convolution of a strided one)"""
    return [(po, pi) for pi, po in pairs]


def dw(X, dY, pairs):
    """[K, Cin, Cout] float64"""
    Xd, Yd = X.double(), dY.double()
    out = torch.zeros(len(pairs), X.shape[1], dY.shape[1], dtype=torch.float64, device=X.device)
    for k, (pi, po) in enumerate(pairs):
        if len(pi):
            out[k] = Xd[pi].t() @ Yd[po]
    return out


def rows(X, W, pairs, M_out, sel):
    """float64 rows ``sel`` (distinct) of the [M_out, W.shape[2]] gather-GEMM  sum_k X[pi] @ W[k] scattered to po"""
    pos = torch.full((M_out,), -1, dtype=torch.long, device=X.device)
    pos[sel] = torch.arange(sel.numel(), device=X.device)
    out = torch.zeros(sel.numel(), W.shape[2], dtype=torch.float64, device=X.device)
    Xd, Wd = X.double(), W.double()
    for k, (pi, po) in enumerate(pairs):
        hit = pos[po] >= 0
        out.index_add_(0, pos[po[hit]], Xd[pi[hit]] @ Wd[k])
    return out


def check_dw(got, X, dY, pairs, frac, what, want=None):
    """assert |got - dW_fp64| <= frac * max|dW_fp64| over ALL offsets, and that the reference with one pair removed
    (the pair of median size in the offset with the fewest pairs) is more than that bound away.  Returns
    (error, bound, error of the one-pair-removed reference)."""
    if want is None:
        want = dw(X, dY, pairs)
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite dW (an unwritten slab or output element)"
    bound = frac * float(want.abs().max())
    diff = got.double() - want
    err = float(diff.abs().max())
    live = [k for k, (pi, _) in enumerate(pairs) if len(pi)]
    k = min(live, key=lambda j: len(pairs[j][0]))
    pi, po = pairs[k]
    size = X[pi].abs().amax(1).double() * dY[po].abs().amax(1).double()
    j = int(torch.argsort(size)[len(pi) // 2])
    dropped = diff[k] + torch.outer(X[pi[j]].double(), dY[po[j]].double())
    err_drop = max(err, float(dropped.abs().max()))
    assert err <= bound, f"{what}: dW max abs error {err:.3e} > {bound:.3e} ({frac:g} of max|dW|)"
    assert err_drop > bound, f"{what}: the bound {bound:.3e} would not see a dropped pair ({err_drop:.3e})"
    return err, bound, err_drop
