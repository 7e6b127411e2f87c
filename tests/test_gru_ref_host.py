"""GRUCellEx and the recurrence around it on the CPU: the fp64 restatement of tests/gru_ref.py against torch autograd over
``GRUCellEx.forward_reference`` and against ``RNNGraphConvModule`` in float64, and the conditioning check that justifies
the bounds of tests/test_gpu_gru_edges.py: on every row count and every hard case of that file, ``forward_reference`` with
autograd in fp32 on the CPU must stay below a quarter of the bounds against the fp64 restatement.

Conditioning figures (error / bound, the bounds = FWD / GRAD of tests/test_gpu_lstm_cell.py; fp32 torch on the CPU against
the fp64 restatement; forward | gradients):

    row counts 1 .. 2049, ordinary rows     0.019 | 0.0049    (hy at S = 2048; weight_hh at S = 1536)
    hard rows, all 27 rows                  0.0099 | 0.0062   (hy of x0 / h0 / x0h0 / tiny; ig.weight of big_h)
    hard rows, the 4 hard rows alone        0.0049 | 0.0016   (hy of h0 and sat_bias; dh of big_h)

so the reference arithmetic alone sits 50 x inside either bound, everything finite.  The fp64 reference without the last
row's upstream gradient stands 39.7 bounds out at the least (ig.bias at S = 2048; 300 and more up to S = 97)."""
import copy

import numpy as np
import pytest
import torch

import graphnet
from tests import gru_ref
from tests.test_gpu_lstm_cell import FWD, GRAD, ratio, rec_graph  # noqa: F401  (rec_graph: the 54-node graph, a fixture)

PER_ROW = ("hy", "dx", "dh")


def _close(a, b, rel, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape and np.isfinite(a).all(), what
    err, scale = float(np.abs(a - b).max()), float(np.abs(b).max())
    assert err <= rel * max(scale, 1e-300), (what, err, scale)


def autograd(cell, x, h, g, dtype):
    """{hy, dx, dh, <parameter name>: gradient} of forward_reference under torch autograd in ``dtype`` on the CPU"""
    cell = copy.deepcopy(cell).to(dtype)
    xr, hr = (t.detach().to(dtype).requires_grad_(True) for t in (x, h))
    hy = cell.forward_reference(xr, hr)
    hy.backward(g.to(dtype))
    out = {"hy": hy.detach().numpy(), "dx": xr.grad.numpy(), "dh": hr.grad.numpy()}
    out.update({n: p.grad.numpy() for n, p in cell.named_parameters()})
    return out


def restated(cell, x, h, dhy, dhy2=None):
    P = gru_ref.params_of(cell)
    hy, k = gru_ref.cell_fwd(P, x.numpy(), h.numpy())
    out = gru_ref.cell_bwd(P, k, None if dhy is None else dhy.numpy(), None if dhy2 is None else dhy2.numpy())
    out["hy"] = hy
    return out, k


@pytest.mark.parametrize("up", ["dhy", "dhy2", "both"])
@pytest.mark.parametrize("kind", ["ordinary"] + gru_ref.HARD_KINDS)
def test_fp64_restatement_equals_autograd_over_forward_reference(kind, up):
    if kind == "ordinary":
        cell = gru_ref.make_cell(3)
        x, h, dhy = gru_ref.make_rows(5, 9, 3)
    else:
        cell, x, h, dhy = gru_ref.hard_case(kind)
    x, h, dhy = x.double(), h.double(), dhy.double()
    dhy2 = torch.randn(x.shape, generator=torch.Generator().manual_seed(6), dtype=torch.float64)
    cell = cell.double()
    a, b = (dhy if up != "dhy2" else None), (dhy2 if up != "dhy" else None)
    got, k = restated(cell, x, h, a, b)
    assert set(got) == {"hy", "dx", "dh", *gru_ref.NAMES} == {"hy", "dx", "dh", *gru_ref.params_of(cell)}
    assert {"pre_gi", "pre_gh", "si", "sh", "gin", "xin", "r", "z", "n"} <= set(k)
    if kind != "ordinary":
        gru_ref.check_hardness(kind, k)
    want = autograd(cell, x, h, sum(t for t in (a, b) if t is not None), torch.float64)
    for name in want:
        _close(got[name], want[name], 1e-12, (kind, up, name))


@pytest.mark.parametrize("cat_all", [True, False])
@pytest.mark.parametrize("R", [0, 1, 3, 7])
def test_fp64_recurrence_equals_the_module_in_float64(rec_graph, R, cat_all):
    G = rec_graph
    assert G["roles"]["isolated"] and G["roles"]["no_in"] and max(G["roles"]["in_hub"].values()) == 33
    torch.manual_seed(40 + R)
    fnet = graphnet.create_fnet([13, 32, 128, 64, 32 * 32], True, True, -1)
    mod = graphnet.RNNGraphConvModule(gru_ref.make_cell(41), fnet, 32, vv=False, nrepeats=R, cat_all=cat_all).double()
    ref = copy.deepcopy(mod)
    mod.set_info(graphnet.GraphConvInfo(torch.from_numpy(np.stack([G["src"], G["tgt"]])), G["feats"].double(), G["S"]))
    x = G["x"].double().requires_grad_(True)
    out = mod(x)
    gout = torch.randn(out.shape, generator=torch.Generator().manual_seed(7), dtype=torch.float64)
    out.backward(gout)
    W = ref._fnet(G["feats"].double()).view(-1, 32, 32)
    want, gr = gru_ref.recurrence(gru_ref.params_of(ref._cell), G["x"].numpy(), W.detach().numpy(), G["src"], G["tgt"], R,
                                  cat_all, gout.numpy())
    assert want.shape == (54, 32 * (R + 1) if cat_all else 32)
    W.backward(torch.from_numpy(gr["dW"]))
    _close(want, out.detach().numpy(), 1e-12, "out")
    _close(gr["dhx"], x.grad.numpy(), 1e-11, "dhx")
    if R == 0:
        assert all(p.grad is None for p in mod.parameters()) and float(np.abs(gr["dW"]).max()) == 0.0
        return
    for n, p in mod._cell.named_parameters():
        _close(gr[n], p.grad.numpy(), 1e-11, n)
    for (n, p), (_, q) in zip(mod._fnet.named_parameters(), ref._fnet.named_parameters()):
        _close(q.grad.numpy(), p.grad.numpy(), 1e-11, "fnet." + n)


# ---------------------------------------------------------------- fp32 on the CPU inside a quarter of the bounds
def _figures(got, want, rows=None):
    rep = {}
    for name, w in want.items():
        tol = FWD if name == "hy" else GRAD
        rep[name] = ratio(got[name], w, tol)
        if rows is not None and name in PER_ROW:
            rep[name + "@hard"] = ratio(got[name][rows], w[rows], tol)
    return rep


def _assert_quarter(rep, what):
    print(what, {k: "%.2g" % v for k, v in rep.items()})
    bad = {k: v for k, v in rep.items() if not v <= 0.25}
    assert not bad, (what, bad)


@pytest.mark.parametrize("S", list(gru_ref.ROW_COUNTS))
def test_fp32_reference_sits_inside_a_quarter_of_the_bounds_at_every_row_count(S):
    cell = gru_ref.make_cell(S)
    x, h, dhy = gru_ref.make_rows(S + 1, S, 3)
    want, _ = restated(cell, x, h, dhy)
    _assert_quarter(_figures(autograd(cell, x, h, dhy, torch.float32), want), f"fp32 / bound, S={S}")
    # the bound bites at this row count: the reference without the last row's upstream gradient stands at least two
    # bounds away on every parameter gradient (the device test asks a result inside one bound to see it)
    drop_dhy = dhy.clone()
    drop_dhy[-1] = 0
    drop, _ = restated(cell, x, h, drop_dhy)
    out = {n: ratio(drop[n], want[n], GRAD) for n in gru_ref.NAMES}
    print(f"dropped row / bound, S={S}", {k: "%.3g" % v for k, v in out.items()})
    assert min(out.values()) > 2.0, out


@pytest.mark.parametrize("kind", gru_ref.HARD_KINDS)
def test_fp32_reference_sits_inside_a_quarter_of_the_bounds_on_hard_rows(kind):
    cell, x, h, dhy = gru_ref.hard_case(kind)
    want, k = restated(cell, x, h, dhy)
    gru_ref.check_hardness(kind, k)
    _assert_quarter(_figures(autograd(cell, x, h, dhy, torch.float32), want, gru_ref.HARD_ROWS), f"fp32 / bound, {kind}")


def test_the_restated_launch_plan():
    """the plan every device case is named for (tests/test_gpu_gru_edges.py asserts the slab counts against the C ABI)"""
    for S, n in gru_ref.ROW_COUNTS.items():
        assert gru_ref.slabs(S) == n, S
    assert [gru_ref.idle_bwd_waves(S) for S in (1, 2, 3, 4, 5, 13)] == [3, 2, 1, 0, 0, 0]
    assert gru_ref.bwd_rows_per_wave(13) == [[2, 2, 2, 2], [2, 1, 1, 1]]
    assert gru_ref.idle_bwd_waves(13, 1) == 3 and gru_ref.slabs(13, 1) == 4          # WSIS_GRU_ROWS=1
    assert [gru_ref.fwd_workgroups(S) for S in (7, 8, 9, 2048, 2049)] == [1, 1, 2, 256, 256]
    assert gru_ref.reduce_plan(7) == [(0, 1)] * 7 + [(0, 0)]
    assert gru_ref.reduce_plan(8) == [(0, 1)] * 8 and gru_ref.reduce_plan(9) == [(0, 2)] + [(0, 1)] * 7
    assert gru_ref.reduce_plan(124) == [(1, 0)] * 4 + [(0, 15)] * 4
    assert gru_ref.reduce_plan(128) == [(1, 0)] * 8
    assert gru_ref.reduce_plan(129) == [(1, 1)] + [(1, 0)] * 7
    assert gru_ref.reduce_plan(171)[0] == (1, 6)
