"""The fused LSTMCellEx kernels (csrc/lstm.hip) against the fp64 restatement of tests/lstm_ref.py: every row count at
which the launch plan changes, hard rows beside ordinary ones, the NULL upstream gradients, byte-equal parameter
gradients over two runs, the cell-state carrying recurrence on both of its paths, the reference's own model file
(tests/golden/lstm_golden.npz) on the device, and the dispatch between the fused kernel and the module walk.

Bounds (the issue's, = test_gru_cell_ex_fwd_bwd of tests/test_gpu_ops.py: the arithmetic has the same structure, K = 32
dots and one row norm): forward rtol 1e-4 / atol 1e-5, gradients rtol 1e-3 / atol 1e-4, atol scaled by max(1, max|ref|)
of the tensor as ``close`` of test_gpu_ops.py does.  They hold on the hard rows too: on those inputs
``forward_reference`` in fp32 on the CPU stays below a quarter of them against fp64 (DESIGN 4.5.1 has the figures), so
no wider bound is needed there."""
import copy

import numpy as np
import pytest
import torch

import graphnet
import wsis_native
import wsis_ops
from tests import graph_ref, lstm_ref
from tests.test_lstm_ref_host import check_golden, golden_network

pytestmark = pytest.mark.gpu
DEV = "cuda"
FWD, GRAD = (1e-4, 1e-5), (1e-3, 1e-4)

# the launch plan of csrc/lstm.hip
WF = 8                    # LSTM_WF: rows per weight staging (= per workgroup) of the forward
WG_ROWS = 4 * 3           # LSTM_WAVES * LSTM_ROWS: rows per workgroup (= per slab) of the backward
MAX_WG = 256              # LSTM_MAX_WG: beyond it the waves stride over the rows
P_FLOATS = 2 * 128 * 32 + 32 * 32 + 2 * 128 + 32      # LSTM_P: floats of a parameter-gradient slab
RED_LANES, RED_DEPTH = 8, 8                           # slab lanes of the reduce, slabs in flight per lane
S_REDUCE = WG_ROWS * (2 * RED_LANES * RED_DEPTH + 3) - 5      # 131 slabs: two batched rounds and a tail per slab lane
S_STRIDE = WG_ROWS * MAX_WG + WG_ROWS + 1                     # every wave of the backward walks a second row
ROW_COUNTS = [1, WF - 1, WF, WF + 1, WG_ROWS - 1, WG_ROWS, WG_ROWS + 1, S_REDUCE, S_STRIDE]


def ratio(got, want, tol):
    """max over the elements of error / (atol * max(1, max|want|) + rtol * |want|): <= 1 passes"""
    rtol, atol = tol
    a = got.detach().cpu().double().numpy() if torch.is_tensor(got) else np.asarray(got, dtype=np.float64)
    b = np.asarray(want, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.isfinite(a).all(), "non-finite values (an unwritten row or element)"
    if b.size == 0:
        return 0.0
    scale = max(1.0, float(np.abs(b).max()))
    return float((np.abs(a - b) / (atol * scale + rtol * np.abs(b))).max())


def make_cell(seed):
    torch.manual_seed(seed)
    return graphnet.LSTMCellEx(32, 32, bias=True, layernorm=True, ingate=True)


def make_rows(seed, S):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(S, 32, generator=g) for _ in range(5)]          # x, h, c, dhy, dcy


def run_cell(cell, x, h, c, dhy, dcy, dev=DEV, fn=None):
    """{hy, cy, dx, dh, dc, <parameter name>: gradient} of cell(x, (h, c)) on ``dev`` (fn: another forward)"""
    cell = copy.deepcopy(cell).to(dev)
    t = [v.clone().to(dev).requires_grad_(True) for v in (x, h, c)]
    hy, cy = cell(t[0], (t[1], t[2])) if fn is None else fn(cell, t[0], (t[1], t[2]))
    outs = [o for o, d in ((hy, dhy), (cy, dcy)) if d is not None]
    torch.autograd.backward(outs, [d.to(dev) for d in (dhy, dcy) if d is not None])
    out = {"hy": hy.detach(), "cy": cy.detach(), "dx": t[0].grad, "dh": t[1].grad, "dc": t[2].grad}
    out.update({n: p.grad for n, p in cell.named_parameters()})
    return out


def ref_cell(cell, x, h, c, dhy, dcy):
    P = lstm_ref.params_of(cell)
    hy, cy, k = lstm_ref.cell_fwd(P, x.numpy(), h.numpy(), c.numpy())
    out = lstm_ref.cell_bwd(P, k, None if dhy is None else dhy.numpy(), None if dcy is None else dcy.numpy())
    out.update(hy=hy, cy=cy)
    return out, k


def compare(got, want, what, rows=None):
    """every output and gradient within the bounds; ``rows``: additionally the per-row tensors on those rows alone
    (with the scale of those rows, so a hard row is not hidden behind the others).  Returns the figures."""
    rep = {}
    for name, w in want.items():
        tol = FWD if name in ("hy", "cy") else GRAD
        rep[name] = ratio(got[name], w, tol)
        if rows is not None and name in ("hy", "cy", "dx", "dh", "dc"):
            rep[name + "@hard"] = ratio(got[name][rows], w[rows], tol)
    print(what, {k: "%.2g" % v for k, v in rep.items()})
    bad = {k: v for k, v in rep.items() if not v <= 1.0}
    assert not bad, (what, bad)
    return rep


def test_the_named_constants_are_the_kernels():
    """the row counts below are named from lstm.hip's constants: the workspace of the C ABI shows the slab size, the rows
    per slab and the cap"""
    ws = wsis_native.hip().wsis_lstm_cell_workspace_bytes
    slab = 4 * P_FLOATS
    assert ws(1) == ws(WG_ROWS) == slab + 256 and ws(WG_ROWS + 1) == 2 * slab + 256
    assert ws(S_REDUCE) == 131 * slab + 256
    assert ws(WG_ROWS * MAX_WG) == ws(S_STRIDE) == MAX_WG * slab + 256


@pytest.mark.parametrize("S", ROW_COUNTS)
def test_fused_cell_fwd_bwd_at_every_row_count(S):
    cell = make_cell(S)
    x, h, c, dhy, dcy = make_rows(S + 1, S)
    want, _ = ref_cell(cell, x, h, c, dhy, dcy)
    compare(run_cell(cell, x, h, c, dhy, dcy), want, f"S={S}")


# ---------------------------------------------------------------- hard rows beside ordinary ones
HARD_ROWS = [0, 5, 13, 26]
HARD_S = 27


def hard_case(kind):
    """(cell, x, h, c, dhy, dcy) with the rows HARD_ROWS made hard in the way ``kind`` names"""
    cell = make_cell(77)
    x, h, c, dhy, dcy = make_rows(78, HARD_S)
    r = HARD_ROWS
    with torch.no_grad():
        if kind == "x0":
            x[r] = 0.0
        elif kind == "h0c0":
            h[r] = 0.0
            c[r] = 0.0
        elif kind == "const_gi":
            # x = 0 leaves gi = bih; a constant bih gives a constant row: variance 0, the eps of the norm decides
            cell.bias_ih.fill_(0.75)
            x[r] = 0.0
        elif kind == "saturated":
            # column 3 of Wih / Whh carries +-30 at one entry of every gate block; ordinary rows have x[3] = h[3] = 0,
            # the hard rows xin[3] = h[3] = 1: pre-norm pre-activations of +-30 there, and after the two norms the gates
            # of those channels sit at +-11
            x[:, 3] = 0.0
            h[:, 3] = 0.0
            h[r, 3] = 1.0
            for o, sgn in ((5, 1.0), (32 + 9, -1.0), (64 + 17, 1.0), (96 + 30, -1.0)):
                cell.weight_ih[o, 3] = 30.0 * sgn
                cell.weight_hh[o, 3] = 30.0 * sgn
            x[r, 3] = 1.0 / torch.sigmoid(cell.ig(h))[r, 3]
        elif kind == "big_c":
            c[r] = 50.0 * torch.sign(c[r])
        else:
            raise ValueError(kind)
    return cell, x, h, c, dhy, dcy


def check_hardness(kind, k):
    """the fp64 forward confirms that the rows are what the case names"""
    r = HARD_ROWS
    if kind == "const_gi":
        assert float(np.ptp(k["pre_gi"][r], axis=1).max()) == 0.0 and float(np.abs(k["gi"][r]).max()) == 0.0
        assert np.allclose(k["si"][r], 1.0 / np.sqrt(1e-5))
    elif kind == "saturated":
        assert 29.0 <= float(np.abs(k["pre_gi"][r]).max()) <= 35.0 and 29.0 <= float(np.abs(k["pre_gh"][r]).max()) <= 35.0
        assert float(k["i"][r, 5].min()) > 1 - 1e-4 and float(k["f"][r, 9].max()) < 1e-4
        assert float(k["g"][r, 17].min()) > 1 - 1e-8 and float(k["o"][r, 30].max()) < 1e-4
    elif kind == "big_c":
        assert float(np.abs(k["c"][r]).min()) == 50.0
        assert (np.abs(k["pre_cy"][r]) > 15.0).mean() > 0.5      # tanh(cy) is flat on most of these entries ...
    elif kind == "x0":
        assert float(np.abs(k["xin"][r]).max()) == 0.0
    elif kind == "h0c0":
        assert float(np.abs(k["h"][r]).max()) == 0.0 and float(np.abs(k["c"][r]).max()) == 0.0


@pytest.mark.parametrize("kind", ["x0", "h0c0", "const_gi", "saturated", "big_c"])
def test_fused_cell_on_hard_rows(kind):
    cell, x, h, c, dhy, dcy = hard_case(kind)
    want, k = ref_cell(cell, x, h, c, dhy, dcy)
    check_hardness(kind, k)
    got = run_cell(cell, x, h, c, dhy, dcy)
    compare(got, want, kind, rows=HARD_ROWS)
    if kind == "big_c":
        # ... and dc still carries f there: dc = dcy * f where tanh(cy) is flat
        sat = np.abs(k["pre_cy"][HARD_ROWS]) > 15.0            # 1 - tanh^2 < 4e-13: nothing of dhy reaches dc
        dc = got["dc"].cpu().double().numpy()[HARD_ROWS]
        assert np.allclose(dc[sat], (dcy.numpy()[HARD_ROWS] * k["f"][HARD_ROWS])[sat], rtol=1e-3, atol=1e-4)
        assert float(np.abs(dc[sat]).max()) > 0.1


@pytest.mark.parametrize("up", ["dhy", "dcy", "both"])
def test_either_upstream_gradient_may_be_absent(up, monkeypatch):
    S = WG_ROWS + 7
    cell = make_cell(11)
    x, h, c, dhy, dcy = make_rows(12, S)
    dhy, dcy = (dhy if up != "dcy" else None), (dcy if up != "dhy" else None)
    seen = []
    monkeypatch.setattr(wsis_native, "ptr", lambda t, _f=wsis_native.ptr: (seen.append(t is None), _f(t))[1])
    want, _ = ref_cell(cell, x, h, c, dhy, dcy)
    got = run_cell(cell, x, h, c, dhy, dcy)
    assert sum(seen) == (0 if up == "both" else 1), "an absent gradient goes to the kernel as NULL, not as zeros"
    compare(got, want, "upstream " + up)


def test_parameter_gradients_are_bit_identical_over_two_runs():
    cell = make_cell(21)
    rows = make_rows(22, S_REDUCE)
    a, b = run_cell(cell, *rows), run_cell(cell, *rows)
    for name in a:
        assert torch.equal(a[name], b[name]), name


# ---------------------------------------------------------------- the recurrence
@pytest.fixture(scope="module")
def rec_graph():
    """54 nodes: an in-hub of 33 edges, a node without in-edges, an isolated node; edges in target order"""
    eu, ev, roles = graph_ref.hub_graph(5, 54, in_hubs=(33,), no_in=1, isolated=1)
    _, (src, tgt) = graph_ref.edge_orders(eu, ev)
    g = torch.Generator().manual_seed(6)
    return dict(src=src, tgt=tgt, S=54, feats=torch.randn(len(src), 13, generator=g), x=torch.randn(54, 32, generator=g),
                gout=torch.randn(54, 32 * 4, generator=g), roles=roles)


@pytest.mark.parametrize("contract", [1, 0])
@pytest.mark.parametrize("cat_all", [True, False])
@pytest.mark.parametrize("R", [0, 1, 3])
def test_recurrence_equals_the_fp64_recurrence(rec_graph, R, cat_all, contract, monkeypatch):
    G = rec_graph
    assert G["roles"]["isolated"] and G["roles"]["no_in"] and max(G["roles"]["in_hub"].values()) == 33
    monkeypatch.setenv("WSIS_ECC_CONTRACT", str(contract))
    torch.manual_seed(40 + R)
    fnet = graphnet.create_fnet([13, 32, 128, 64, 32 * 32], True, True, -1)
    mod = graphnet.RNNGraphConvModule(make_cell(41), fnet, 32, vv=False, nrepeats=R, cat_all=cat_all)
    ref = copy.deepcopy(mod).double()
    mod = mod.to(DEV)
    ei = torch.from_numpy(np.stack([G["src"], G["tgt"]]))
    mod.set_info(graphnet.GraphConvInfo(ei.to(DEV), G["feats"].to(DEV), G["S"]))
    x = G["x"].clone().to(DEV).requires_grad_(True)
    assert mod._contract_ok(x) == bool(contract)
    calls = []
    monkeypatch.setattr(wsis_ops, "lstm_cell_ex", lambda *a, _f=wsis_ops.lstm_cell_ex: (calls.append(1), _f(*a))[1])
    out = mod(x)
    assert len(calls) == R, "every repeat runs the fused cell"
    gout = G["gout"][:, :32 * (R + 1)] if cat_all else G["gout"][:, :32]
    out.backward(gout.to(DEV))
    # fp64: the filters from the float64 filter net, the recurrence in numpy, the filter gradient back through the net
    W = ref._fnet(G["feats"].double()).view(-1, 32, 32)
    want, gr = lstm_ref.recurrence(lstm_ref.params_of(ref._cell), G["x"].numpy(), W.detach().numpy(), G["src"], G["tgt"],
                                   R, cat_all, gout.numpy())
    W.backward(torch.from_numpy(gr["dW"]))
    rep = {"out": ratio(out, want, FWD), "dhx": ratio(x.grad, gr["dhx"], GRAD)}
    if R > 0:
        for n, p in mod._cell.named_parameters():
            rep[n] = ratio(p.grad, gr[n], GRAD)
        for (n, p), (_, q) in zip(mod._fnet.named_parameters(), ref._fnet.named_parameters()):
            rep["fnet." + n] = ratio(p.grad, q.grad.numpy(), GRAD)
    print(f"R={R} cat_all={cat_all} contract={contract}", {k: "%.2g" % v for k, v in rep.items()})
    assert all(v <= 1.0 for v in rep.values()), rep


def test_gru_recurrence_still_takes_its_one_node_loop(rec_graph, monkeypatch):
    """the GRU cell's path through the module is what it was: one ecc_gru_loop call, no per-repeat cell call"""
    G = rec_graph
    torch.manual_seed(3)
    net = graphnet.GraphNetwork("gru_3_0", 32, [13, 32, 128, 64]).to(DEV)
    mod = net.gconvs[0]
    mod.set_info(graphnet.GraphConvInfo(torch.from_numpy(np.stack([G["src"], G["tgt"]])).to(DEV), G["feats"].to(DEV), G["S"]))
    calls = {"loop": 0, "cell": 0, "lstm": 0}
    for key, name in (("loop", "ecc_gru_loop"), ("cell", "gru_cell_ex"), ("lstm", "lstm_cell_ex")):
        monkeypatch.setattr(wsis_ops, name,
                            lambda *a, _f=getattr(wsis_ops, name), _k=key: (calls.__setitem__(_k, calls[_k] + 1), _f(*a))[1])
    assert mod(G["x"].to(DEV)).shape == (G["S"], 32 * 4)
    assert calls == {"loop": 1, "cell": 0, "lstm": 0}


# ---------------------------------------------------------------- the reference's model file on the device
def test_lstm_network_matches_the_reference_model_file_on_the_device(monkeypatch):
    calls = []
    monkeypatch.setattr(wsis_ops, "lstm_cell_ex", lambda *a, _f=wsis_ops.lstm_cell_ex: (calls.append(1), _f(*a))[1])
    net, x, g = golden_network(DEV)
    worst = check_golden(net, x, g, 2e-5)             # the same bound as on the host
    print({k: "%.1e" % v for k, v in worst.items()})
    assert len(calls) == 3


# ---------------------------------------------------------------- dispatch
@pytest.mark.parametrize("how", ["env", "layernorm", "ingate"])
def test_the_module_walk_runs_where_the_fused_kernel_does_not_apply(how, monkeypatch):
    S = 40
    torch.manual_seed(50)
    cell = graphnet.LSTMCellEx(32, 32, bias=True, layernorm=how != "layernorm", ingate=how != "ingate")
    x, h, c, dhy, dcy = make_rows(51, S)
    calls = []
    monkeypatch.setattr(wsis_ops, "lstm_cell_ex", lambda *a, _f=wsis_ops.lstm_cell_ex: (calls.append(1), _f(*a))[1])
    if how == "env":
        fused = run_cell(cell, x, h, c, dhy, dcy)
        assert len(calls) == 1
        monkeypatch.setenv("WSIS_FUSE_GRU", "0")
    walk = run_cell(cell, x, h, c, dhy, dcy)
    assert len(calls) == (1 if how == "env" else 0), "the module walk must not call the fused cell"
    P = lstm_ref.params_of(cell)
    hy, cy, k = lstm_ref.cell_fwd(P, x.numpy(), h.numpy(), c.numpy(), how != "layernorm", how != "ingate")
    want = lstm_ref.cell_bwd(P, k, dhy.numpy(), dcy.numpy())
    want.update(hy=hy, cy=cy)
    compare(walk, want, "walk " + how)
    if how == "env":
        compare(fused, want, "fused")
        compare(fused, {n: v.cpu().double().numpy() for n, v in walk.items()}, "fused against the walk")
