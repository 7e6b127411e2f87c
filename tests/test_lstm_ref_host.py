"""LSTMCellEx, the ``lstm_*`` config token and the cell-state carrying recurrence on the CPU: the fp64 restatement of
tests/lstm_ref.py against torch autograd over ``LSTMCellEx.forward_reference``, the plain ``torch.nn.LSTMCell`` as the
special case without layernorm / ingate, the token grammar of the reference (graphnet.py:77-92), and the reference's own
model file through tests/golden/lstm_golden.npz."""
import os

import numpy as np
import pytest
import torch

import graphnet
from tests import lstm_ref
from tests.util import seeded_state_dict

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lstm_golden.npz")
FNET = [13, 32, 128, 64]


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def _seeded_cell(seed, layernorm, ingate, H=32):
    torch.manual_seed(seed)
    cell = graphnet.LSTMCellEx(H, H, bias=True, layernorm=layernorm, ingate=ingate).double()
    with torch.no_grad():
        for p in cell.parameters():
            p.copy_(torch.randn_like(p) * 0.4)
    return cell


@pytest.mark.parametrize("layernorm,ingate", [(1, 1), (1, 0), (0, 1), (0, 0)])
@pytest.mark.parametrize("up", ["both", "dhy", "dcy"])
def test_fp64_restatement_equals_autograd_over_forward_reference(layernorm, ingate, up):
    S, H = 9, 32
    cell = _seeded_cell(3, bool(layernorm), bool(ingate))
    g = torch.Generator().manual_seed(5)
    x, h, c = (torch.randn(S, H, generator=g, dtype=torch.float64).requires_grad_(True) for _ in range(3))
    dhy, dcy = torch.randn(S, H, generator=g, dtype=torch.float64), torch.randn(S, H, generator=g, dtype=torch.float64)
    hy, cy = cell.forward_reference(x, (h, c))
    ((hy * dhy).sum() * (up != "dcy") + (cy * dcy).sum() * (up != "dhy")).backward()
    P = lstm_ref.params_of(cell)
    assert set(P) == (set(lstm_ref.NAMES) if ingate else set(lstm_ref.NAMES[:4]))
    rhy, rcy, k = lstm_ref.cell_fwd(P, x.detach().numpy(), h.detach().numpy(), c.detach().numpy(), bool(layernorm),
                                    bool(ingate))
    b = lstm_ref.cell_bwd(P, k, None if up == "dcy" else dhy.numpy(), None if up == "dhy" else dcy.numpy())
    assert np.allclose(rhy, hy.detach().numpy(), rtol=1e-12, atol=1e-13)
    assert np.allclose(rcy, cy.detach().numpy(), rtol=1e-12, atol=1e-13)
    for name, want in [("dx", x.grad), ("dh", h.grad), ("dc", c.grad)] + [(n, p.grad) for n, p in cell.named_parameters()]:
        assert np.allclose(b[name], want.numpy(), rtol=1e-10, atol=1e-11), name


def test_without_layernorm_and_ingate_the_cell_is_torch_lstmcell():
    S, H = 7, 32
    cell = _seeded_cell(4, False, False).float()
    plain = torch.nn.LSTMCell(H, H)
    plain.load_state_dict(cell.state_dict(), strict=True)
    g = torch.Generator().manual_seed(6)
    x, h, c = (torch.randn(S, H, generator=g) for _ in range(3))
    hy, cy = cell(x, (h, c))
    py, pc = plain(x, (h, c))
    assert torch.allclose(hy, py, rtol=1e-5, atol=1e-6) and torch.allclose(cy, pc, rtol=1e-5, atol=1e-6)


def _graph(seed, S, E):
    """edges sorted by target; node 0 has no in-edges, node 1 is a hub (a third of all edges end there)"""
    rng = np.random.default_rng(seed)
    src = rng.integers(0, S, E)
    tgt = np.where(rng.random(E) < 0.33, 1, rng.integers(1, S, E))
    keep = src != tgt
    src, tgt = src[keep], tgt[keep]
    order = np.argsort(tgt, kind="stable")
    ei = torch.from_numpy(np.stack([src[order], tgt[order]]).astype(np.int64))
    return ei, torch.from_numpy(rng.standard_normal((ei.shape[1], 13)).astype(np.float32))


def test_lstm_network_runs_on_the_cpu_and_equals_the_fp64_recurrence():
    torch.manual_seed(0)
    net = graphnet.GraphNetwork("lstm_2_0,f_8", nfeat=32, fnet_widths=list(FNET)).double()
    gconv = net.gconvs[0]
    assert isinstance(gconv._cell, graphnet.LSTMCellEx) and gconv._isLSTM
    ei, ef = _graph(1, 20, 70)
    net.set_info(graphnet.GraphConvInfo(ei, ef.double(), 20), cuda=False)
    x = torch.randn(20, 32, dtype=torch.float64)
    out = net(x)
    assert out.shape == (20, 8)
    with torch.no_grad():
        W = gconv._fnet(ef.double()).view(-1, 32, 32).numpy()
        want = lstm_ref.recurrence(lstm_ref.params_of(gconv._cell), x.numpy(), W, ei[0].numpy(), ei[1].numpy(), 2, True)
        got = gconv(x)
    assert got.shape == (20, 96) and np.allclose(got.numpy(), want, rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("kind", ["lstm", "gru"])
def test_gate_defaults_parse_as_in_the_reference(kind):
    cell_type = {"lstm": graphnet.LSTMCellEx, "gru": graphnet.GRUCellEx}[kind]
    net = graphnet.GraphNetwork(kind + "_3,f_8", nfeat=32, fnet_widths=list(FNET))
    gconv = net._modules["0"]
    assert type(gconv._cell) is cell_type and gconv._isLSTM == (kind == "lstm")
    assert gconv._vv and gconv._cell._layernorm and gconv._cell._ingate and gconv._cat_all and gconv._nrepeats == 3
    assert gconv._fnet[-1].out_features == 32                     # vv: one weight per channel
    assert net._modules["1"].in_features == 32 * (3 + 1)          # cat_all multiplies nfeat by R + 1
    net = graphnet.GraphNetwork(kind + "_2_0_0_1_0,f_8", nfeat=32, fnet_widths=list(FNET))
    gconv = net._modules["0"]
    assert not gconv._vv and not gconv._cell._layernorm and gconv._cell._ingate and not gconv._cat_all
    assert gconv._fnet[-1].out_features == 32 * 32 and net._modules["1"].in_features == 32
    assert "ig" in gconv._cell._modules and set(gconv._cell._modules) == {"ig"}
    assert gconv._cell.weight_ih.shape == ((4 if kind == "lstm" else 3) * 32, 32)


def test_gru_strings_build_what_they_built_before():
    net = graphnet.GraphNetwork("gru_7_0,f_64,b,r", nfeat=32, fnet_widths=list(FNET), fnet_bnidx=2)
    names = sorted(net.state_dict())
    assert type(net._modules["0"]._cell) is graphnet.GRUCellEx and not net._modules["0"]._isLSTM
    assert [n for n in names if n.startswith("0._cell")] == [
        "0._cell.bias_hh", "0._cell.bias_ih", "0._cell.ig.bias", "0._cell.ig.weight", "0._cell.weight_hh",
        "0._cell.weight_ih"]
    assert net.state_dict()["0._cell.weight_ih"].shape == (96, 32)
    assert net._modules["1"].in_features == 32 * 8
    with pytest.raises(NotImplementedError):
        graphnet.GraphNetwork("crf_2", nfeat=32, fnet_widths=list(FNET))


def test_network_default_keeps_its_state_dict_and_the_lstm_variant_is_reachable():
    import harness
    import backbone_3D_WSIS
    cfg = harness.default_cfg()
    names = list(backbone_3D_WSIS.Network(cfg.model).state_dict())
    assert len(names) == 361 and "ecc.0._cell.weight_ih" in names
    lstm = backbone_3D_WSIS.Network(cfg.model, ecc_config="lstm_7_0,f_64,b,r")
    assert isinstance(lstm.ecc._modules["0"]._cell, graphnet.LSTMCellEx)
    assert list(lstm.state_dict()) == names
    assert lstm.state_dict()["ecc.0._cell.weight_ih"].shape == (128, 32)


# ---------------------------------------------------------------- the reference's own model file (lstm_golden.npz)
def golden_network(dev="cpu"):
    """this build's GraphNetwork('lstm_3_0,f_8') with the fixture's weights, loaded strictly, and its inputs"""
    g = np.load(GOLD)
    torch.manual_seed(0)
    net = graphnet.GraphNetwork("lstm_3_0,f_8", nfeat=32, fnet_widths=list(FNET))
    sd = net.state_dict()
    assert sorted(sd) == list(g["state_names"]), "the state dict must carry the reference's names"
    net.load_state_dict(seeded_state_dict({k: v.shape for k, v in sd.items()}), strict=True)
    net = net.to(dev)
    S = g["in_x"].shape[0]
    net.set_info(graphnet.GraphConvInfo(torch.from_numpy(g["in_edge_indexes"]).to(dev),
                                        torch.from_numpy(g["in_edgefeats"]).to(dev), S), cuda=dev != "cpu")
    return net, torch.from_numpy(g["in_x"]).to(dev).requires_grad_(True), g


def check_golden(net, x, g, tol):
    """output and the gradients of its sum (node features, every parameter) within ``tol`` relative L2 error of what the
    reference's model file gave; returns the figures"""
    out = net(x)
    out.sum().backward()
    worst = {"out": _rel(out.detach().cpu().numpy(), g["out"]), "grad_x": _rel(x.grad.cpu().numpy(), g["grad_x"])}
    for n, p in net.named_parameters():
        worst["grad_" + n] = _rel(p.grad.cpu().numpy(), g["grad_" + n])
    bad = {k: v for k, v in worst.items() if not v <= tol}
    assert not bad, bad
    return worst


def test_fixture_has_a_node_without_in_edges_and_a_hub():
    g = np.load(GOLD)
    S, tgt = g["in_x"].shape[0], g["in_edge_indexes"][1]
    deg = np.bincount(tgt, minlength=S)
    assert 35 <= S <= 45 and 120 <= tgt.size <= 180 and deg.min() == 0 and deg.max() >= 20
    assert (np.diff(tgt) >= 0).all()


def test_lstm_network_matches_the_reference_model_file():
    net, x, g = golden_network()
    check_golden(net, x, g, 2e-5)          # the host bound of the GRU network fixture (tests/test_network_golden.py)
