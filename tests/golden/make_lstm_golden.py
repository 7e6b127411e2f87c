"""lstm_golden.npz: what the REFERENCE's own model file computes for its LSTM variant of the superpoint GNN.

Runs ``graphnet.GraphNetwork('lstm_3_0,f_8', nfeat=32, fnet_widths=[13, 32, 128, 64])`` of the reference's
modules/model/graphnet.py (with it ``spg_modules.py`` NNConv / RNNGraphConvModule / LSTMCellEx) on the
CPU, behind the stand-ins of make_network_golden.py for the packages the reference imports and this container lacks.
Input: a seeded graph of 40 nodes and about 150 edges sorted by target, in which node 0 has no in-edges and node 1 is a
hub.  Weights: tests/util.seeded_state_dict (drawn per NAME).  Stored: the inputs, the sorted parameter names, the
output [40, 8] and the gradients of the output's sum with respect to the node features and every parameter.  Only
arrays are written -- no reference source text.

    python tests/golden/make_lstm_golden.py          (needs the reference tree; never runs on the GPU box)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_network_golden as mk      # noqa: E402  (puts the repository root on sys.path)


def make_graph(seed=7, S=40, E=156):
    rng = np.random.default_rng(seed)
    src = rng.integers(0, S, E)
    tgt = np.where(rng.random(E) < 0.2, 1, rng.integers(1, S, E))       # node 0: no in-edges; node 1: hub
    pairs = sorted({(int(s), int(t)) for s, t in zip(src, tgt) if s != t}, key=lambda p: (p[1], p[0]))
    ei = np.array(pairs, dtype=np.int64).T
    return dict(x=rng.standard_normal((S, 32)).astype(np.float32), edge_indexes=np.ascontiguousarray(ei),
                edgefeats=rng.standard_normal((ei.shape[1], 13)).astype(np.float32))


def main():
    batch = make_graph()
    mk.register_standins()
    sys.path.insert(0, os.path.join(mk.REF, "modules", "model"))
    import graphnet as ref_graphnet
    assert ref_graphnet.__file__.startswith(mk.REF)
    from tests.util import seeded_state_dict
    torch.manual_seed(0)
    net = ref_graphnet.GraphNetwork("lstm_3_0,f_8", nfeat=32, fnet_widths=[13, 32, 128, 64], cuda=False)
    sd = net.state_dict()
    net.load_state_dict(seeded_state_dict({k: v.shape for k, v in sd.items()}), strict=True)
    net.set_info(mk._GI(torch.from_numpy(batch["edge_indexes"]), torch.from_numpy(batch["edgefeats"])), cuda=False)
    x = torch.from_numpy(batch["x"]).requires_grad_(True)
    out = net(x)
    out.sum().backward()
    res = {"in_" + k: v for k, v in batch.items()}
    res["state_names"] = np.array(sorted(sd.keys()))
    res["out"] = out.detach().numpy()
    res["grad_x"] = x.grad.numpy()
    for n, p in net.named_parameters():
        res["grad_" + n] = p.grad.numpy()
    path = os.path.join(HERE, "lstm_golden.npz")
    np.savez_compressed(path, **res)
    deg = np.bincount(batch["edge_indexes"][1], minlength=batch["x"].shape[0])
    print("lstm_golden.npz:", os.path.getsize(path), "bytes; nodes", batch["x"].shape[0], "edges",
          batch["edge_indexes"].shape[1], "max in-degree", int(deg.max()), "nodes without in-edges", int((deg == 0).sum()),
          "names", len(sd))


if __name__ == "__main__":
    main()
