"""Superpoint graph network 'gru_7_0,f_64,b,r' of 3D-WSIS ("next" row 8f-1): plain-torch
restatement on top of the HIP segmented mean, same parameter names as the reference so its checkpoints load
(modules/model/graphnet.py:19-114, modules/model/spg_modules.py:61-121,128-185,207-253,264-318; state-dict grammar
in SURVEY App. B: ``ecc.0._cell.*``, ``ecc.0._fnet.{0,2,4,5,7}``, ``ecc.1``, ``ecc.2``).  The ``lstm_R_...`` token
builds the same network around LSTMCellEx.
"""
import os

import torch
import torch.nn as nn
import torch.nn.functional as F
import torch.nn.init as init

from torch_scatter import SegmentCSR, scatter


class GraphConvInfo(object):
    """Vectorised graph structure of a batch (replaces modules/model/ecc/GraphConvInfo.py:34-87, without
    igraph): ``edge_indexes`` int64 [2,E] = (source, target) SORTED BY TARGET within each graph and
    ``edgefeats`` fp32 [E,13] in that same order."""

    def __init__(self, edge_indexes, edgefeats, num_nodes):
        self._edge_indexes = edge_indexes
        self._edgefeats = edgefeats
        self.num_nodes = int(num_nodes)
        self._csr = None

    def cuda(self):
        if not self._edge_indexes.is_cuda:
            self._edge_indexes = self._edge_indexes.cuda()
            self._edgefeats = self._edgefeats.cuda()
        return self

    def get_buffers(self):
        return self._edgefeats

    def get_pyg_buffers(self):
        return self._edge_indexes

    def csr(self):
        if self._csr is None:
            self._csr = SegmentCSR(self._edge_indexes[0], self.num_nodes)
        return self._csr

    def csr_dst(self):
        if getattr(self, "_csr_dst", None) is None:
            self._csr_dst = SegmentCSR(self._edge_indexes[1], self.num_nodes)
        return self._csr_dst


def create_fnet(widths, orthoinit, llbias, bnidx=-1):
    """filter-generating MLP (graphnet.py:19-36)"""
    mods = []
    for k in range(len(widths) - 2):
        mods.append(nn.Linear(widths[k], widths[k + 1]))
        if orthoinit:
            init.orthogonal_(mods[-1].weight, gain=init.calculate_gain("relu"))
        if bnidx == k:
            mods.append(nn.BatchNorm1d(widths[k + 1]))
        mods.append(nn.ReLU(True))
    mods.append(nn.Linear(widths[-2], widths[-1], bias=llbias))
    if orthoinit:
        init.orthogonal_(mods[-1].weight)
    if bnidx == len(widths) - 1:
        mods.append(nn.BatchNorm1d(mods[-1].weight.size(0)))
    return nn.Sequential(*mods)


def _run_modules(mods, x):
    """nn.Sequential semantics over ``mods`` with the device forms of the plain layers: Linear over many rows through
    ``tall_linear`` (weight gradient = a [Cin x Cout] output reduced over the rows: one workgroup in hipBLASLt, the
    row-split MFMA reduction here), BatchNorm1d (+ a following ReLU) as the fused two-kernel form instead of four
    torch launches each way.  WSIS_FNET_TALL=0 / WSIS_FUSE_BN=0: the modules as they are."""
    if not x.is_cuda:
        for m in mods:
            x = m(x)
        return x
    import wsis_ops
    tall = os.environ.get("WSIS_FNET_TALL", "1") != "0"
    fuse_bn = os.environ.get("WSIS_FUSE_BN", "1") != "0"
    i = 0
    while i < len(mods):
        m = mods[i]
        if tall and type(m) is nn.Linear and x.dim() == 2:
            x = wsis_ops.tall_linear(x, m)
        elif type(m) is nn.BatchNorm1d and x.dim() == 2 and wsis_ops.sync_group(m) is not None:
            # statistics shared across ranks: always the collective form (zero / one row and non-affine layers included;
            # a rank on another path would leave its peers waiting in the all-reduce)
            relu = i + 1 < len(mods) and type(mods[i + 1]) is nn.ReLU
            x = wsis_ops.batch_norm_relu(x.float(), m, relu=relu)
            i += 1 if relu else 0
        elif (fuse_bn and type(m) is nn.BatchNorm1d and x.dim() == 2 and m.affine and x.shape[0] > 1
              and x.dtype == torch.float32):
            relu = i + 1 < len(mods) and type(mods[i + 1]) is nn.ReLU
            x = wsis_ops.batch_norm_relu(x, m, relu=relu)
            i += 1 if relu else 0
        else:
            x = m(x)
        i += 1
    return x


class GRUCellEx(nn.GRUCell):
    """GRU cell with per-row normalisation of the gate pre-activations and an input gate
    (spg_modules.py:207-253).  The reference's InstanceNorm1d(1) over [S,1,3H] is a per-row
    (x-mean)/sqrt(var+1e-5) without affine parameters."""

    def __init__(self, input_size, hidden_size, bias=True, layernorm=True, ingate=True):
        super().__init__(input_size, hidden_size, bias)
        self._layernorm = layernorm
        self._ingate = ingate
        if ingate:
            self.add_module("ig", nn.Linear(hidden_size, input_size, bias=True))

    @staticmethod
    def _rownorm(x):
        mu = x.mean(dim=1, keepdim=True)
        var = x.var(dim=1, unbiased=False, keepdim=True)
        return (x - mu) / torch.sqrt(var + 1e-5)

    def forward(self, input, hidden):
        import os
        if (input.is_cuda and self._ingate and self._layernorm and self.bias and input.shape[1] == 32
                and self.hidden_size == 32 and input.shape[0] > 0 and os.environ.get("WSIS_FUSE_GRU", "1") != "0"):
            import wsis_ops
            return wsis_ops.gru_cell_ex(input, hidden, self)   # one HIP kernel instead of ~30 launches
        return self.forward_reference(input, hidden)

    def forward_reference(self, input, hidden):
        if self._ingate:
            input = torch.sigmoid(self._modules["ig"](hidden)) * input
        gi = F.linear(input, self.weight_ih)
        gh = F.linear(hidden, self.weight_hh)
        if self._layernorm:
            gi, gh = self._rownorm(gi), self._rownorm(gh)
        i_r, i_i, i_n = gi.chunk(3, 1)
        h_r, h_i, h_n = gh.chunk(3, 1)
        bih_r, bih_i, bih_n = self.bias_ih.chunk(3)
        bhh_r, bhh_i, bhh_n = self.bias_hh.chunk(3)
        resetgate = torch.sigmoid(i_r + bih_r + h_r + bhh_r)
        inputgate = torch.sigmoid(i_i + bih_i + h_i + bhh_i)
        newgate = torch.tanh(i_n + bih_n + resetgate * (h_n + bhh_n))
        return newgate + inputgate * (hidden - newgate)


class LSTMCellEx(nn.LSTMCell):
    """LSTM cell with per-row normalisation of the gate pre-activations and an input gate
    (spg_modules.py:264-318), the cell of the ``lstm_R_...`` configurations.  Unlike GRUCellEx the biases are added
    BEFORE the row norm (spg_modules.py:298-300).  Gate order i, f, g, o as nn.LSTMCell."""

    def __init__(self, input_size, hidden_size, bias=True, layernorm=True, ingate=True):
        super().__init__(input_size, hidden_size, bias)
        self._layernorm = layernorm
        self._ingate = ingate
        if ingate:
            self.add_module("ig", nn.Linear(hidden_size, input_size, bias=True))

    def forward(self, input, hidden):
        if (input.is_cuda and self._ingate and self._layernorm and self.bias and input.shape[1] == 32
                and self.hidden_size == 32 and input.shape[0] > 0 and os.environ.get("WSIS_FUSE_GRU", "1") != "0"):
            import wsis_ops
            return wsis_ops.lstm_cell_ex(input, hidden[0], hidden[1], self)   # one HIP kernel instead of ~30 launches
        return self.forward_reference(input, hidden)

    def forward_reference(self, input, hidden):
        hx, cx = hidden
        if self._ingate:
            input = torch.sigmoid(self._modules["ig"](hx)) * input
        gi = F.linear(input, self.weight_ih, self.bias_ih)
        gh = F.linear(hx, self.weight_hh, self.bias_hh)
        if self._layernorm:
            gi, gh = GRUCellEx._rownorm(gi), GRUCellEx._rownorm(gh)
        ingate, forgetgate, cellgate, outgate = (gi + gh).chunk(4, 1)
        ingate, forgetgate, outgate = torch.sigmoid(ingate), torch.sigmoid(forgetgate), torch.sigmoid(outgate)
        cellgate = torch.tanh(cellgate)
        cy = forgetgate * cx + ingate * cellgate
        hy = outgate * torch.tanh(cy)
        return hy, cy


class RNNGraphConvModule(nn.Module):
    """R x { edge-conditioned message passing -> GRUCellEx or LSTMCellEx } (spg_modules.py:152-185 with the PyG NNConv
    of :61-121).  With an LSTM cell the recurrence carries a cell state: cx starts as zeros of hx's shape, every repeat
    does hx, cx = cell(inp, (hx, cx)), only the hx are concatenated (:170-183); it runs op by op on both paths.

    Direction: a node receives the MEAN over its IN-edges (s -> t) of x[s] @ W_e.  NNConv's constructor names a
    ``flow="target_to_source"`` parameter but never hands it to ``MessagePassing.__init__`` (spg_modules.py:61-72:
    ``super().__init__(aggr=aggr, **kwargs)``), so PyG's default ``source_to_target`` is what runs: x_j = x[edge_index[0]]
    aggregated at edge_index[1] -- the same sum the non-PyG branch forms (ecc/GraphConvModule.py:49-78: sources
    ``idxn`` sorted by target, averaged over the in-degree).  Pinned by tests/golden/network_golden.npz, which runs the
    reference's own module file (round 1-2 of this build had the two ends exchanged)."""

    def __init__(self, cell, filter_net, nfeat, vv=True, nrepeats=1, cat_all=False):
        super().__init__()
        self._cell = cell
        self._isLSTM = isinstance(cell, nn.LSTMCell)     # the recurrence carries a cell state (spg_modules.py:137,170-171)
        self._fnet = filter_net
        self._nrepeats = nrepeats
        self._cat_all = cat_all
        self._vv = vv
        self._gci = None

    def set_info(self, gc_info):
        self._gci = gc_info
        self._pre = None

    def _step(self, inp, hx, cx):
        """one cell evaluation -> (hx, cx); cx is None for the GRU cell"""
        if self._isLSTM:
            return self._cell(inp, (hx, cx))
        return self._cell(inp, hx), None

    def _filter_state(self):
        """(h [E,64], W' [32, 65*32]) of the filter-free evaluation: the fnet hidden state of every edge and the last
        Linear folded per node channel -- functions of the edge features and the parameters alone"""
        last = self._fnet[-1]
        h = _run_modules(list(self._fnet[:-1]), self._gci.get_buffers())     # fnet hidden state [E, 64]
        # W'[a, c*32 + b] = Wl[a*32 + b, c];  W'[a, 64*32 + b] = bl[a*32 + b]
        Waug = torch.cat([last.weight.view(32, 32, 64).permute(0, 2, 1).reshape(32, 64 * 32),
                          last.bias.view(32, 32)], 1)
        return h, Waug

    def prefetch_filter_state(self, stream, ready=None):
        """run the filter net on ``stream`` now (it does not depend on the node features): its five launches run beside
        the sparse UNet instead of between UNet and recurrence, and -- autograd runs a node's backward on the stream of
        its forward -- its ~20 backward launches beside the UNet's backward pass instead of in front of it.  The state is
        handed to the next ``forward`` (which makes the current stream wait for ``stream``)."""
        if self._gci is None or not self._contract_ok(None):
            return
        # the parameters must be final: ``ready`` = an event recorded on the main stream behind the previous optimizer step
        # (None: everything queued so far)
        if ready is not None:
            stream.wait_event(ready)
        else:
            stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            h, Waug = self._filter_state()
            done = torch.cuda.Event()
            done.record(stream)              # (the consumer waits for this, not for what else the stream gets later)
        self._pre = (h, Waug, done)

    def _contract_ok(self, hx):
        """the filter-free evaluation applies to the model's configuration: 32 node channels, a filter net that ends
        in Linear(64 -> 32*32) with bias (graphnet.py:77-92), on the GPU; WSIS_ECC_CONTRACT=0 keeps the [E,1024] path"""
        import os
        last = self._fnet[-1]
        if hx is None:       # asked before the node features exist (prefetch): the model's width
            node_ok = self._cell.hidden_size == 32 and self._gci.get_buffers().is_cuda
        else:
            node_ok = hx.is_cuda and hx.size(1) == 32
        return (node_ok and isinstance(last, nn.Linear) and last.in_features == 64
                and last.out_features == 1024 and last.bias is not None and len(self._fnet) >= 2
                and os.environ.get("WSIS_ECC_CONTRACT", "1") != "0")

    def _forward_contract(self, hx):
        """7 x { U = x @ W' (per node) -> m_e = h_e . U_s (per edge, one kernel) -> mean over the in-edges -> GRU }:
        the per-edge filters W_e = reshape(Wl h_e + bl) [E, 1024] of the reference (spg_modules.py:168-183) are never
        formed; what is kept per step is the per-node U [S, 65*32]."""
        import wsis_ops
        edge_indexes = self._gci.get_pyg_buffers()
        tgt = edge_indexes[1]                      # messages are aggregated at the edge's target
        pre, self._pre = getattr(self, "_pre", None), None
        if pre is not None:          # computed ahead on a branch stream (prefetch_filter_state)
            h, Waug, done = pre
            main = torch.cuda.current_stream()
            main.wait_event(done)
            h.record_stream(main)
            Waug.record_stream(main)
        else:
            h, Waug = self._filter_state()
        csr_gat, csr_agg = self._gci.csr(), self._gci.csr_dst()      # gather side = sources, aggregation side = targets
        cell = self._cell
        if (not self._isLSTM and os.environ.get("WSIS_GNN_LOOP", "1") != "0" and os.environ.get("WSIS_FUSE_GRU", "1") != "0"
                and getattr(cell, "_ingate", False) and getattr(cell, "_layernorm", False) and cell.bias
                and getattr(cell, "hidden_size", 0) == 32 and hx.shape[0] > 0 and h.shape[0] > 0):
            # the whole recurrence as one autograd node (same kernels, same order)
            return wsis_ops.ecc_gru_loop(hx, h, Waug, cell, csr_agg, csr_gat, self._nrepeats, self._cat_all)
        hxs = [hx]
        cx = torch.zeros_like(hx) if self._isLSTM else None         # (the LSTM cell runs op by op: no one-node loop yet)
        for _ in range(self._nrepeats):
            U = hx @ Waug                                                  # [S, 65*32]
            msg = wsis_ops.ecc_contract(h, U, csr_gat)                     # [E, 32]: m_e = h_e . U[source_e]
            inp = scatter(msg, tgt, dim=0, dim_size=hx.size(0), reduce="mean", csr=csr_agg)
            hx, cx = self._step(inp, hx, cx)
            hxs.append(hx)
        return torch.cat(hxs, 1) if self._cat_all else hx

    def forward(self, hx):
        if self._contract_ok(hx):
            return self._forward_contract(hx)
        edgefeats = self._gci.get_buffers()
        edge_indexes = self._gci.get_pyg_buffers()
        src, dst = edge_indexes[0], edge_indexes[1]
        weights = self._fnet(edgefeats)
        nc = hx.size(1)
        assert weights.size(1) in (nc, nc * nc)
        if weights.size(1) != nc:
            weights = weights.view(-1, nc, nc)
        fused = weights.dim() == 3 and nc <= 32 and hx.is_cuda
        csr_agg = self._gci.csr_dst() if hx.is_cuda else None
        if fused:
            import wsis_ops
            src_c, dst_c = src.contiguous(), dst.contiguous()
            csr_gat = self._gci.csr()
        hxs = [hx]
        cx = torch.zeros_like(hx) if self._isLSTM else None
        for _ in range(self._nrepeats):
            if fused:
                # gather + per-edge mat-vec + mean over the in-edges in ONE kernel (and one for the backward):
                # wsis_ops.ecc_message(x, w, agg_index, gather_index, csr over agg, csr over gather)
                inp = wsis_ops.ecc_message(hx, weights, dst_c, src_c, csr_agg, csr_gat)
            else:
                x_j = hx[src]
                msg = torch.bmm(x_j.unsqueeze(1), weights).squeeze(1) if weights.dim() == 3 else x_j * weights
                if hx.is_cuda:
                    inp = scatter(msg, dst, dim=0, dim_size=hx.size(0), reduce="mean", csr=csr_agg)
                else:       # (the segmented mean is a device operator; on the host the same mean in plain torch)
                    deg = torch.bincount(dst, minlength=hx.size(0)).clamp(min=1).to(msg.dtype).unsqueeze(1)
                    inp = torch.zeros_like(hx).index_add_(0, dst, msg) / deg
            hx, cx = self._step(inp, hx, cx)
            hxs.append(hx)
        return torch.cat(hxs, 1) if self._cat_all else hx


class GraphNetwork(nn.Module):
    """config-string driven container (graphnet.py:39-114); supports the tokens the reference uses:
    gru_R_vv_layernorm_ingate_catall, lstm_R_vv_layernorm_ingate_catall, f_N, b, r, d_p (not crf: it needs
    ecc.GraphConvModule)."""

    def __init__(self, config, nfeat, fnet_widths, fnet_orthoinit=True, fnet_llbias=True, fnet_bnidx=-1,
                 edge_mem_limit=1e20, use_pyg=True, cuda=True):
        super().__init__()
        self.gconvs = []
        for d, conf in enumerate(config.split(",")):
            conf = conf.strip().split("_")
            if conf[0] == "f":
                self.add_module(str(d), nn.Linear(nfeat, int(conf[1])))
                nfeat = int(conf[1])
            elif conf[0] == "b":
                self.add_module(str(d), nn.BatchNorm1d(nfeat, eps=1e-5, affine=len(conf) == 1))
            elif conf[0] == "r":
                self.add_module(str(d), nn.ReLU(True))
            elif conf[0] == "d":
                self.add_module(str(d), nn.Dropout(p=float(conf[1]), inplace=False))
            elif conf[0] == "gru" or conf[0] == "lstm":
                nrepeats = int(conf[1])
                vv = bool(int(conf[2])) if len(conf) > 2 else True
                layernorm = bool(int(conf[3])) if len(conf) > 3 else True
                ingate = bool(int(conf[4])) if len(conf) > 4 else True
                cat_all = bool(int(conf[5])) if len(conf) > 5 else True
                fnet = create_fnet(fnet_widths + [nfeat ** 2 if not vv else nfeat], fnet_orthoinit, fnet_llbias,
                                   fnet_bnidx)
                cell_type = GRUCellEx if conf[0] == "gru" else LSTMCellEx
                cell = cell_type(nfeat, nfeat, bias=True, layernorm=layernorm, ingate=ingate)
                gconv = RNNGraphConvModule(cell, fnet, nfeat, vv=vv, nrepeats=nrepeats, cat_all=cat_all)
                self.add_module(str(d), gconv)
                self.gconvs.append(gconv)
                if cat_all:
                    nfeat *= nrepeats + 1
            elif len(conf[0]) > 0:
                raise NotImplementedError("Unknown module: " + conf[0])

    def set_info(self, gc_infos, cuda=True):
        gc_infos = gc_infos if isinstance(gc_infos, (list, tuple)) else [gc_infos]
        for i, gc in enumerate(self.gconvs):
            if cuda:
                gc_infos[i].cuda()
            gc.set_info(gc_infos[i])

    def forward(self, input):
        return _run_modules(list(self._modules.values()), input)
