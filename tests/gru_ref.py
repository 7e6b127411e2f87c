"""fp64 numpy restatement of GRUCellEx (forward and analytic backward) and of the R-repeat recurrent graph convolution
around it, for the value tests of the fused cell and of the one-node loop (tests/test_gru_ref_host.py,
tests/test_gpu_gru_edges.py).  Written from the formulas, not from the module code:

    xin = sigmoid(Wig h + big) * x
    gi  = rownorm(Wih xin),  gh = rownorm(Whh h)          [3H] each, (v - mean) / sqrt(biased var + 1e-5) over a row;
                                                          the biases stay OUTSIDE the norm (unlike LSTMCellEx)
    r = sigmoid(gi_r + bih_r + gh_r + bhh_r),  z = sigmoid(gi_z + bih_z + gh_z + bhh_z)
    n = tanh(gi_n + bih_n + r * (gh_n + bhh_n)),  hy = n + z * (h - n)

Parameters travel as a dict of float64 arrays under the module's names: weight_ih [3H,C], weight_hh [3H,H], bias_ih,
bias_hh [3H], ig.weight [C,H], ig.bias [C].

The second half of the file holds the inputs the host and the device tests share: the row counts at which the launch
plan of csrc/gru.hip changes (with the plan restated), and the hard rows."""
import numpy as np
import torch

EPS = 1e-5
NAMES = ("weight_ih", "weight_hh", "bias_ih", "bias_hh", "ig.weight", "ig.bias")


def params_of(cell):
    """{name: float64 array} of a torch cell"""
    return {n: p.detach().cpu().double().numpy() for n, p in cell.named_parameters()}


def _sigmoid(v):
    e = np.exp(-np.abs(v))                         # (no overflow at either end, and the small end keeps its digits)
    return np.where(v >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def _rownorm(v):
    mu = v.mean(1, keepdims=True)
    d = v - mu
    s = 1.0 / np.sqrt((d * d).mean(1, keepdims=True) + EPS)
    return d * s, s


def _rownorm_bwd(dy, yhat, s):
    return (dy - dy.mean(1, keepdims=True) - yhat * (dy * yhat).mean(1, keepdims=True)) * s


def cell_fwd(P, x, h):
    """(hy, cache); the cache holds x, h, gin, xin, pre_gi / pre_gh (before the norm), si / sh (the two
    1 / sqrt(var + 1e-5)), gi / gh (normalised), r, z, n"""
    x, h = (np.asarray(a, dtype=np.float64) for a in (x, h))
    k = {"x": x, "h": h}
    k["gin"] = _sigmoid(h @ P["ig.weight"].T + P["ig.bias"])
    k["xin"] = k["gin"] * x
    k["pre_gi"], k["pre_gh"] = k["xin"] @ P["weight_ih"].T, h @ P["weight_hh"].T
    k["gi"], k["si"] = _rownorm(k["pre_gi"])
    k["gh"], k["sh"] = _rownorm(k["pre_gh"])
    ir, iz, i_n = np.split(k["gi"] + P["bias_ih"], 3, axis=1)
    hr, hz, h_n = np.split(k["gh"] + P["bias_hh"], 3, axis=1)
    r, z = _sigmoid(ir + hr), _sigmoid(iz + hz)
    n = np.tanh(i_n + r * h_n)
    k.update(r=r, z=z, n=n, h_n=h_n)
    return n + z * (h - n), k


def cell_bwd(P, k, dhy=None, dhy2=None):
    """{dx, dh, <parameter name>: gradient} for the upstream gradient dhy + dhy2 (None = zero)"""
    x, h = k["x"], k["h"]
    g = np.zeros_like(x)
    for d in (dhy, dhy2):
        if d is not None:
            g = g + np.asarray(d, dtype=np.float64)
    r, z, n = k["r"], k["z"], k["n"]
    dn_pre = g * (1.0 - z) * (1.0 - n * n)
    dz_pre = g * (h - n) * z * (1.0 - z)
    dr_pre = dn_pre * k["h_n"] * r * (1.0 - r)
    yi = np.concatenate([dr_pre, dz_pre, dn_pre], 1)               # gradient of gi + bih
    yh = np.concatenate([dr_pre, dz_pre, dn_pre * r], 1)           # gradient of gh + bhh
    dgi, dgh = _rownorm_bwd(yi, k["gi"], k["si"]), _rownorm_bwd(yh, k["gh"], k["sh"])
    dxin = dgi @ P["weight_ih"]
    gin = k["gin"]
    da = dxin * x * gin * (1.0 - gin)
    return {"dx": dxin * gin, "dh": g * z + dgh @ P["weight_hh"] + da @ P["ig.weight"],
            "weight_ih": dgi.T @ k["xin"], "weight_hh": dgh.T @ h, "bias_ih": yi.sum(0), "bias_hh": yh.sum(0),
            "ig.weight": da.T @ h, "ig.bias": da.sum(0)}


def recurrence(P, hx0, W, src, tgt, R, cat_all, gout=None):
    """R x { m_e = hx[src_e] @ W_e -> mean over the IN-edges of every node (0 for a node without) -> cell }, the output
    cat([hx_0 .. hx_R], 1) or hx_R.  W [E,C,C].  Returns out, and with ``gout`` (gradient of out) also
    {dhx, dW, <parameter name>: gradient}."""
    hx = np.asarray(hx0, dtype=np.float64)
    W = np.asarray(W, dtype=np.float64)
    S, C = hx.shape
    deg = np.maximum(np.bincount(tgt, minlength=S), 1).astype(np.float64)[:, None]
    hxs, caches = [hx], []
    for _ in range(R):
        inp = np.zeros_like(hx)
        np.add.at(inp, tgt, np.einsum("ea,eab->eb", hx[src], W))
        hx, k = cell_fwd(P, inp / deg, hx)
        caches.append(k)
        hxs.append(hx)
    out = np.concatenate(hxs, 1) if cat_all else hx
    if gout is None:
        return out
    gout = np.asarray(gout, dtype=np.float64)
    piece = (lambda i: gout[:, i * C:(i + 1) * C]) if cat_all else (lambda i: gout if i == R else 0.0)
    grads = {n: np.zeros_like(P[n]) for n in P}
    dW = np.zeros_like(W)
    dhx = piece(R) + np.zeros_like(hx)
    for i in range(R - 1, -1, -1):
        b = cell_bwd(P, caches[i], dhx)
        for n in P:
            grads[n] += b[n]
        prev = hxs[i]
        dmsg = (b["dx"] / deg)[tgt]
        dprev = np.zeros_like(prev)
        np.add.at(dprev, src, np.einsum("eb,eab->ea", dmsg, W))
        dW += prev[src][:, :, None] * dmsg[:, None, :]
        dhx = b["dh"] + dprev + piece(i)
    grads.update(dhx=dhx, dW=dW)
    return out, grads


# ---------------------------------------------------------------- the launch plan of csrc/gru.hip, restated
WF = 8                    # GRU_WF: rows (= waves) per workgroup of the forward, one weight staging each
WAVES, ROWS = 4, 3        # GRU_WAVES, rows per wave of the backward: 12 rows per workgroup = per parameter-gradient slab
MAX_WG = 256              # both launches: beyond it the waves stride over the rows
P_FLOATS = 2 * 96 * 32 + 32 * 32 + 2 * 96 + 32        # GRU_P: floats of a slab
RED_LANES, RED_DEPTH = 8, 16                          # gru_reduce_kernel: slab lanes, slabs in flight per lane and trip


def slabs(S, rows_per_wave=ROWS):
    """workgroups of the backward launch = slabs the reduce adds"""
    return min(MAX_WG, max(1, -(-S // (WAVES * rows_per_wave))))


def fwd_workgroups(S):
    return min(MAX_WG, max(1, -(-S // WF)))


def bwd_rows_per_wave(S, rows_per_wave=ROWS):
    """rows every wave of the backward launch walks, [slab][wave]: wave w of workgroup b takes the rows 4 b + w,
    4 b + w + 4 nb, ...  A wave with 0 rows is idle: its zero accumulators still enter the slab merge."""
    nb = slabs(S, rows_per_wave)
    return [[len(range(b * WAVES + w, S, nb * WAVES)) for w in range(WAVES)] for b in range(nb)]


def idle_bwd_waves(S, rows_per_wave=ROWS):
    return sum(n == 0 for wg in bwd_rows_per_wave(S, rows_per_wave) for n in wg)


def reduce_plan(nslab):
    """per slab lane of gru_reduce_kernel: (unrolled 16-slab trips, slabs of the tail loop)"""
    plan = []
    for sy in range(RED_LANES):
        k, trips = sy, 0
        while k + (RED_DEPTH - 1) * RED_LANES < nslab:
            k += RED_DEPTH * RED_LANES
            trips += 1
        plan.append((trips, len(range(k, nslab, RED_LANES))))
    return plan


# row count -> the slab count it is named for
ROW_COUNTS = {1: 1, 2: 1, 3: 1, 4: 1, 5: 1, 7: 1, 8: 1, 9: 1, 11: 1, 12: 1, 13: 2, 84: 7, 96: 8, 97: 9, 1488: 124,
              1536: 128, 1537: 129, 2048: 171, 2049: 171}


# ---------------------------------------------------------------- shared inputs
def make_cell(seed):
    import graphnet
    torch.manual_seed(seed)
    return graphnet.GRUCellEx(32, 32, bias=True, layernorm=True, ingate=True)


def make_rows(seed, S, n=4):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(S, 32, generator=g) for _ in range(n)]          # x, h, dhy, dhy2


HARD_ROWS = [0, 5, 13, 26]
HARD_S = 27
HARD_KINDS = ["x0", "h0", "x0h0", "tiny", "sat_bias", "ig_sat", "big_h"]
SAT_IH = {5: 30.0, 9: -30.0, 32 + 9: -100.0, 32 + 11: 30.0, 64 + 17: 30.0, 64 + 30: -30.0}
SAT_HH = {64 + 3: 40.0}


def hard_case(kind):
    """(cell, x, h, dhy) with the rows HARD_ROWS made hard in the way ``kind`` names (the bias cases change the cell:
    every row meets the saturated channels, beside the ordinary ones)"""
    cell = make_cell(77)
    x, h, dhy = make_rows(78, HARD_S, 3)
    r = HARD_ROWS
    with torch.no_grad():
        if kind in ("x0", "x0h0"):
            x[r] = 0.0
        if kind in ("h0", "x0h0"):
            h[r] = 0.0
        if kind == "tiny":
            x[r] *= 1e-4
            h[r] *= 1e-4
        elif kind == "sat_bias":
            for o, v in SAT_IH.items():
                cell.bias_ih[o] = v
            for o, v in SAT_HH.items():
                cell.bias_hh[o] = v
        elif kind == "ig_sat":
            cell.ig.bias[4] = -100.0
            cell.ig.bias[7] = 100.0
        elif kind == "big_h":
            h[r] = 50.0 * torch.sign(h[r])
        elif kind not in ("x0", "h0", "x0h0"):
            raise ValueError(kind)
    return cell, x, h, dhy


def check_hardness(kind, k):
    """the fp64 forward confirms that the rows are what the case names"""
    r = HARD_ROWS
    if kind in ("x0", "x0h0"):
        assert float(np.abs(k["pre_gi"][r]).max()) == 0.0 and float(np.abs(k["gi"][r]).max()) == 0.0
        assert np.allclose(k["si"][r], 1.0 / np.sqrt(1e-5), rtol=1e-14)
    if kind in ("h0", "x0h0"):
        assert float(np.abs(k["h"][r]).max()) == 0.0 and float(np.abs(k["pre_gh"][r]).max()) == 0.0
        assert np.allclose(k["sh"][r], 1.0 / np.sqrt(1e-5), rtol=1e-14)
    if kind == "tiny":
        for pre in ("pre_gi", "pre_gh"):
            assert float(k[pre][r].var(axis=1).max()) < EPS, "eps decides the norm of these rows"
            assert float(k[pre][r].var(axis=1).min()) > 0.0
    elif kind == "sat_bias":
        # the normalised pre-activations are O(1) (|.| <= sqrt(95) each): the biases decide these channels on EVERY row
        assert float(k["r"][:, 5].min()) > 1 - 1e-4 and float(k["r"][:, 9].max()) < 1e-4
        assert float(k["z"][:, 9].max()) < 1e-4 and float(k["z"][:, 11].min()) > 1 - 1e-4
        assert float(k["n"][:, 17].min()) > 1 - 1e-8 and float(k["n"][:, 30].max()) < -1 + 1e-8
        # bias_hh[64 + 3] = 40 reaches n only through r[3], an ordinary gate: r * 40 inside the tanh, 40 in d r
        assert float(k["h_n"][:, 3].min()) > 30.0
        assert 1e-3 < float(k["r"][:, 3].min()) and float(k["r"][:, 3].max()) < 1 - 1e-3
    elif kind == "ig_sat":
        assert float(k["gin"][:, 4].max()) < 1e-30 and float(k["gin"][:, 7].min()) == 1.0
    elif kind == "big_h":
        assert float(np.abs(k["h"][r]).min()) == 50.0 and float(np.abs(k["h"][r]).max()) == 50.0
