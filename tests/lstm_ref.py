"""fp64 numpy restatement of LSTMCellEx (forward and analytic backward) and of the R-repeat recurrent graph convolution
around it, for the value tests of the fused cell (tests/test_lstm_ref_host.py, tests/test_gpu_lstm_cell.py).  Written
from the formulas, not from the module code:

    xin = sigmoid(Wig h + big) * x                        (ingate; else xin = x)
    gi  = Wih xin + bih,  gh = Whh h + bhh                [4H] each, the biases inside the norm
    gi, gh = rownorm(gi), rownorm(gh)                     (layernorm) (v - mean) / sqrt(biased var + 1e-5) over a row
    i, f, g, o = chunk4(gi + gh);  i, f, o = sigmoid, g = tanh
    cy = f * c + i * g,  hy = o * tanh(cy)

Parameters travel as a dict of float64 arrays under the module's names: weight_ih [4H,C], weight_hh [4H,H], bias_ih,
bias_hh [4H], ig.weight [C,H], ig.bias [C]."""
import numpy as np

EPS = 1e-5
NAMES = ("weight_ih", "weight_hh", "bias_ih", "bias_hh", "ig.weight", "ig.bias")


def params_of(cell):
    """{name: float64 array} of a torch cell"""
    return {n: p.detach().cpu().double().numpy() for n, p in cell.named_parameters()}


def _sigmoid(v):
    return 0.5 * (1.0 + np.tanh(0.5 * v))          # (no overflow at either end)


def _rownorm(v):
    mu = v.mean(1, keepdims=True)
    d = v - mu
    s = 1.0 / np.sqrt((d * d).mean(1, keepdims=True) + EPS)
    return d * s, s


def _rownorm_bwd(dy, yhat, s):
    return (dy - dy.mean(1, keepdims=True) - yhat * (dy * yhat).mean(1, keepdims=True)) * s


def cell_fwd(P, x, h, c, layernorm=True, ingate=True):
    """(hy, cy, cache)"""
    x, h, c = (np.asarray(a, dtype=np.float64) for a in (x, h, c))
    k = {"x": x, "h": h, "c": c, "layernorm": layernorm, "ingate": ingate}
    if ingate:
        k["gin"] = _sigmoid(h @ P["ig.weight"].T + P["ig.bias"])
        xin = k["gin"] * x
    else:
        xin = x
    k["xin"] = xin
    gi = xin @ P["weight_ih"].T + P["bias_ih"]
    gh = h @ P["weight_hh"].T + P["bias_hh"]
    k["pre_gi"], k["pre_gh"] = gi, gh
    if layernorm:
        gi, k["si"] = _rownorm(gi)
        gh, k["sh"] = _rownorm(gh)
    k["gi"], k["gh"] = gi, gh
    pi, pf, pg, po = np.split(gi + gh, 4, axis=1)
    i, f, g, o = _sigmoid(pi), _sigmoid(pf), np.tanh(pg), _sigmoid(po)
    cy = f * c + i * g
    tc = np.tanh(cy)
    k.update(i=i, f=f, g=g, o=o, tc=tc, pre_cy=cy)
    return o * tc, cy, k


def cell_bwd(P, k, dhy=None, dcy=None):
    """{dx, dh, dc, <parameter name>: gradient} for the upstream gradients (None = zero)"""
    x, h, c = k["x"], k["h"], k["c"]
    dhy = np.zeros_like(x) if dhy is None else np.asarray(dhy, dtype=np.float64)
    dcy = np.zeros_like(x) if dcy is None else np.asarray(dcy, dtype=np.float64)
    i, f, g, o, tc = k["i"], k["f"], k["g"], k["o"], k["tc"]
    dct = dcy + dhy * o * (1.0 - tc * tc)
    dp = np.concatenate([dct * g * i * (1.0 - i), dct * c * f * (1.0 - f), dct * i * (1.0 - g * g),
                         dhy * tc * o * (1.0 - o)], 1)
    if k["layernorm"]:
        dgi, dgh = _rownorm_bwd(dp, k["gi"], k["si"]), _rownorm_bwd(dp, k["gh"], k["sh"])
    else:
        dgi = dgh = dp
    out = {"dc": dct * f, "bias_ih": dgi.sum(0), "bias_hh": dgh.sum(0), "weight_ih": dgi.T @ k["xin"],
           "weight_hh": dgh.T @ h}
    dxin = dgi @ P["weight_ih"]
    dh = dgh @ P["weight_hh"]
    if k["ingate"]:
        gin = k["gin"]
        da = dxin * x * gin * (1.0 - gin)
        out["ig.weight"], out["ig.bias"] = da.T @ h, da.sum(0)
        dh = dh + da @ P["ig.weight"]
        out["dx"] = dxin * gin
    else:
        out["dx"] = dxin
    out["dh"] = dh
    return out


def recurrence(P, hx0, W, src, tgt, R, cat_all, gout=None, layernorm=True, ingate=True):
    """R x { m_e = hx[src_e] @ W_e -> mean over the in-edges of every node (0 for a node without) -> cell }, cx from zeros,
    only the hx concatenated.  W [E,C,C] (or [E,C]: elementwise).  Returns out, and with ``gout`` (gradient of out) also
    {dhx, dW, <parameter name>: gradient}."""
    hx = np.asarray(hx0, dtype=np.float64)
    W = np.asarray(W, dtype=np.float64)
    S = hx.shape[0]
    deg = np.maximum(np.bincount(tgt, minlength=S), 1).astype(np.float64)[:, None]
    cx = np.zeros_like(hx)
    hxs, caches = [hx], []

    def messages(v):
        return np.einsum("ea,eab->eb", v[src], W) if W.ndim == 3 else v[src] * W

    for _ in range(R):
        inp = np.zeros_like(hx)
        np.add.at(inp, tgt, messages(hx))
        hx, cx, k = cell_fwd(P, inp / deg, hx, cx, layernorm, ingate)
        caches.append(k)
        hxs.append(hx)
    out = np.concatenate(hxs, 1) if cat_all else hx
    if gout is None:
        return out
    gout = np.asarray(gout, dtype=np.float64)
    C = hx.shape[1]
    piece = (lambda r: gout[:, r * C:(r + 1) * C]) if cat_all else (lambda r: gout if r == R else 0.0)
    grads = {n: np.zeros_like(P[n]) for n in P}
    dW = np.zeros_like(W)
    dhx, dcx = piece(R) + np.zeros_like(hx), None
    for r in range(R - 1, -1, -1):
        b = cell_bwd(P, caches[r], dhx, dcx)
        for n in P:
            grads[n] += b[n]
        prev = hxs[r]
        dmsg = (b["dx"] / deg)[tgt]
        dprev = np.zeros_like(prev)
        if W.ndim == 3:
            np.add.at(dprev, src, np.einsum("eb,eab->ea", dmsg, W))
            dW += prev[src][:, :, None] * dmsg[:, None, :]
        else:
            np.add.at(dprev, src, dmsg * W)
            dW += prev[src] * dmsg
        dhx, dcx = b["dh"] + dprev + piece(r), b["dc"]
    grads.update(dhx=dhx, dW=dW)
    return out, grads
