"""Plain fp64 reference of BatchNorm1d(+ReLU) as csrc/bn.hip computes it, and the hard inputs its tests run on: CPU torch /
numpy in float64, written from the formulas (torch.nn.BatchNorm1d; Chan's combination of centred slice partials) and not
from the kernels.  tests/test_bn_ref_host.py checks this file against torch autograd and checks every generator.

Reference.  ``stats`` / ``forward`` / ``backward`` take the fp32 input exactly as stored and work in fp64.
``slice_partials`` / ``bwd_slice_partials`` give the [n_part, 2, C] fp32 tensors of the centred-partials path (one row per
32-row slice; computed in fp64, rounded once); ``finish_from_partials`` is the finish of that path evaluated EXACTLY (rational
arithmetic) on those fp32 partials, so that a finish kernel can be held to its own rounding alone.

Generators.  Each is seeded and returns a ``Case`` (fp32 x, fp32 gamma / beta or None, per-channel notes):
  offset(ratio)       |mean| / sigma of channel c is {0, 30, ratio}[c % 3], the sign alternates every three channels; the
                      columns are standardised, so the ratio is met exactly before the fp32 rounding; the first 8 rows (the
                      pivot of bn.hip) are rows like any other
  displaced_pivot(d)  the mean of the first 8 rows lies d sigma off the channel mean (both signs), d <= PIVOT_LIMIT = 8: the
                      pivot design of bn.hip promises a pivot "within a few sigma" of the mean, sum (x - K)^2 is then
                      (1 + d^2) times the centred sum, 65 at the limit.  Nothing here puts the pivot further off than 8 sigma
                      (a pivot 1000 sigma off is outside what the design claims); needs M >= 1023 rows
  degenerate          channel c is of kind KINDS[c % len(KINDS)]: constant with a short mantissa (variance exactly 0),
                      constant with a full 24-bit mantissa, sigma 1e-4 around 1 (variance 1e-8, far below eps), zeros with
                      one row of 1e4, gamma = 0, gamma = beta = 0 (pre-activation exactly 0, mask closed), beta = -2.326
                      (about 1 % of the rows open), and a plain channel
  dy_scaled           standard normal rows scaled by 10^u, u uniform in [-3, 3]

ReLU margin.  A mask that differs between fp32 and fp64 changes dgamma by a whole dy * xhat, so every generator guarantees
that the fp64 pre-activation z = gamma * xhat + beta of EVERY element is either exactly 0 by construction (gamma = beta = 0;
a single row, whose xhat is 0, with beta = 0) or has |z| >= MARGIN = 1e-3: elements inside the margin are moved out of it
along x and the statistics re-evaluated until none is left (``ensure_margin``).  No element is excluded from any
comparison: the share of excluded elements is zero.  In evaluation mode the margin is taken with the running statistics
the case is run with (``stats=``)."""
import math
from fractions import Fraction

import numpy as np
import torch

EPS = 1e-4
MARGIN = 1e-3
PIVOT_LIMIT = 8.0
KINDS = ("const_short", "const_full", "tiny_sigma", "spike", "gamma0", "gamma0_beta0", "beta_masks", "plain")
# kinds whose z does not depend on x in a way a nudge could use (or whose x must stay as it is): z is beta, 0, or fixed
_FROZEN = ("const_short", "const_full", "spike", "gamma0", "gamma0_beta0")


def f64(t):
    """detached fp64 CPU copy (None stays None)"""
    return None if t is None else torch.as_tensor(t).detach().cpu().double().clone()


# ---------------------------------------------------------------- reference

def stats(x):
    """(mean, biased variance, unbiased variance) per channel, fp64; the unbiased one equals the biased one for one row"""
    x = f64(x)
    M = x.shape[0]
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    return mean, var, var * (M / (M - 1.0)) if M > 1 else var.clone()


def running(old_mean, old_var, x, momentum):
    """the running statistics after one training step: (1 - m) old + m new, the variance unbiased (n / (n - 1), n > 1)"""
    mean, _, unb = stats(x)
    return (1.0 - momentum) * f64(old_mean) + momentum * mean, (1.0 - momentum) * f64(old_var) + momentum * unb


def _affine(C, gamma, beta):
    return (torch.ones(C, dtype=torch.float64) if gamma is None else f64(gamma),
            torch.zeros(C, dtype=torch.float64) if beta is None else f64(beta))


def pre_activation(x, mean, var, gamma, beta, eps):
    x = f64(x)
    g, b = _affine(x.shape[1], gamma, beta)
    return (x - f64(mean)) / torch.sqrt(f64(var) + eps) * g + b


def forward(x, mean, var, gamma, beta, eps, relu):
    z = pre_activation(x, mean, var, gamma, beta, eps)
    return torch.clamp_min(z, 0.0) if relu else z


def backward(x, dy, gamma, beta, eps, relu, training, addend=None, mean=None, var=None):
    """(dx, dgamma, dbeta) in closed form.  training: batch statistics of x, dx = gamma rstd (dz - dbeta / M - xhat dgamma / M);
    evaluation: the given mean / var, dx = gamma rstd dz.  dz = dy where z > 0 (relu) or dy.  ``addend`` is added to dx."""
    x, dy = f64(x), f64(dy)
    M, C = x.shape
    if training:
        mean, var, _ = stats(x)
    mean, var = f64(mean), f64(var)
    g, b = _affine(C, gamma, beta)
    rstd = 1.0 / torch.sqrt(var + eps)
    xh = (x - mean) * rstd
    dz = torch.where(xh * g + b > 0, dy, torch.zeros_like(dy)) if relu else dy
    dbeta, dgamma = dz.sum(0), (dz * xh).sum(0)
    dx = g * rstd * ((dz - dbeta / M - xh * dgamma / M) if training else dz)
    if addend is not None:
        dx = dx + f64(addend)
    return dx, dgamma, dbeta


def _slices(t):
    """[M, C] -> ([n_part, 32, C] zero-padded, rows per slice [n_part])"""
    M, C = t.shape
    n_part = (M + 31) // 32
    pad = n_part * 32 - M
    tp = torch.cat([t, torch.zeros(pad, C, dtype=t.dtype)]) if pad else t
    cnt = torch.full((n_part,), 32.0, dtype=torch.float64)
    cnt[-1] = 32 - pad
    return tp.view(n_part, 32, C), cnt


def slice_partials(x):
    """[n_part, 2, C] fp32: per 32-row slice (the last one shorter) the sum and the sum of squared deviations from the
    slice's OWN mean -- what the convolution epilogues hand to wsis_bn_stats_finalize"""
    x = f64(x)
    M = x.shape[0]
    blocks, cnt = _slices(x)
    s = blocks.sum(1)
    live = (torch.arange(blocks.shape[0] * 32) < M).view(-1, 32, 1)
    dev = torch.where(live, blocks - (s / cnt.unsqueeze(1)).unsqueeze(1), torch.zeros_like(blocks))
    return torch.stack([s, (dev * dev).sum(1)], 1).float().contiguous()


def bwd_slice_partials(x, dy, mean, var, gamma, beta, eps, relu):
    """[n_part, 2, C] fp32: per 32-row slice (sum dz, sum dz * xhat) -- what the dIn epilogue hands to
    wsis_bn_bwd_from_partials"""
    x, dy = f64(x), f64(dy)
    g, b = _affine(x.shape[1], gamma, beta)
    xh = (x - f64(mean)) / torch.sqrt(f64(var) + eps)
    dz = torch.where(xh * g + b > 0, dy, torch.zeros_like(dy)) if relu else dy
    return torch.stack([_slices(dz)[0].sum(1), _slices(dz * xh)[0].sum(1)], 1).float().contiguous()


def finish_from_partials(partials, M):
    """mean = sum S_i / M, var = (sum Q_i + sum S_i^2 / n_i - M mean^2) / M on the fp32 partials, evaluated exactly and
    rounded once to fp64.  Returns (mean, biased var, unbiased var, mass): ``mass`` = (sum Q_i + sum S_i^2 / n_i + M mean^2)
    / M is the size of the terms that cancel in var -- fp64 arithmetic in any order is within (its number of roundings) x
    2^-53 x mass of the exact value."""
    p = partials.detach().cpu().double().numpy()
    n_part, _, C = p.shape
    assert n_part == (M + 31) // 32
    left = [min(32, M - 32 * i) for i in range(n_part)]
    out = np.zeros((4, C))
    for c in range(C):
        S = sum((Fraction(float(v)) for v in p[:, 0, c]), Fraction(0))
        Q = sum((Fraction(float(v)) for v in p[:, 1, c]), Fraction(0))
        W = sum((Fraction(float(v)) ** 2 / n for v, n in zip(p[:, 0, c], left)), Fraction(0))
        mu = S / M
        var = max((Q + W - M * mu * mu) / M, Fraction(0))
        out[:, c] = (float(mu), float(var), float(var * M / (M - 1)) if M > 1 else float(var),
                     float((abs(Q) + W + M * mu * mu) / M))
    return tuple(torch.from_numpy(out[i].copy()) for i in range(4))


def sum_partials(partials):
    """(sum of [:, 0], sum of [:, 1], sum of |[:, 0]|, sum of |[:, 1]|) per channel, the sums exact and rounded once"""
    p = partials.detach().cpu().double().numpy()
    C = p.shape[2]
    cols = lambda a: torch.tensor([math.fsum(a[:, c]) for c in range(C)], dtype=torch.float64)
    return cols(p[:, 0]), cols(p[:, 1]), cols(np.abs(p[:, 0])), cols(np.abs(p[:, 1]))


def ulp32(t):
    """spacing of fp32 at |t| (fp64 tensor in, fp64 out; the smallest normal's spacing below it)"""
    _, e = torch.frexp(f64(t).abs().clamp_min(2.0 ** -126))      # |t| = m 2^e, 0.5 <= m < 1
    return torch.exp2(e.double() - 24)


# ---------------------------------------------------------------- generators

class Case:
    """x [M, C] fp32, gamma / beta [C] fp32 or None, eps; ``ratio`` (claimed |mean| / sigma), ``kinds``, ``nudged`` (the
    number of elements ensure_margin moved), ``exact_zero`` (bool [C]: z is exactly 0 by construction)"""

    def __init__(self, x, gamma, beta, **notes):
        self.x, self.gamma, self.beta, self.eps = x, gamma, beta, EPS
        self.ratio = self.kinds = self.displacement = None
        self.nudged = 0
        self.__dict__.update(notes)
        self.M, self.C = x.shape


def _standard(rng, M, C):
    """standard normal columns; with two rows or more: sample mean exactly 0 and biased sample sigma exactly 1 (fp64)"""
    u = rng.standard_normal((M, C))
    if M >= 2:
        u = (u - u.mean(0)) / u.std(0)
    return u


def _gamma_beta(rng, C, affine):
    if not affine:
        return None, None
    gamma = rng.uniform(0.5, 1.5, C) * np.where(np.arange(C) % 5 == 4, -1.0, 1.0)      # every fifth scale negative
    return gamma, rng.standard_normal(C) * 0.3


def ensure_margin(x, gamma, beta, eps=EPS, stats_given=None, frozen=None, both=True):
    """fp32 x whose fp64 pre-activation has |z| >= MARGIN at every element of the channels not ``frozen`` (bool [C]): the
    elements inside the margin are moved to |z| = 2 MARGIN on their own side (z = 0: the open side), the statistics (batch
    statistics of the fp32 x, or ``stats_given`` = (mean, var)) re-evaluated, until none is left.  With ``both`` and two
    rows or more, a channel whose mask is all open or all closed first has its beta set to 0.  Returns (x, beta, nudged)."""
    x = torch.as_tensor(np.asarray(x, dtype=np.float32)).clone()
    M, C = x.shape
    g = None if gamma is None else torch.as_tensor(np.asarray(gamma, dtype=np.float32))
    b = None if beta is None else torch.as_tensor(np.asarray(beta, dtype=np.float32)).clone()
    free = torch.ones(C, dtype=torch.bool) if frozen is None else ~torch.as_tensor(frozen)
    moved = torch.zeros(M, C, dtype=torch.bool)

    def z_now():
        mean, var = stats(x)[:2] if stats_given is None else stats_given
        return pre_activation(x, mean, var, g, b, eps), torch.sqrt(f64(var) + eps)

    z = None
    if both and M >= 2 and b is not None:
        z, std = z_now()
        one_sided = ((z > 0).all(0) | (z <= 0).all(0)) & free
        if bool(one_sided.any()):
            b[one_sided] = 0.0
            z = None
    for _ in range(200):
        if z is None:
            z, std = z_now()
        bad = (z.abs() < MARGIN) & free
        if M == 1 and stats_given is None:          # one row: xhat = 0 whatever x is, z = beta
            assert not bool((bad & (z != 0)).any()), "a single row needs |beta| >= MARGIN or beta == 0"
            break
        if not bool(bad.any()):
            break
        gd = _affine(C, g, b)[0]
        side = torch.where(z >= 0, 1.0, -1.0)
        step = side * (2.0 * MARGIN - z.abs()) * std / gd          # along x: dz / dx = gamma / std
        x = torch.where(bad, (x.double() + step).float(), x)
        moved |= bad
        z = None
    else:
        raise AssertionError("the ReLU margin was not reached")
    assert bool(((z.abs() >= MARGIN) | (z == 0)).all()), "a frozen channel lies inside the ReLU margin"
    return x, b, int(moved.sum())


def offset(M, C, ratio, seed, affine=True, stats_given=None):
    """|mean| / sigma = {0, 30, ratio}[c % 3] with the sign (-1)^(c // 3); sigma = 2^u, u uniform in [-1, 1]"""
    assert 0 <= ratio <= 1000
    rng = np.random.default_rng(seed)
    u = _standard(rng, M, C)
    sigma = 2.0 ** rng.uniform(-1, 1, C)
    r = np.array([0.0, 30.0, float(ratio)])[np.arange(C) % 3] * np.where((np.arange(C) // 3) % 2 == 0, 1.0, -1.0)
    gamma, beta = _gamma_beta(rng, C, affine)
    if M == 1 and beta is not None:
        beta = np.where(np.abs(beta) < 2 * MARGIN, 2 * MARGIN, beta)
    x, beta, n = ensure_margin(sigma * (u + r), gamma, beta, stats_given=stats_given)
    return Case(x, _t32(gamma), beta, ratio=torch.from_numpy(np.abs(r)), nudged=n,
                exact_zero=torch.zeros(C, dtype=torch.bool))


def displaced_pivot(M, C, d, seed):
    """the first 8 rows are a cluster whose mean is d sigma (of the whole channel) off the channel mean, the sign
    (-1)^(c // 2); channel means {0, 30}[c % 2] sigma.  d is reached from below by bisection: 0.99 d <= displacement <= d"""
    assert 0 < d <= PIVOT_LIMIT and M >= 1023
    rng = np.random.default_rng(seed)
    u = _standard(rng, M, C)
    sign = np.where((np.arange(C) // 2) % 2 == 0, 1.0, -1.0)

    def place(off):
        v = u.copy()
        v[:8] = 0.25 * u[:8] + off * sign
        v = (v - v.mean(0)) / v.std(0)
        return v, np.abs(v[:8].mean(0))

    lo, hi = np.zeros(C), np.full(C, 64.0)
    for _ in range(32):
        mid = 0.5 * (lo + hi)
        under = place(mid)[1] <= 0.998 * d
        lo, hi = np.where(under, mid, lo), np.where(under, hi, mid)
    v, disp = place(lo)
    sigma = 2.0 ** rng.uniform(-1, 1, C)
    r = np.array([0.0, 30.0])[np.arange(C) % 2]
    gamma, beta = _gamma_beta(rng, C, True)
    x, beta, n = ensure_margin(sigma * (v + r), gamma, beta)
    return Case(x, _t32(gamma), beta, ratio=torch.from_numpy(r), displacement=torch.from_numpy(disp), nudged=n,
                exact_zero=torch.zeros(C, dtype=torch.bool))


def degenerate(M, C, seed):
    """channel c of kind KINDS[c % 8] (module docstring); needs M >= 64 so that 1 % of the rows is a row"""
    assert M >= 64
    rng = np.random.default_rng(seed)
    x = _standard(rng, M, C) * 2.0 ** rng.uniform(-1, 1, C) + rng.standard_normal(C)
    gamma, beta = _gamma_beta(rng, C, True)
    beta = np.where(np.abs(beta) < 0.05, 0.05, beta)              # (frozen channels have z = beta)
    kinds = [KINDS[c % len(KINDS)] for c in range(C)]
    for c, kind in enumerate(kinds):
        if kind == "const_short":
            x[:, c] = 1.5 * (1 + c % 3)                            # 1.5, 3, 4.5: a few mantissa bits
        elif kind == "const_full":
            bits = np.float32(1.2345678 + 0.37 * c).view(np.uint32) | np.uint32(1)      # lowest mantissa bit set
            x[:, c] = float(bits.view(np.float32))
        elif kind == "tiny_sigma":
            x[:, c] = 1.0 + 1e-4 * _standard(rng, M, 1)[:, 0]
            beta[c] = 0.0
        elif kind == "spike":
            x[:, c] = 0.0
            x[int(rng.integers(0, M)), c] = 1e4
            gamma[c], beta[c] = abs(gamma[c]), 0.3                 # zero rows: z = 0.3 - gamma / sqrt(M - 1) > 0
        elif kind == "gamma0":
            gamma[c] = 0.0
        elif kind == "gamma0_beta0":
            gamma[c], beta[c] = 0.0, 0.0
        elif kind == "beta_masks":
            gamma[c], beta[c] = 1.0, -2.326                        # z > 0 where xhat > 2.326: 1 % of a normal sample
    frozen = torch.tensor([k in _FROZEN for k in kinds])
    # beta_masks keeps its beta (its mask is meant to be nearly closed); the other free channels get both sides
    x, beta, n = ensure_margin(x, gamma, beta, frozen=frozen, both=False)
    return Case(x, _t32(gamma), beta, kinds=kinds, nudged=n,
                exact_zero=torch.tensor([k == "gamma0_beta0" for k in kinds]))


def dy_scaled(M, C, seed):
    """standard normal gradient rows, row r scaled by 10^u_r, u uniform in [-3, 3]: scales from 1e-3 to 1e3"""
    rng = np.random.default_rng(seed)
    scale = 10.0 ** rng.uniform(-3, 3, (M, 1))
    if M >= 2:
        scale[0], scale[-1] = 1e-3, 1e3
    return torch.from_numpy((rng.standard_normal((M, C)) * scale).astype(np.float32))


def _t32(a):
    return None if a is None else torch.as_tensor(np.asarray(a, dtype=np.float32))


# ---------------------------------------------------------------- the parameter sets of tests/test_gpu_bn_edges.py
# (kind, M, C, p, affine, evaluation): tests/test_bn_ref_host.py checks every one of them, ``case`` builds no other

ROWS = (1, 2, 7, 8, 9, 1023, 1024, 1025, 4095, 4096, 4097)            # around the one-launch kernels (M <= 4096)
LAYOUT_C = (4, 32, 96, 160, 260, 516, 1024, 1, 3, 5, 21, 33, 70)      # thread layouts of the two-launch kernels
LAYOUT_M = (333, 4101)                                                # 4101: no multiple of any bn_rows_per_wg(C)
NBLK_M = {17: 4196, 64: 16384, 65: 16385, 129: 33000}                 # C = 32: 256 rows per workgroup
MODE_SHAPES = ((1025, 33), (4101, 32))
GEN_SHAPES = ((1025, 32), (4500, 33))                                 # one-launch / two-launch (stand-alone path)
CENTRED_GEN_SHAPES = ((1025, 33), (4799, 32))                         # G = 1 / 2 (n_part = 33, 150)
RATIOS = (100, 300, 1000)                                             # (every offset case has channels at 0 and 30 as well)
DISPLACEMENTS = (1, 4, 8)
ISOLATION_SHAPES = ((1025, 33), (4500, 96))
# n_part at every edge of bn_fin_chunks (G = n_part / 64 capped at 64) -> (C, remainders M % 32 of the last slice)
CENTRED_EDGES = {1: (32, (0, 1, 31)), 2: (33, (0, 1, 31)), 127: (96, (31,)), 128: (32, (0, 1, 31)), 129: (33, (1,)),
                 191: (96, (0,)), 192: (32, (31,)), 4095: (4, (31,)), 4096: (4, (0,)), 4097: (4, (1,))}


def layout_shapes():
    """every layout at 4101 rows; the one-launch kernels (333 rows) where their loads are scalar (C = 32 is in ROWS)"""
    return [(C, M) for C in LAYOUT_C for M in LAYOUT_M if M > 4096 or C % 4]


def centred_rows(n_part, rem):
    return 32 * (n_part - 1) + (rem if rem else 32)


def gpu_cases():
    out = []
    for M in ROWS:
        out += [("offset", M, 32, 1000, True, False), ("offset", M, 32, 1000, True, True)]
    out += [("offset", M, C, 1000, True, False) for C, M in layout_shapes()]
    out += [("offset", M, 32, 1000, True, False) for M in NBLK_M.values()]
    out += [("offset", M, C, 300, affine, ev) for M, C in MODE_SHAPES for affine in (True, False) for ev in (False, True)]
    for M, C in GEN_SHAPES + CENTRED_GEN_SHAPES:
        out += [("offset", M, C, r, True, False) for r in RATIOS]
        out += [("displaced_pivot", M, C, d, True, False) for d in DISPLACEMENTS]
        out += [("degenerate", M, C, None, True, False)]
    out += [("offset", M, C, 30, True, False) for M, C in ISOLATION_SHAPES]
    for n_part, (C, rems) in CENTRED_EDGES.items():
        out += [("offset", centred_rows(n_part, rem), C, 1000, True, False) for rem in rems]
    return list(dict.fromkeys(out))


_CASES = {}


def case(kind, M, C, p=None, affine=True, evaluation=False):
    """the Case of one registered parameter set, built once per process (callers must not write to its tensors).  An
    evaluation case carries running statistics ``rm`` / ``rv`` (fp32) near the batch statistics and has its ReLU margin
    taken with them."""
    key = (kind, M, C, p, affine, evaluation)
    assert key in set(gpu_cases()), key
    if key not in _CASES:
        seed = 1000003 * M + 1009 * C + 7 * int(p or 0) + 2 * int(affine) + int(evaluation)
        if kind == "offset":
            given = None
            if evaluation:
                base = offset(M, C, p, seed, affine)
                rng = np.random.default_rng(seed + 1)
                mean, var, _ = stats(base.x)
                sd = torch.sqrt(var) if M > 1 else torch.ones(C, dtype=torch.float64)
                rm = (mean + 0.1 * sd * torch.from_numpy(rng.standard_normal(C))).float()
                rv = ((var if M > 1 else sd) * torch.from_numpy(rng.uniform(0.8, 1.25, C))).float()
                given = (rm.double(), rv.double())
            c = offset(M, C, p, seed, affine, stats_given=given)
            if evaluation:
                c.rm, c.rv = rm, rv
        elif kind == "displaced_pivot":
            c = displaced_pivot(M, C, p, seed)
        else:
            c = degenerate(M, C, seed)
        _CASES[key] = c
    return _CASES[key]
