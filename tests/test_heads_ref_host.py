"""tests/heads_ref.py against torch autograd in float64, every generator against its own promises, the drop condition on
the reference alone at every case tests/test_gpu_heads_edges.py runs, and wsis_heads_workspace_bytes against the layout
wsis_heads_fwd / wsis_heads_bwd carve out of the workspace.  No GPU."""
import numpy as np
import pytest
import torch

import heads_ref as ref
import wsis_native as _n


def _agree(a, b, tol=1e-12):
    assert set(a) == set(b), set(a) ^ set(b)
    for name, w in b.items():
        scale = max(float(w.abs().max()), 1.0)
        err = float((a[name].double() - w).abs().max())
        assert err <= tol * scale, (name, err, scale)


# ---- the reference against autograd ------------------------------------------------------------------------------
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("S", [2, 33, 700])
def test_reference_matches_autograd_in_float64(S, training):
    """plain chains in float64: tracked and untracked statistics (head 2 in training), a second Linear with and without
    bias (head 1), eps / momentum other than the defaults"""
    c = ref.plain(S, 4, 2, variant=3, seed=5, eps=1e-3, momentum=0.3, training=training)
    assert c.heads[1].b2 is None and c.heads[0].b2 is not None
    assert (c.heads[2].rm is None) == training and c.heads[0].rm is not None
    _agree(ref.evaluate(c), ref.chain(c, torch.float64))


def test_reference_matches_autograd_on_hard_columns():
    c = ref.hard(257, 5, 1, variant=1, seed=2, eps=1e-5, momentum=1.0)
    want = ref.evaluate(c)
    got = ref.chain(c, torch.float64)
    # the bias in front of a training-mode BatchNorm: true gradient 0, both sides hold rounding noise of the dW1 scale
    for p in range(5):
        for d in (want, got):
            assert float(d[f"db1.{p}"].abs().max()) <= 1e-9 * float(want[f"dW1.{p}"].abs().max())
            d[f"db1.{p}"] = torch.zeros(64, dtype=torch.float64)
    _agree(want, got, 1e-9)       # rstd up to 316 on the constant columns amplifies the fp64 rounding of both sides


def test_none_output_gradient_contributes_zeros():
    c = ref.plain(100, 3, 2, seed=9)
    c.dys[1] = None
    c.dys[4] = None
    want = ref.evaluate(c)
    _agree(want, ref.chain(c, torch.float64))
    for name in ("dW1.1", "dgamma.1", "dbeta.1", "dW2.1", "dW1.4"):
        assert float(want[name].abs().max()) == 0.0
    assert float(want["rm.1"].abs().max()) > 0.0       # the statistics are updated all the same


def test_lattice_rstd_without_eps_is_what_fp32_computes():
    """the lattice reference uses rstd = 1 / sqrt(var); torch in fp32 with eps = 2^-40 computes the same number, and the
    fp32 CPU module chain equals the exact result bit for bit"""
    for S, cfg in ((1, (4, 3)), (513, (8, 0)), (4097, (5, 3))):
        c = ref.case("lattice", cfg, S, variant=S % 8)
        want = ref.evaluate(c)
        got = ref.chain(c, torch.float32)
        for name, w in want.items():
            assert torch.equal(got[name].double(), w), (S, cfg, name)


def test_training_with_one_row_raises_like_the_modules():
    c = ref.plain(1, 2, 1, seed=1)
    with pytest.raises(ValueError):
        ref.evaluate(c)
    heads, _ = ref.modules(c)
    with pytest.raises(ValueError):
        heads[0](c.x)


# ---- the generators -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ref.EXACT_CONFIGS)
def test_lattice_promises(cfg):
    """integers, power-of-four variances, the 2^24 bound, exact zeros, both masks (asserted inside the generator too) at
    every row count; every cout in slot 0 and in a slot >= 4 over the variants"""
    slot0, high = set(), set()
    for i, S in enumerate(ref.ROWS):
        c = ref.case("lattice", cfg, S, variant=i % 8)
        assert not c.training and c.eps == 2.0 ** -40
        for t in [c.x] + [d for d in c.dys if d is not None]:
            assert torch.equal(t, t.round()) and float(t.abs().max()) <= 2
        for p, hd in enumerate(c.heads):
            for t in (hd.W1, hd.b1, hd.gamma, hd.beta, hd.rm, hd.W2):
                assert torch.equal(t, t.round())
            assert set(hd.rv.tolist()) <= {0.25, 1.0, 4.0, 16.0}
            assert (hd.b2 is None) == (p in (1, 5))
            (slot0 if p == 0 else high if p >= 4 else set()).add(hd.cout)
        assert c.worst / ref.GRAIN < 2.0 ** 24
        if c.heads:
            assert c.zeros >= 0.01 * c.total
    if cfg[0] >= 5:
        assert slot0 == set(ref.COUTS) and high == set(ref.COUTS)
    assert set(ref.COUTS) == {1, 3, 15, 16, 17, 20, 31, 32}


def test_every_cout_occurs_in_slot_0_and_above_3_in_the_training_cases():
    assert {ref.couts(8, v)[0] for v in range(8)} == set(ref.COUTS)
    assert {c for v in range(8) for c in ref.couts(8, v)[4:]} == set(ref.COUTS)


@pytest.mark.parametrize("S", [2, 33, 513])
def test_hard_generator_promises(S):
    c = ref.hard(S, 5, 3, variant=2, seed=4)
    _, cache, _ = ref.forward(c)
    for p, hd in enumerate(c.heads):
        z, h = cache[p]["z"], cache[p]["h"]
        assert bool(((z.abs() >= ref.MARGIN) | (z == 0)).all())
        mean, var, _ = ref.batch_stats(h)
        sd = var.sqrt()
        kinds = c.kinds[p]
        assert kinds[:8] == list(ref.KINDS)
        for col, kind in enumerate(kinds):
            zc = z[:, col]
            if kind == "offset100":
                assert float(mean[col].abs() / sd[col]) > 50
            elif kind == "const":
                assert float(var[col]) == 0.0 and bool((h[:, col] == 0.5).all())
                assert bool((zc == float(hd.beta[col])).all()) and (float(hd.beta[col]) == 0.0) == bool(c.exact_zero[p][col])
            elif kind == "tiny_sigma":
                assert 0 < float(sd[col]) < 1e-2
            elif kind == "dead":
                assert bool((zc < 0).all())
            elif kind == "gamma0":
                assert float(hd.gamma[col]) == 0.0 and bool((zc == float(hd.beta[col])).all())
            elif kind == "all_open":
                assert bool((zc > 0).all())
            elif kind == "neg_gamma":
                assert float(hd.gamma[col]) < 0
        assert bool((z == 0).any())                      # exact zeros present: the mask is z > 0
    assert c.heads[2].rm is None and c.heads[1].b2 is None and c.heads[0].rm is not None


def test_registered_cases_cover_eps_and_momentum_with_both_generators():
    cases = ref.train_cases()
    for gen in ("hard", "plain"):
        assert {(e, m) for g, _, _, e, m in cases if g == gen} == {(1e-4, 0.1), (1e-4, 1.0), (1e-5, 0.1), (1e-5, 1.0)}
    assert {(cfg, S) for _, cfg, S, _, _ in cases} == \
        {(c, S) for S in (2, 33, 512, 513, 4096, 4097) for c in ((4, 3), (5, 3))} | {((1, 0), 4097), ((8, 0), 4097)}


# ---- the drop condition on the reference alone -------------------------------------------------------------------
def _drop_visible(key):
    c = ref.case(*key)
    want, drops, _, _ = ref.references(*key)
    floor = ref.floors(c, want)
    assert len(drops) == len(ref.drop_rows(c.S))
    for d in drops:
        for name, w in want.items():
            if name in floor:
                continue
            gap = float((d[name] - w).abs().max())
            assert gap > ref.FLOOR * float(w.abs().max()), (key, name, gap, float(w.abs().max()))


@pytest.mark.parametrize("key", ref.train_cases(), ids=lambda k: "-".join(map(str, k)))
def test_one_dropped_row_is_visible_in_every_training_tensor(key):
    _drop_visible(key)


@pytest.mark.parametrize("cfg,S", ref.EVAL_CASES)
def test_one_dropped_row_is_visible_in_every_eval_tensor(cfg, S):
    c = ref.case("plain_eval", cfg, S)
    want = ref.evaluate(c)
    for r in ref.drop_rows(S):
        d = ref.evaluate(c, drop=r)
        for name, w in want.items():
            if ref.kind_of(name) in ("rm", "rv"):
                assert torch.equal(d[name], w)           # evaluation mode: the running statistics are inputs
                continue
            assert float((d[name] - w).abs().max()) > ref.FLOOR * float(w.abs().max()), (cfg, S, name)


def test_only_the_listed_tensors_get_more_than_four_times_the_cpu_chain_error():
    cases = {k[:3] for k in ref.train_cases()}
    assert set(ref.RAISED) <= cases and all(gen in ("plain", "hard") for gen, _, _ in ref.RAISED)
    assert sum(len(v) for v in ref.RAISED.values()) == 5 and all(f == 8.0 for v in ref.RAISED.values() for f in v.values())
    for key in [k for k in ref.train_cases() if k[2] <= 33] + [("plain_eval",) + c for c in ref.EVAL_CASES]:
        want, _, frac, cpu = ref.references(*key)
        raised = ref.RAISED.get(key[:3], {})
        assert set(raised) <= set(want)
        for name, f in frac.items():
            assert f == max((8.0 if name in raised else 4.0) * cpu[name], ref.FLOOR), (key, name)


def test_drop_rows():
    assert ref.drop_rows(1) == [0] and ref.drop_rows(4096) == [4095] and ref.drop_rows(4097) == [4096]
    assert ref.drop_rows(8225) == [8224, 4101] and 4101 // 32 == 128


# ---- the workspace ------------------------------------------------------------------------------------------------------
HB, W1P, W2P, MAX_PART = 8, 64 * 64 + 64, 32 * 64 + 32, 128


def _carved_bytes(S, n_heads, n_lin):
    """what the two entry points carve out: forward the statistics partials [n_slices][n_heads][2][64]; backward those,
    dZ [n_heads][S][64], the dW1 / db1 partials [n_part][blocks][64*64 + 64], the dW2 / db2 partials
    [n_part][n_heads][32*64 + 32] and the column means [n_heads][2][64], fp32 each, n_part = min(n_slices, 128)"""
    n_slices = (S + 31) // 32
    n_part = min(n_slices, MAX_PART)
    part = n_slices * n_heads * 2 * 64
    fwd = part
    bwd = part + n_heads * S * 64 + n_part * (n_heads + n_lin) * W1P + n_part * n_heads * W2P + n_heads * 2 * 64
    return 4 * max(fwd, bwd)


def test_workspace_covers_what_the_entry_points_carve():
    lib = _n.hip()
    assert _n.HEADS_MAX == HB
    for S in ref.ROWS + (2289, 5000):
        for nh, nl in ref.CONFIGS:
            got = lib.wsis_heads_workspace_bytes(S, nh, nl)
            assert got >= _carved_bytes(S, nh, nl), (S, nh, nl, got)
    for S in (0, -1):
        assert lib.wsis_heads_workspace_bytes(S, 4, 3) == -1
    for nh, nl in ((9, 0), (0, 9), (5, 4), (8, 1)):
        assert lib.wsis_heads_workspace_bytes(64, nh, nl) == -1
    assert lib.wsis_heads_workspace_bytes(64, -1, 2) == -1 and lib.wsis_heads_workspace_bytes(64, 2, -1) == -1


# ---- the position MLP ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [0, 255, 256, 257, 2049])
def test_position_lattice_reference_matches_autograd(E):
    c = ref.pos_lattice(E)
    want = ref.pos_reference(c)
    W1, b1, W2, b2 = (c[k].double().requires_grad_(True) for k in ("W1", "b1", "W2", "b2"))
    d = c["centre"].double()[c["eu"]] - c["centre"].double()[c["ev"]]
    pos = (torch.relu(d @ W1.T + b1) @ W2.T + b2).reshape(-1)
    (pos * c["dpos"].double()).sum().backward()
    assert torch.equal(pos.detach(), want["pos"])
    for name, t in (("dW1", W1), ("db1", b1), ("dW2", W2), ("db2", b2)):
        assert torch.equal(t.grad, want[name]), name
    assert np.ceil(2049 / 256) == 9
