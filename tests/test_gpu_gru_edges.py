"""GPU: the fused GRUCellEx kernels (csrc/gru.hip) and the one-node recurrence _EccGruLoop (wsis_ops.py) against the fp64
restatement of tests/gru_ref.py at every branch of the launch plan -- the default path of every training step (seven
gru_fwd_kernel<true> and seven gru_bwd_kernel evaluations inside the loop).

The cell goes through the C ABI directly: every output pre-filled with NaN, the workspace with 0xFF, every case twice with
identical bytes.  Bounds = FWD / GRAD of tests/test_gpu_lstm_cell.py (forward rtol 1e-4 / atol 1e-5, gradients rtol 1e-3 /
atol 1e-4, atol scaled by max(1, max|ref|)); tests/test_gru_ref_host.py shows ``forward_reference`` in fp32 on the CPU
below a quarter of them on every case here.  The plan a case is named for (slabs, idle waves, trips of the slab reduce,
segment lengths) is derived from gru_ref's restatement of the launch rules and asserted, and held to the C ABI through
wsis_gru_cell_workspace_bytes.

  a  constants         slab = 7392 floats; workspace = min(256, ceil(S / 12)) slabs + 256 bytes; WSIS_GRU_ROWS=1 ->
                       ceil(S / 4) slabs (S = 13: four workgroups, three idle waves)
  b  row counts        1..3 (idle backward waves), 4, 5, 7..9 (forward workgroup of 8 waves), 11..13 (1 and 2 slabs), 84 /
                       96 / 97 (7, 8, 9 slabs against the reduce's 8 slab lanes), 1488 / 1536 / 1537 (124, 128, 129 slabs:
                       16-deep trip on lanes 0..3 only, on all lanes without a tail, with a tail of one), 2048 / 2049 (the
                       forward cap).  S = 13 under the default plan has NO idle wave (the waves stride over the rows of the
                       whole launch: five waves walk two rows, three walk one); idle waves beside a second slab are case a's
  c  fwd_mean          segments of 0, 1, 2, 3, 14..18, 31..33 and 70 messages, a shuffled perm: bit-equal to
                       wsis_segment_reduce_fwd (mean) followed by wsis_gru_cell_fwd
  d  bwd_seq           S = 29; one slot == wsis_gru_cell_bwd, dhy + dhy2 added once in fp32, dhy NULL with a pitch-256 dhy2
                       among NaN columns, 2 and 7 slots (regions of the workspace, parameter outputs untouched before
                       ``finish``), refusals that write nothing
  e  hard rows         x = 0 (1 / sqrt(eps) = 316 in the backward), h = 0, both, rows where eps decides the norm, gate
                       biases that saturate sigmoid / tanh and overflow expf, a saturated input gate, |h| = 50
  f  the loop          RNNGraphConvModule on a 54-node graph (in-hub of 33, no-in, isolated) and on 2 nodes with one edge:
                       R in {0, 1, 3, 7} x cat_all x {default, WSIS_ECC_OWN_GEMM=0, WSIS_GNN_LOOP=0}, the calls counted, the
                       two torch-product paths bit-equal in the forward, frozen inputs bit-equal to the unfrozen run

Tightness: per row count the reference with the LAST row's upstream gradient zeroed must stand outside the bound on every
parameter gradient (and on that row's dx / dh).

Measured on an MI355X (2026-10-21), all 62 tests passing, the whole file in 4.6 s.  Largest error / bound per case group
(forward | gradients), and the smallest factor by which the dropped-row reference stood outside the gradient bound:
  case group                                              forward   gradients
  a  WSIS_GRU_ROWS=1, S = 13                              0.010     0.0016
  b  row counts 1 .. 2049                                 0.030     0.0023     (hy at S = 1; ig.bias at S = 1537)
     dropped last row, six parameter gradients                      >= 38      (ig.bias at S = 2048; >= 300 up to S = 97)
  c  fwd_mean (x_out and hy; == segment mean + cell)      0.0074
  d  dhy NULL, dhy2 at pitch 256                                    0.0012
     2 | 7 slots: dx / dh per slot, parameter sums                  0.0015 | 0.0018
  e  hard rows, all 27 rows                               0.0077    0.0071     (hy of x0; ig.weight of big_h)
     hard rows alone                                      0.0049    0.0028     (hy of sat_bias; dh of big_h)
  f  54 nodes: default | torch products | per op          0.065 | 0.063 | 0.063   0.010 | 0.011 | 0.011  (R = 7, no cat)
     2 nodes, one edge                                    0.016     0.0044
No figure is near 1: the kernels sit where fp32 ``forward_reference`` sits on the CPU (0.019 / 0.0062 there), the recurrence
over seven repeats at three times that.  Every bit-equality above held.

R = 0 under WSIS_GNN_LOOP=0 leaves the filter net without a gradient (``None``; the loop returns zeros): both are the
reference's exact zero and the test says which it expects."""
import copy

import numpy as np
import pytest
import torch

import graphnet
import wsis_native as _n
import wsis_ops
from tests import gru_ref
from tests.test_gpu_lstm_cell import FWD, GRAD, ratio, rec_graph  # noqa: F401  (rec_graph: the 54-node graph, a fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
ORDER = ("ig.weight", "ig.bias", "weight_ih", "weight_hh", "bias_ih", "bias_hh")       # the C ABI's parameter order
SLAB_BYTES = 4 * gru_ref.P_FLOATS
PER_ROW = ("hy", "dx", "dh")


def _lib():
    return _n.hip()


def _nan(*shape):
    return torch.full(shape, NAN, device=DEV)


def _dev(*ts):
    return [t.to(DEV).contiguous() for t in ts]


def _params(cell):
    return {n: t.detach().float().to(DEV).contiguous() for n, t in cell.named_parameters()}


def _pp(p):
    return [_n.ptr(p[n]) for n in ORDER]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bytes(a, b, what):
    for name in a:
        assert torch.equal(_bits(a[name]), _bits(b[name])), f"{what} {name}: not the same bytes"


def _ws(nbytes):
    return torch.full((nbytes,), 255, dtype=torch.uint8, device=DEV)


def _fwd(x, h, p):
    hy = _nan(x.shape[0], 32)
    _n.check(_lib().wsis_gru_cell_fwd(_n.ptr(x), _n.ptr(h), *_pp(p), _n.ptr(hy), x.shape[0], 32, _n.stream_ptr()),
             "gru_cell_fwd")
    return hy


def _grad_outputs(S, p):
    out = {"dx": _nan(S, 32), "dh": _nan(S, 32)}
    out.update({n: torch.full_like(p[n], NAN) for n in ORDER})
    return out


def _bwd(x, h, p, gy):
    lib, S = _lib(), x.shape[0]
    out = _grad_outputs(S, p)
    wsb = lib.wsis_gru_cell_workspace_bytes(S)
    ws = _ws(wsb)
    _n.check(lib.wsis_gru_cell_bwd(_n.ptr(x), _n.ptr(h), *_pp(p), _n.ptr(gy), _n.ptr(out["dx"]), _n.ptr(out["dh"]),
                                   *[_n.ptr(out[n]) for n in ORDER], S, 32, _n.ptr(ws), wsb, _n.stream_ptr()),
             "gru_cell_bwd")
    torch.cuda.synchronize()
    return out


def _cell_run(x, h, p, gy):
    out = _bwd(x, h, p, gy)
    out["hy"] = _fwd(x, h, p)
    torch.cuda.synchronize()
    return out


def _seq(x, h, p, dhy, dhy2, pitch, out, slot, n_slots, finish, ws, ws_bytes=None, params=True):
    """one raw wsis_gru_cell_bwd_seq call -> status (dhy2: an address or None; params=False: NULL parameter outputs)"""
    st = _lib().wsis_gru_cell_bwd_seq(
        _n.ptr(x), _n.ptr(h), *_pp(p), _n.ptr(dhy), dhy2, pitch, _n.ptr(out["dx"]), _n.ptr(out["dh"]),
        *[_n.ptr(out[n]) if params else None for n in ORDER], x.shape[0], 32, slot, n_slots, finish, _n.ptr(ws),
        ws.numel() if ws_bytes is None else ws_bytes, _n.stream_ptr())
    torch.cuda.synchronize()
    return st


def _seq_ws_bytes(S, n_slots):
    return (_lib().wsis_gru_cell_workspace_bytes(S) - 256) * n_slots + 256


def _ref(cell, x, h, dhy, dhy2=None):
    """the fp64 restatement on host tensors -> ({hy, dx, dh, <parameter>: gradient}, cache)"""
    P = gru_ref.params_of(cell)
    hy, k = gru_ref.cell_fwd(P, x.numpy(), h.numpy())
    out = gru_ref.cell_bwd(P, k, None if dhy is None else dhy.numpy(), None if dhy2 is None else dhy2.numpy())
    out["hy"] = hy
    return out, k


def _compare(got, want, what, rows=None):
    """every output and gradient of ``want`` within the bounds (``rows``: the per-row tensors on those rows alone too, with
    their own scale); prints and returns the figures"""
    rep = {}
    for name, w in want.items():
        tol = FWD if name in ("hy", "out", "x_out") else GRAD
        rep[name] = ratio(got[name], w, tol)
        if rows is not None and name in PER_ROW:
            rep[name + "@hard"] = ratio(got[name][rows], w[rows], tol)
    print(what, {k: "%.2g" % v for k, v in rep.items()})
    bad = {k: v for k, v in rep.items() if not v <= 1.0}
    assert not bad, (what, bad)
    return rep


# ---------------------------------------------------------------- a. the named constants are the kernels'
def test_the_named_constants_are_the_kernels():
    ws = _lib().wsis_gru_cell_workspace_bytes
    assert gru_ref.P_FLOATS == 7392 and SLAB_BYTES == 29568
    for S in (1, 12, 13, 3072, 3073):
        assert ws(S) == min(256, -(-S // 12)) * 29568 + 256 == gru_ref.slabs(S) * SLAB_BYTES + 256, S
    for S, n in gru_ref.ROW_COUNTS.items():
        assert ws(S) == n * SLAB_BYTES + 256, S


def test_one_row_per_wave_under_the_tuning_knob(monkeypatch):
    """WSIS_GRU_ROWS=1 (read per call): min(256, ceil(S / 4)) slabs; S = 13 then runs four workgroups, the last with one
    row and three idle waves beside three other slabs"""
    S = 13
    monkeypatch.setenv("WSIS_GRU_ROWS", "1")
    ws = _lib().wsis_gru_cell_workspace_bytes
    for s in (1, 4, 5, 13, 1024, 1025, 3073):
        assert ws(s) == min(256, -(-s // 4)) * SLAB_BYTES + 256 == gru_ref.slabs(s, 1) * SLAB_BYTES + 256, s
    assert gru_ref.bwd_rows_per_wave(S, 1) == [[1] * 4] * 3 + [[1, 0, 0, 0]] and gru_ref.idle_bwd_waves(S, 1) == 3
    cell = gru_ref.make_cell(130)
    x, h, gy = gru_ref.make_rows(131, S, 3)
    want, _ = _ref(cell, x, h, gy)
    p = _params(cell)
    dx, dh, dgy = _dev(x, h, gy)
    got = _cell_run(dx, dh, p, dgy)
    _same_bytes(got, _cell_run(dx, dh, p, dgy), "WSIS_GRU_ROWS=1")
    _compare(got, want, "WSIS_GRU_ROWS=1 S=13")
    monkeypatch.delenv("WSIS_GRU_ROWS")
    assert ws(S) == 2 * SLAB_BYTES + 256


# ---------------------------------------------------------------- b. row counts
def _assert_plan(S):
    """the branch the row count is named for, from the restated plan"""
    nslab, rows = gru_ref.slabs(S), gru_ref.bwd_rows_per_wave(S)
    assert nslab == gru_ref.ROW_COUNTS[S] and sum(map(sum, rows)) == S
    plan = gru_ref.reduce_plan(nslab)
    if S <= 3:
        assert gru_ref.idle_bwd_waves(S) == 4 - S and nslab == 1
    if S in (4, 5):
        assert rows == [[1 + (S == 5), 1, 1, 1]]
    if S in (7, 8, 9):
        assert gru_ref.fwd_workgroups(S) == (2 if S == 9 else 1)
    if S in (11, 12):
        assert rows == ([[3, 3, 3, 2]] if S == 11 else [[3, 3, 3, 3]])
    if S == 13:
        assert rows == [[2, 2, 2, 2], [2, 1, 1, 1]]
    if nslab < 8:
        assert [t for t, _ in plan] == [0] * 8 and [n for _, n in plan] == [1] * nslab + [0] * (8 - nslab)
    if S in (96, 97):
        assert plan == ([(0, 1)] * 8 if S == 96 else [(0, 2)] + [(0, 1)] * 7)
    if S == 1488:
        assert plan == [(1, 0)] * 4 + [(0, 15)] * 4        # lanes 0..3 the unrolled trip, lanes 4..7 only the tail
    if S == 1536:
        assert plan == [(1, 0)] * 8                         # one trip, no tail
    if S == 1537:
        assert plan == [(1, 1)] + [(1, 0)] * 7
    if S in (2048, 2049):
        assert gru_ref.fwd_workgroups(S) == 256 and -(-S // 8) == (256 if S == 2048 else 257)     # the cap: the first wave
        #                                                                          of workgroup 0 walks row 2048 as well


@pytest.mark.parametrize("S", list(gru_ref.ROW_COUNTS))
def test_cell_fwd_bwd_at_every_row_count(S):
    _assert_plan(S)
    assert _lib().wsis_gru_cell_workspace_bytes(S) == gru_ref.ROW_COUNTS[S] * SLAB_BYTES + 256
    cell = gru_ref.make_cell(S)
    x, h, gy = gru_ref.make_rows(S + 1, S, 3)
    want, _ = _ref(cell, x, h, gy)
    p = _params(cell)
    dx, dh, dgy = _dev(x, h, gy)
    got = _cell_run(dx, dh, p, dgy)
    _same_bytes(got, _cell_run(dx, dh, p, dgy), f"S={S}")
    _compare(got, want, f"S={S}")
    # the last row's upstream gradient dropped: out of every parameter sum, its own dx / dh rows 0
    gy_drop = gy.clone()
    gy_drop[-1] = 0
    drop, _ = _ref(cell, x, h, gy_drop)
    out = {n: ratio(got[n], drop[n], GRAD) for n in ORDER + ("dx", "dh")}
    print(f"S={S} dropped row / bound", {k: "%.3g" % v for k, v in out.items()})
    assert all(v > 1.0 for v in out.values()), (S, out)


# ---------------------------------------------------------------- c. the mean folded into the forward
SEG_LENGTHS = (0, 1, 2, 3, 14, 15, 16, 17, 18, 31, 32, 33, 70)


def test_fwd_mean_is_segment_mean_then_cell_bit_for_bit():
    S = 70
    rng = np.random.default_rng(70)
    lengths = np.concatenate([SEG_LENGTHS, rng.integers(1, 9, S - len(SEG_LENGTHS))])
    lengths = lengths[rng.permutation(S)]
    assert len(lengths) == S and set(SEG_LENGTHS) <= set(lengths.tolist())
    # lane group 0 of gru_seg_mean takes the 8-deep trip from 15 messages on, group 1 from 16: both sides of each
    assert {14, 15, 16, 17} <= set(lengths.tolist())
    index = np.repeat(np.arange(S), lengths)
    index = index[rng.permutation(len(index))]                 # message e belongs to row index[e]: a non-identity perm
    E = len(index)
    perm_np = np.argsort(index, kind="stable").astype(np.int32)
    off_np = np.searchsorted(index[perm_np], np.arange(S + 1)).astype(np.int32)
    assert (np.diff(off_np) == lengths).all() and (perm_np != np.arange(E)).any()
    perm, off = torch.from_numpy(perm_np).to(DEV), torch.from_numpy(off_np).to(DEV)
    cell = gru_ref.make_cell(71)
    g = torch.Generator().manual_seed(72)
    m, h = torch.randn(E, 32, generator=g), torch.randn(S, 32, generator=g)
    p = _params(cell)
    dm, dh = _dev(m, h)
    lib = _lib()

    def fused():
        x_out, hy = _nan(S, 32), _nan(S, 32)
        _n.check(lib.wsis_gru_cell_fwd_mean(_n.ptr(dm), _n.ptr(perm), _n.ptr(off), _n.ptr(x_out), _n.ptr(dh), *_pp(p),
                                            _n.ptr(hy), S, 32, _n.stream_ptr()), "gru_cell_fwd_mean")
        torch.cuda.synchronize()
        return {"x_out": x_out, "hy": hy}

    got = fused()
    _same_bytes(got, fused(), "fwd_mean")
    mean = _nan(S, 32)
    _n.check(lib.wsis_segment_reduce_fwd(_n.ptr(dm), _n.ptr(perm), _n.ptr(off), _n.ptr(mean), None, E, S, 32, 1,
                                         _n.stream_ptr()), "segment_reduce_fwd")
    two = {"x_out": mean, "hy": _fwd(mean, dh, p)}
    torch.cuda.synchronize()
    _same_bytes(got, two, "fwd_mean against segment mean + cell")
    x64 = np.zeros((S, 32))
    np.add.at(x64, index, m.double().numpy())
    x64 /= np.maximum(lengths, 1)[:, None]
    hy64, _ = gru_ref.cell_fwd(gru_ref.params_of(cell), x64, h.numpy())
    _compare(got, {"x_out": x64, "hy": hy64}, "fwd_mean")
    _compare(two, {"x_out": x64, "hy": hy64}, "segment mean + cell")
    empty = int(np.flatnonzero(lengths == 0)[0])
    assert bool((got["x_out"][empty] == 0).all()) and float(np.abs(x64[empty]).max()) == 0.0


# ---------------------------------------------------------------- d. the backward as one evaluation of a sequence
SEQ_S = 29


def _seq_inputs(seed, n=1):
    cell = gru_ref.make_cell(seed)
    rows = [gru_ref.make_rows(seed + 1 + k, SEQ_S, 4) for k in range(n)]
    return cell, _params(cell), rows


def test_the_plan_of_the_sequence_cases():
    assert gru_ref.slabs(SEQ_S) == 3
    # 12 waves stride over 29 rows: waves 0..4 of the launch walk three rows, the other seven two
    assert gru_ref.bwd_rows_per_wave(SEQ_S) == [[3, 3, 3, 3], [3, 2, 2, 2], [2, 2, 2, 2]]
    assert _seq_ws_bytes(SEQ_S, 1) == _lib().wsis_gru_cell_workspace_bytes(SEQ_S) == 3 * SLAB_BYTES + 256
    assert _seq_ws_bytes(SEQ_S, 7) == 21 * SLAB_BYTES + 256


@pytest.mark.parametrize("up", ["dhy", "both"])
def test_a_sequence_of_one_is_the_single_backward(up):
    """slot 0 of 1 is first, last and finishing at once; dhy + dhy2 (pitch 32) = the single backward fed their fp32 sum"""
    cell, p, [(x, h, dhy, dhy2)] = _seq_inputs(290)
    x, h, dhy, dhy2 = _dev(x, h, dhy, dhy2)

    def run():
        out, ws = _grad_outputs(SEQ_S, p), _ws(_seq_ws_bytes(SEQ_S, 1))
        assert _seq(x, h, p, dhy, dhy2.data_ptr() if up == "both" else None, 32 if up == "both" else 0, out, 0, 1, 1,
                    ws) == 0
        return out

    got = run()
    _same_bytes(got, run(), "seq of one")
    single = _bwd(x, h, p, dhy + dhy2 if up == "both" else dhy)
    assert all(bool(torch.isfinite(t).all()) for t in got.values())
    _same_bytes(got, single, "seq of one against gru_cell_bwd")


def test_only_the_second_gradient_at_a_wide_pitch():
    """dhy NULL, dhy2 = columns 96..127 of a [S, 256] tensor whose other columns are NaN"""
    cell, p, [(x, h, _, dhy2)] = _seq_inputs(291)
    want, _ = _ref(cell, x, h, None, dhy2)
    x, h = _dev(x, h)
    wide = _nan(SEQ_S, 256)
    wide[:, 96:128] = dhy2.to(DEV)

    def run():
        out, ws = _grad_outputs(SEQ_S, p), _ws(_seq_ws_bytes(SEQ_S, 1))
        assert _seq(x, h, p, None, wide.data_ptr() + 4 * 96, 256, out, 0, 1, 1, ws) == 0
        return out

    got = run()
    _same_bytes(got, run(), "dhy2 alone")
    want.pop("hy")
    _compare(got, want, "dhy NULL, dhy2 at pitch 256")


@pytest.mark.parametrize("n_slots", [2, 7])
def test_slots_of_a_sequence(n_slots):
    """the order of _EccGruLoop.backward: slot 0 first (no carried gradient: dhy NULL), ``finish`` on the last; slot k adds
    slice k of a [S, 32 n] output gradient"""
    cell, p, rows = _seq_inputs(292 + n_slots, n_slots)
    gcat = torch.cat([r[3] for r in rows], 1)                       # dhy2 of slot k = columns 32 k .. 32 k + 31
    wants = [_ref(cell, x, h, None if k == 0 else dhy, dhy2)[0] for k, (x, h, dhy, dhy2) in enumerate(rows)]
    dev_rows = [_dev(*r) for r in rows]
    dcat = gcat.to(DEV).contiguous()
    region = 3 * SLAB_BYTES

    def run(check):
        ws = _ws(_seq_ws_bytes(SEQ_S, n_slots))
        pouts = {n: torch.full_like(p[n], NAN) for n in ORDER}
        outs = []
        for k, (x, h, dhy, _) in enumerate(dev_rows):
            out = dict(pouts, dx=_nan(SEQ_S, 32), dh=_nan(SEQ_S, 32))
            before = ws.clone()
            assert _seq(x, h, p, None if k == 0 else dhy, dcat.data_ptr() + 4 * 32 * k, 32 * n_slots, out, k, n_slots,
                        int(k == n_slots - 1), ws) == 0
            outs.append(out)
            if not check:
                continue
            changed = (ws != before).nonzero().flatten()
            assert changed.numel() > 0.9 * region, "the slot's slabs are written"
            assert int(changed.min()) >= k * region and int(changed.max()) < (k + 1) * region, \
                f"slot {k} wrote outside its region of the workspace"
            mine = ws[k * region:(k + 1) * region].view(torch.float32)
            assert bool(torch.isfinite(mine).all()), "every float of the slot's three slabs is written"
            if k < n_slots - 1:
                assert all(bool(torch.isnan(t).all()) for t in pouts.values()), "parameter outputs before finish"
        return outs, pouts

    outs, pouts = run(True)
    outs2, pouts2 = run(False)
    _same_bytes(pouts, pouts2, f"{n_slots} slots")
    for k in range(n_slots):
        _same_bytes({n: outs[k][n] for n in ("dx", "dh")}, {n: outs2[k][n] for n in ("dx", "dh")}, f"slot {k}")
        _compare(outs[k], {n: wants[k][n] for n in ("dx", "dh")}, f"{n_slots} slots, slot {k}")
    _compare(pouts, {n: sum(w[n] for w in wants) for n in ORDER}, f"{n_slots} slots, parameter gradients")


@pytest.mark.parametrize("what", ["slot", "no_gradient", "pitch", "finish_null", "short_ws"])
def test_refusals_write_nothing(what):
    cell, p, [(x, h, dhy, dhy2)] = _seq_inputs(299)
    x, h, dhy, dhy2 = _dev(x, h, dhy, dhy2)
    out, ws = _grad_outputs(SEQ_S, p), _ws(_seq_ws_bytes(SEQ_S, 2))
    if what == "slot":
        st = _seq(x, h, p, dhy, None, 0, out, 2, 2, 0, ws)
    elif what == "no_gradient":
        st = _seq(x, h, p, None, None, 32, out, 0, 2, 0, ws)
    elif what == "pitch":
        st = _seq(x, h, p, dhy, dhy2.data_ptr(), 31, out, 0, 2, 0, ws)
    elif what == "finish_null":
        st = _seq(x, h, p, dhy, None, 0, out, 1, 2, 1, ws, params=False)
    else:
        st = _seq(x, h, p, dhy, None, 0, out, 0, 2, 0, ws, ws_bytes=ws.numel() - 1)
    assert st != 0 and _lib().wsis_last_error()
    assert all(bool(torch.isnan(t).all()) for t in out.values()) and bool((ws == 255).all())


# ---------------------------------------------------------------- e. hard rows beside ordinary ones
@pytest.mark.parametrize("kind", gru_ref.HARD_KINDS)
def test_cell_on_hard_rows(kind):
    cell, x, h, gy = gru_ref.hard_case(kind)
    want, k = _ref(cell, x, h, gy)
    gru_ref.check_hardness(kind, k)
    assert gru_ref.bwd_rows_per_wave(gru_ref.HARD_S) == [[3, 3, 3, 2], [2, 2, 2, 2], [2, 2, 2, 2]]
    p = _params(cell)
    dx, dh, dgy = _dev(x, h, gy)
    got = _cell_run(dx, dh, p, dgy)
    _same_bytes(got, _cell_run(dx, dh, p, dgy), kind)
    _compare(got, want, kind, rows=gru_ref.HARD_ROWS)


# ---------------------------------------------------------------- f. the one-node loop
PATHS = {"default": {}, "torch_gemm": {"WSIS_ECC_OWN_GEMM": "0"}, "per_op": {"WSIS_GNN_LOOP": "0"}}


@pytest.fixture(scope="module")
def two_nodes():
    g = torch.Generator().manual_seed(8)
    return dict(src=np.array([0]), tgt=np.array([1]), S=2, feats=torch.randn(1, 13, generator=g),
                x=torch.randn(2, 32, generator=g))


def _module(R, cat_all):
    torch.manual_seed(40 + R)
    fnet = graphnet.create_fnet([13, 32, 128, 64, 32 * 32], True, True, -1)
    return graphnet.RNNGraphConvModule(gru_ref.make_cell(41), fnet, 32, vv=False, nrepeats=R, cat_all=cat_all)


def _gout(S, R, cat_all):
    g = torch.randn(S, 32 * 8, generator=torch.Generator().manual_seed(9))
    return g[:, :32 * (R + 1)].contiguous() if cat_all else g[:, :32].contiguous()


def _count_calls(monkeypatch):
    calls = {"loop": 0, "cell": 0}
    for key, name in (("loop", "ecc_gru_loop"), ("cell", "gru_cell_ex")):
        monkeypatch.setattr(wsis_ops, name,
                            lambda *a, _f=getattr(wsis_ops, name), _k=key: (calls.__setitem__(_k, calls[_k] + 1), _f(*a))[1])
    return calls


def _loop_run(mod, G, gout, hx_grad=True):
    """{out, dhx, <parameter name>: gradient or None} of a device copy of ``mod``"""
    mod = copy.deepcopy(mod).to(DEV)
    ei = torch.from_numpy(np.stack([G["src"], G["tgt"]]))
    mod.set_info(graphnet.GraphConvInfo(ei.to(DEV), G["feats"].to(DEV), G["S"]))
    x = G["x"].clone().to(DEV).requires_grad_(hx_grad)
    assert mod._contract_ok(x)
    out = mod(x)
    if out.requires_grad:
        out.backward(gout.to(DEV))
    torch.cuda.synchronize()
    got = {"out": out.detach(), "dhx": x.grad}
    got.update({n: p.grad for n, p in mod.named_parameters()})
    return got


def _loop_ref(mod, G, R, cat_all, gout):
    ref = copy.deepcopy(mod).double()
    W = ref._fnet(G["feats"].double()).view(-1, 32, 32)
    out, gr = gru_ref.recurrence(gru_ref.params_of(ref._cell), G["x"].numpy(), W.detach().numpy(), G["src"], G["tgt"], R,
                                 cat_all, gout.numpy())
    W.backward(torch.from_numpy(gr["dW"]))
    want = {"out": out, "dhx": gr["dhx"]}
    want.update({"_cell." + n: gr[n] for n in gru_ref.NAMES})
    want.update({"_fnet." + n: q.grad.numpy() for n, q in ref._fnet.named_parameters()})
    return want


@pytest.mark.parametrize("cat_all", [True, False])
@pytest.mark.parametrize("R", [0, 1, 3, 7])
@pytest.mark.parametrize("graph", ["hub54", "two_nodes"])
def test_recurrence_equals_the_fp64_recurrence_on_every_path(rec_graph, two_nodes, graph, R, cat_all, monkeypatch):
    G = rec_graph if graph == "hub54" else two_nodes
    if graph == "hub54":
        assert G["roles"]["isolated"] and G["roles"]["no_in"] and max(G["roles"]["in_hub"].values()) == 33
    mod = _module(R, cat_all)
    gout = _gout(G["S"], R, cat_all)
    want = _loop_ref(mod, G, R, cat_all, gout)
    assert want["out"].shape == (G["S"], 32 * (R + 1) if cat_all else 32)
    calls = _count_calls(monkeypatch)
    fwd = {}
    for path, env in PATHS.items():
        with monkeypatch.context() as mp:
            for key, val in env.items():
                mp.setenv(key, val)
            calls.update(loop=0, cell=0)
            got = _loop_run(mod, G, gout)
            assert calls == ({"loop": 0, "cell": R} if path == "per_op" else {"loop": 1, "cell": 0}), (path, calls)
            again = _loop_run(mod, G, gout)
        fwd[path] = got["out"]
        if R == 0:
            # the reference's gradient of every parameter is an exact zero: the loop returns zeros for the filter net and
            # the cell, the per-op path never touched them
            assert all(float(np.abs(want[n]).max()) == 0.0 for n in want if n not in ("out", "dhx"))
            for n in [n for n in want if n not in ("out", "dhx")]:
                if path == "per_op":
                    assert got[n] is None, (path, n)
                    got[n] = again[n] = torch.zeros(want[n].shape)
                else:
                    assert got[n] is not None and float(got[n].abs().max()) == 0.0, (path, n)
        _same_bytes(got, again, f"{graph} R={R} cat_all={cat_all} {path}")
        _compare(got, want, f"{graph} R={R} cat_all={cat_all} {path}")
    # the same kernels in the same order (the docstring of _EccGruLoop)
    assert torch.equal(_bits(fwd["torch_gemm"]), _bits(fwd["per_op"]))


@pytest.mark.parametrize("path", ["default", "torch_gemm"])
@pytest.mark.parametrize("frozen", ["hx", "cell", "fnet"])
def test_frozen_inputs_leave_the_other_gradients_bit_equal(rec_graph, frozen, path, monkeypatch):
    G, R = rec_graph, 3
    for key, val in PATHS[path].items():
        monkeypatch.setenv(key, val)
    mod = _module(R, True)
    gout = _gout(G["S"], R, True)
    calls = _count_calls(monkeypatch)
    full = _loop_run(mod, G, gout)
    assert all(v is not None for v in full.values())
    part_mod = copy.deepcopy(mod)
    for n, q in part_mod.named_parameters():
        if n.startswith("_" + frozen + "."):
            q.requires_grad_(False)
    part = _loop_run(part_mod, G, gout, hx_grad=frozen != "hx")
    assert calls == {"loop": 2, "cell": 0}
    gone = [n for n in full if (n == "dhx" if frozen == "hx" else n.startswith("_" + frozen + "."))]
    assert len(gone) == {"hx": 1, "cell": 6, "fnet": 8}[frozen]
    for n in full:
        if n in gone:
            assert part[n] is None, n
        else:
            assert torch.equal(_bits(part[n]), _bits(full[n])), (frozen, path, n)
