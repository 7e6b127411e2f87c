"""16-bit against fp32 sparse convolutions on the C2 scene's real tables (GPU box), one JSON line on stdout:
   python tools/lowp_conv_bench.py [--steps N]

Per UNet layer shape of levels 0-4 (SubM C -> C, SubM 2C -> C of the decoder, SparseConv3d C -> C') at one and at four
scenes: us per launch of the forward, dIn and dW products in fp32, bf16 and fp16 (the weight cast is not timed: it is
one small launch per call), the algorithmic bytes P (Cin + Cout) e + 8 P with e = 4 / 2 bytes per feature value, their
fraction of 8 TB/s, and the max error of the 16-bit forward against fp64 on sampled rows (relative to max |ref|).
Then one Network forward + loss + backward in three forms -- fp32 recorded native pass, fp32 module walk, bf16 autocast
module walk -- with the step time and torch.cuda.max_memory_allocated."""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
importlib.import_module("3d-wsis_amd")
import numpy as np  # noqa: E402
import torch  # noqa: E402

import harness  # noqa: E402
from spconv import ops  # noqa: E402

DEV = "cuda:0"
PLANES = (32, 64, 96, 128, 160)
HBM = 8.0e12


def timeit(f, n):
    for _ in range(3):
        f()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n):
        f()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / n * 1e3


def levels_of(scenes):
    b = harness.collate(scenes)
    idx = b["voxel_locs"].int().to(DEV).contiguous()
    shape = [int(s) for s in b["spatial_shape"]]
    out = []
    for l in range(5):
        ent = {"M": int(idx.shape[0]), "subm": ops.build_subm_rulebook(idx, shape, [3] * 3, [1] * 3)}
        if l < 4:
            ent["down"] = ops.build_down_rulebook(idx, shape, [2] * 3, [2] * 3, [0] * 3)
            idx, shape = ent["down"].out_indices, ent["down"].out_shape
        out.append(ent)
    return out


def max_rel_err(X16, W, nbr, order, out16, M_out, n=256):
    """max |out16 - fp64| / max |fp64| over n sampled output rows (X16 and the 16-bit-rounded W in fp64)"""
    K = W.shape[0]
    g = torch.Generator(device=DEV).manual_seed(0)
    sel = torch.randperm(M_out, device=DEV, generator=g)[:n]
    nb = nbr.long()
    if order is not None:                      # packed table: column t is output row order[t]
        col = torch.empty(M_out, dtype=torch.long, device=DEV)
        col[order.long()] = torch.arange(M_out, device=DEV)
        nb = nb[:, col[sel]]
    else:
        nb = nb[:, sel]
    Wd = W.to(X16.dtype).double()
    ref = torch.zeros(sel.numel(), W.shape[2], dtype=torch.float64, device=DEV)
    for k in range(K):
        hit = nb[k] >= 0
        ref[hit] += X16[nb[k][hit]].double() @ Wd[k]
    return float((out16[sel].double() - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def product_rows(levels, steps):
    rows = []
    for l, ent in enumerate(levels):
        C = PLANES[l]
        M = ent["M"]
        jobs = [("subm", C, C, ent["subm"].nbr_p, ent["subm"].order, ent["subm"].nbr_p, ent["subm"].order, 1, M)]
        if l < 4:
            jobs.append(("subm_cat", 2 * C, C, ent["subm"].nbr_p, ent["subm"].order, ent["subm"].nbr_p,
                         ent["subm"].order, 1, M))
            d = ent["down"]
            jobs.append(("down", C, PLANES[l + 1], d.nbr_p, d.order, d.nbr_up_p, d.order_up, 0, d.out_indices.shape[0]))
        for name, cin, cout, nf, of, nb, ob, flip, M_out in jobs:
            K = nf.shape[0]
            P = int((nf >= 0).sum())
            W = torch.randn(K, cin, cout, device=DEV) / np.sqrt(K * cin)
            X = torch.randn(M, cin, device=DEV)
            dY = torch.randn(M_out, cout, device=DEV)
            row = {"level": l, "layer": name, "Cin": cin, "Cout": cout, "K": K, "rows_in": M, "rows_out": int(M_out),
                   "pairs": P}
            t = {"fwd": timeit(lambda: ops._fwd_fp32(X, nf, of, W, None, M_out), steps),
                 "dIn": timeit(lambda: ops._din_fp32(dY, nb, ob, W, flip, M), steps),
                 "dW": timeit(lambda: ops._dw(X, nf, of, dY, K, cin, cout), steps)}
            row["fp32"] = {"us": t, "bytes": P * (cin + cout) * 4 + 8 * P}
            for dt, tag in ((torch.bfloat16, "bf16"), (torch.float16, "fp16")):
                X16, dY16 = X.to(dt), dY.to(dt)
                WT, W16 = ops._weight_lp(W, dt, 1, 0), ops._weight_lp(W, dt, 0, 0)
                t = {"fwd": timeit(lambda: ops._conv_lp(X16, nf, of, WT, 0, None, M_out), steps),
                     "dIn": timeit(lambda: ops._conv_lp(dY16, nb, ob, W16, flip, None, M), steps),
                     "dW": timeit(lambda: ops._dw_lp(X16, nf, of, dY16, K, cin, cout), steps)}
                out16 = ops._conv_lp(X16, nf, of, WT, 0, None, M_out)
                row[tag] = {"us": t, "bytes": P * (cin + cout) * 2 + 8 * P,
                            "fwd_max_rel_err": max_rel_err(X16, W, nf, of, out16, int(M_out))}
            for tag in ("fp32", "bf16", "fp16"):
                r = row[tag]
                r["frac_8TBps"] = {k: r["bytes"] / (v * 1e-6) / HBM for k, v in r["us"].items()}
            row["bf16_over_fp32"] = {k: row["bf16"]["us"][k] / row["fp32"]["us"][k] for k in ("fwd", "dIn", "dW")}
            rows.append(row)
            print(f"L{l} {name:8s} {cin:3d}->{cout:3d}  fp32 " +
                  " ".join(f"{k} {v:7.1f}" for k, v in row["fp32"]["us"].items()) + " | bf16 " +
                  " ".join(f"{k} {v:7.1f}" for k, v in row["bf16"]["us"].items()), file=sys.stderr)
    return rows


def network_forms(steps):
    cfg = harness.default_cfg()
    batch = harness.to_device(harness.collate([harness.bench_scene(1)]), DEV)
    model, crit, _ = harness.build_model(cfg, DEV)
    out = {}
    for form, native, autocast in (("fp32_native", "1", False), ("fp32_modules", "0", False),
                                   ("bf16_autocast_modules", "1", True)):
        os.environ["WSIS_NATIVE_UNET"] = native

        def step():
            model.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
                loss, _ = harness.forward_loss(model, crit, batch, cfg)
            loss.backward()
            return loss

        step()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        ms = timeit(step, steps) / 1e3
        out[form] = {"ms": ms, "max_memory_allocated": int(torch.cuda.max_memory_allocated()),
                     "pass": getattr(model, "last_pass", None), "loss": float(step().detach())}
    os.environ["WSIS_NATIVE_UNET"] = "1"
    out["bf16_over_fp32_modules"] = {
        "ms": out["bf16_autocast_modules"]["ms"] / out["fp32_modules"]["ms"],
        "memory": out["bf16_autocast_modules"]["max_memory_allocated"] / out["fp32_modules"]["max_memory_allocated"]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()
    res = {"tool": "lowp_conv_bench", "device": torch.cuda.get_device_name(0), "steps": a.steps}
    res["one_scene"] = product_rows(levels_of([harness.make_scene(1)]), a.steps)
    res["four_scenes"] = product_rows(levels_of([harness.bench_scene(s) for s in (1, 2, 3, 4)]), a.steps)
    res["network"] = network_forms(max(3, a.steps // 4))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
