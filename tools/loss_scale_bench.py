"""What dynamic loss scaling costs around the one-launch AdamW, on the C2 model's parameter tensors (GPU box), one JSON line
on stdout (profiles/loss_scale_bench.json is a recorded run):
   python tools/loss_scale_bench.py [--rounds N]

Four ways through one optimizer step over the same parameters and gradients, alternated in one process, median of
``--rounds`` (30) of the time between two device events around the step -- with the step queued behind other device work
(device_us) and alone (lone_us) -- and of the host time the calls take:
  plain                 FlatAdamW.step()                                  (wsis_adamw_step, no scaling)
  loss_scaler           LossScaler.step + update                          (wsis_grad_nonfinite, wsis_adamw_step_scaled,
                                                                           wsis_loss_scale_update: no read-back)
  grad_scaler_generic   torch.amp.GradScaler.step + update with FlatAdamW's _step_supports_amp_scaling cleared on the
                        instance: unscale_ over every gradient, found_inf.item(), then the plain step -- what an
                        optimizer without the protocol gets
  grad_scaler_protocol  torch.amp.GradScaler.step + update through the protocol (torch's own non-finite check, then
                        wsis_adamw_step_scaled)
The scale is 1 everywhere (unscale_ rewrites the gradients in place every step; the arithmetic does not depend on the
value), the gradients are finite, no step is skipped.  Each optimizer has its own copy of the parameters."""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
importlib.import_module("3d-wsis_amd")
import numpy as np  # noqa: E402
import torch  # noqa: E402

import harness  # noqa: E402
import wsis_optim  # noqa: E402

DEV = "cuda:0"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    a = ap.parse_args()
    model, _, _ = harness.build_model(harness.default_cfg(), DEV)
    shapes = [tuple(p.shape) for p in model.parameters() if p.requires_grad]
    g = torch.Generator(device=DEV).manual_seed(0)
    grads = [torch.randn(s, device=DEV, generator=g) * 1e-3 for s in shapes]
    variants = {}
    for name in ("plain", "loss_scaler", "grad_scaler_generic", "grad_scaler_protocol"):
        params = [p.detach().clone().requires_grad_(True) for p in model.parameters() if p.requires_grad]
        for p, gr in zip(params, grads):
            p.grad = gr.clone()
        opt = wsis_optim.FlatAdamW(params, lr=1e-3, weight_decay=1e-4)
        if name == "plain":
            run = opt.step
        else:
            if name == "loss_scaler":
                sc = wsis_optim.LossScaler(init_scale=1.0)
            else:
                sc = torch.amp.GradScaler("cuda", init_scale=1.0)
                sc.scale(torch.zeros((), device=DEV))       # torch makes its scale tensor when a loss is first scaled
                if name == "grad_scaler_generic":
                    opt._step_supports_amp_scaling = False

            def run(sc=sc, opt=opt):
                sc.step(opt)
                sc.update()
        variants[name] = (run, opt)
    # "queued": a ~1 ms matrix product runs in front of the first event, so the host has issued the whole step before the
    # GPU reaches it and the events see device time alone -- unless the step makes the host wait for the device
    # (found_inf.item()), which then shows as the gap it is.  "lone": nothing in front; the host's own work (filling
    # the segment table, torch's Python walk) is inside the interval.
    filler = torch.randn(4096, 4096, device=DEV)
    dev_ms = {m: {k: [] for k in variants} for m in ("queued", "lone")}
    host_ms = {k: [] for k in variants}
    for r in range(3 + a.rounds):                     # three untimed rounds first
        for mode in ("queued", "lone"):
            for name, (run, _) in variants.items():
                torch.cuda.synchronize()
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                if mode == "queued":
                    torch.mm(filler, filler)
                t0 = time.perf_counter()
                s.record()
                run()
                e.record()
                t1 = time.perf_counter()
                torch.cuda.synchronize()
                if r >= 3:
                    dev_ms[mode][name].append(s.elapsed_time(e))
                    if mode == "lone":
                        host_ms[name].append((t1 - t0) * 1e3)
    n = int(sum(int(np.prod(s)) for s in shapes))
    res = {"tool": "loss_scale_bench", "device": torch.cuda.get_device_name(0), "rounds": a.rounds,
           "tensors": len(shapes), "parameters": n, "check_bytes": 4 * n, "step_bytes": 28 * n}
    for name, (_, opt) in variants.items():
        res[name] = {"device_us_median": float(np.median(dev_ms["queued"][name])) * 1e3,
                     "device_us_min": float(np.min(dev_ms["queued"][name])) * 1e3,
                     "lone_us_median": float(np.median(dev_ms["lone"][name])) * 1e3,
                     "host_us_median": float(np.median(host_ms[name])) * 1e3,
                     "scaled_entry_point": opt._skipped is not None}
    us = {k: res[k]["device_us_median"] for k in variants}
    res["loss_scaler_minus_plain_us"] = us["loss_scaler"] - us["plain"]
    res["loss_scaler_over_grad_scaler_generic"] = us["loss_scaler"] / us["grad_scaler_generic"]
    assert not res["plain"]["scaled_entry_point"] and not res["grad_scaler_generic"]["scaled_entry_point"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
