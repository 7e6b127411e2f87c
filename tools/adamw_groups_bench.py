"""What a second parameter group costs the one-launch AdamW, on the default Network's parameter tensors (GPU box), one JSON
line on stdout:
   python tools/adamw_groups_bench.py [--rounds N]

Four optimizers over copies of the same parameters and gradients, alternated in one process:
  one_group            FlatAdamW(params).step()                              (wsis_adamw_step: the step as it always was)
  two_groups           FlatAdamW(split_decay_groups(model, wd)).step()       (wsis_adamw_step_groups)
  one_group_scaled     LossScaler.step + update over one group               (wsis_adamw_step_scaled)
  two_groups_scaled    LossScaler.step + update over the two groups          (wsis_adamw_step_scaled_groups)
Per variant the median, the minimum and the 10th / 90th percentile over ``--rounds`` (50) of the time between two device
events around the step, with a ~1 ms matrix product queued in front so that the host has issued everything before the
GPU arrives (device_us: device time alone), and of the host time the calls take with nothing in front (host_us).  The
one-group variants are the yardstick: ``inside_spread`` says whether the grouped median lies inside the 10th-90th
percentile band of its one-group partner.  Scale 1, finite gradients, no step skipped."""
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
PAIRS = (("one_group", "two_groups"), ("one_group_scaled", "two_groups_scaled"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=50)
    a = ap.parse_args()
    variants, grads = {}, None
    for name in (n for pair in PAIRS for n in pair):
        model, _, _ = harness.build_model(harness.default_cfg(), DEV)         # its own parameters for every optimizer
        params = [p for p in model.parameters() if p.requires_grad]
        if grads is None:
            g = torch.Generator(device=DEV).manual_seed(0)
            grads = [torch.randn(p.shape, device=DEV, generator=g) * 1e-3 for p in params]
        for p, gr in zip(params, grads):
            p.grad = gr.clone()
        if name.startswith("one_group"):
            opt = wsis_optim.FlatAdamW(params, lr=1e-3, weight_decay=1e-4)
        else:
            opt = wsis_optim.FlatAdamW(wsis_optim.split_decay_groups(model, 1e-4), lr=1e-3)
        run = opt.step
        if name.endswith("_scaled"):
            sc = wsis_optim.LossScaler(init_scale=1.0)

            def run(sc=sc, opt=opt):
                sc.step(opt)
                sc.update()
        variants[name] = (run, opt)
    filler = torch.randn(4096, 4096, device=DEV)
    dev_ms, host_ms = {k: [] for k in variants}, {k: [] for k in variants}
    for r in range(5 + a.rounds):                     # five untimed rounds first
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
                if r >= 5:
                    if mode == "queued":
                        dev_ms[name].append(s.elapsed_time(e))
                    else:
                        host_ms[name].append((t1 - t0) * 1e3)
    one = variants["two_groups"][1]
    res = {"tool": "adamw_groups_bench", "device": torch.cuda.get_device_name(0), "rounds": a.rounds,
           "tensors": len(one.params), "parameters": int(one._numel.sum()), "step_bytes": 28 * int(one._numel.sum()),
           "group_sizes": [len(grp["params"]) for grp in one.param_groups]}
    for name, (_, opt) in variants.items():
        d = np.asarray(dev_ms[name]) * 1e3
        res[name] = {"device_us_median": float(np.median(d)), "device_us_min": float(d.min()),
                     "device_us_p10": float(np.percentile(d, 10)), "device_us_p90": float(np.percentile(d, 90)),
                     "host_us_median": float(np.median(host_ms[name])) * 1e3, "groups": len(opt.param_groups),
                     "scaled_entry_point": opt._skipped is not None}
    for base, grouped in PAIRS:
        b, m = res[base], res[grouped]["device_us_median"]
        res[grouped]["minus_one_group_us"] = m - b["device_us_median"]
        res[grouped]["inside_spread"] = bool(b["device_us_p10"] <= m <= b["device_us_p90"])
    assert [res[k]["groups"] for k in variants] == [1, 2, 1, 2]
    assert [res[k]["scaled_entry_point"] for k in variants] == [False, False, True, True]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
