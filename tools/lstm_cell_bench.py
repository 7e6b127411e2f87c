"""LSTMCellEx alone: the fused kernels (csrc/lstm.hip) against the module walk (``LSTMCellEx.forward_reference``) on the
device, forward and forward + backward, at S = 2,289 rows (one scene's superpoints) and 9,156 (four scenes).  Median of
30 runs between device events after 5 warm-up runs; writes profiles/lstm_cell_bench.json.

    python tools/lstm_cell_bench.py [OUTPUT.json]
"""
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
importlib.import_module("3d-wsis_amd")
import torch                 # noqa: E402
import graphnet              # noqa: E402

RUNS, WARMUP = 30, 5


def median_us(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(RUNS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    return statistics.median(times)


def main():
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    cell = graphnet.LSTMCellEx(32, 32, bias=True, layernorm=True, ingate=True).to(dev)
    res = {"device": torch.cuda.get_device_name(0), "runs": RUNS, "warmup": WARMUP, "unit": "us (median)", "rows": {}}
    for S in (2289, 9156):
        x, h, c = (torch.randn(S, 32, device=dev, requires_grad=True) for _ in range(3))
        dhy, dcy = torch.randn(S, 32, device=dev), torch.randn(S, 32, device=dev)

        def fwd(f):
            with torch.no_grad():
                f(x, (h, c))

        def fwd_bwd(f):
            hy, cy = f(x, (h, c))
            torch.autograd.backward([hy, cy], [dhy, dcy])
            x.grad = h.grad = c.grad = None
            cell.zero_grad(set_to_none=True)

        row = {}
        for name, f in (("fused", cell), ("module_walk", cell.forward_reference)):
            row[name] = {"fwd": median_us(lambda: fwd(f)), "fwd_bwd": median_us(lambda: fwd_bwd(f))}
        row["speedup_fwd"] = row["module_walk"]["fwd"] / row["fused"]["fwd"]
        row["speedup_fwd_bwd"] = row["module_walk"]["fwd_bwd"] / row["fused"]["fwd_bwd"]
        res["rows"][str(S)] = row
        print(S, json.dumps(row))
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "lstm_cell_bench.json")
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
