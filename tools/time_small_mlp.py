"""Time MLPTrainer.step on resident bf16 rows for small nets, fused one-kernel step on and off.

    python tools/time_small_mlp.py [--rows 20000000] [--chunk 2097152] [--repeats 3] [--steps 3]
                                   [--shapes 200-50-1,...,500-64-64-1] [--arms 0,1]

The arms (SHIFU_MLP_FUSED_SMALL=0 / 1) alternate inside one process on the same rows; every
repeat is `--steps` whole steps between two device events.  One JSON line per (shape, arm).
With one arm and --repeats 1 it is the workload for a kernel trace."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from shifu_amd.models.nn import MLPSpec, MLPTrainer, TrainData  # noqa: E402


def resident_rows(spec, n, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.zeros(n, spec.layer_kpad[0], dtype=torch.bfloat16, device=dev)
    for r0 in range(0, n, 1 << 20):                      # chunked: no fp32 copy of the whole shard
        r1 = min(n, r0 + (1 << 20))
        x[r0:r1, : spec.n_in] = torch.randn(r1 - r0, spec.n_in, generator=g, device=dev).bfloat16()
    x[:, spec.n_in] = 1
    y = (x[:, :3].float().sum(1, keepdim=True) > 0).float()
    return TrainData(x, y, None, n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=20_000_000)
    ap.add_argument("--chunk", type=int, default=1 << 21)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--shapes", default="200-50-1,200-45-45-1,400-64-1,300-50-1,400-45-45-1,500-64-64-1")
    ap.add_argument("--arms", default="0,1")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    for shape in a.shapes.split(","):
        dims = [int(v) for v in shape.split("-")]
        spec = MLPSpec(n_in=dims[0], hidden=dims[1:-1], acts=["tanh"] * (len(dims) - 2), n_out=dims[-1])
        data = resident_rows(spec, a.rows, dev)
        trainers = {}
        for arm in a.arms.split(","):
            os.environ["SHIFU_MLP_FUSED_SMALL"] = arm
            trainers[arm] = MLPTrainer(spec, device=dev, seed=1, chunk_rows=a.chunk)
            trainers[arm].step(data)                     # warm-up: code objects, workspaces
        torch.cuda.synchronize()
        ms = {arm: [] for arm in trainers}
        errs = {}
        for _ in range(a.repeats):
            for arm, tr in trainers.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.steps):
                    errs[arm] = tr.step(data)
                e1.record()
                e1.synchronize()
                ms[arm].append(e0.elapsed_time(e1) / a.steps)
        for arm, tr in trainers.items():
            v = sorted(ms[arm])
            print(json.dumps({"shape": shape, "fused_small_env": int(arm), "fused_small": bool(tr.fused_small),
                              "rows": a.rows, "chunk": a.chunk, "ms_per_step": [round(t, 3) for t in ms[arm]],
                              "median_ms": round(v[len(v) // 2], 3), "spread_ms": round(v[-1] - v[0], 3),
                              "rows_per_s": round(a.rows / (v[len(v) // 2] * 1e-3)), "last_error": errs[arm]}),
                  flush=True)
        del data, trainers


if __name__ == "__main__":
    main()
