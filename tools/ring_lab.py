"""Forward-GEMM engine comparison at the bench's first layer (2M-row chunk x 1024 -> 512, sigmoid +
bias column): times the persistent ring forward (gemm_ring_nt.hip) against the 8-phase kernel in
interleaved rounds of one process.  One JSON line per engine and round.  tools/pmc_ring.sh runs
it under the counter collection.

    python tools/ring_lab.py [--rows 2097152] [--k 1024] [--n 512] [--iters 10] [--rounds 2]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 21)
    ap.add_argument("--k", type=int, default=1024)
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--nv", type=int, default=500)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=2)
    a = ap.parse_args()
    import torch
    from shifu_amd.ops import _native as nat
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(3)
    M, K, N = a.rows, a.k, a.n
    A = torch.empty(M, K, dtype=torch.bfloat16, device=dev)
    A.normal_(generator=g)
    B = (torch.randn(N, K, device=dev, generator=g) * 0.05).to(torch.bfloat16)
    C = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
    st = nat.stream_of(A)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * a.iters)]

    def launch():
        r = nat.call_hip("shifu_gemm_nt", A, K, B, K, a.nv, C, N, None, 0, None, 0, None, 0,
                         M, N, K, 0, 0, a.nv, 1, 0.0, st)
        assert r == 0, r

    def timed():
        launch()
        torch.cuda.synchronize()
        for i in range(a.iters):
            ev[2 * i].record()
            launch()
            ev[2 * i + 1].record()
        torch.cuda.synchronize()
        ts = sorted(ev[2 * i].elapsed_time(ev[2 * i + 1]) for i in range(a.iters))
        return ts[len(ts) // 2], ts[0]

    flop = 2.0 * M * K * a.nv
    nat.call_hip("shifu_gemm_set_tune", 14, 0)      # the strip engine would take the shape first
    for rnd in range(a.rounds):
        for name, ring in (("8phase", 0), ("ring", 1)):
            nat.call_hip("shifu_gemm_set_tune", 12, ring)
            med, mn = timed()
            print(json.dumps({"variant": name, "round": rnd, "ms_median": round(med, 4), "ms_min": round(mn, 4),
                              "tflops_median": round(flop / med / 1e9, 1), "M": M, "K": K, "N": N}), flush=True)
    nat.call_hip("shifu_gemm_set_tune", 12, 1)
    nat.call_hip("shifu_gemm_set_tune", 14, 1)


if __name__ == "__main__":
    main()
