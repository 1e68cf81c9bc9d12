#!/usr/bin/env python3
"""What the robust aggregate costs per round on the real arena (DistilBERT: 66.4 M floats), in ONE
process beside the two passes a round makes today:

    robust  ``ops.kernels.robust_agg`` for M in {2, 4, 8, 16} clients, at k = 0 (the mean summed in
            sorted order) and at the median's k = (M - 1) // 2: M arenas read once, the master and the
            bf16 shadow written, the trimmed counts reduced
    plain   ``scale_cast(master, shadow, 1 / N)``: plain FedAvg's finalisation
    server  ``server_opt`` (adam): the FedOpt finalisation

Each pass is timed alone with device events; printed: the median / min / max of --reps repetitions
after --warmup, the bytes the pass must move at least, and the GB/s that makes beside the 6.29 TB/s a
float4 copy reaches on this GPU.  No threshold: the script reports what it measures.

    python3 scripts/robust_agg_cost.py > profiles/robust_agg_cost.txt
"""
import argparse
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = "detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd"
COPY_TBS = 6.29  # float4 copy, measured (the microarchitecture notes' HBM figure)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--layers", type=int, default=6)
    ap.add_argument("--clients", default="2,4,8,16")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from importlib import import_module
    models = import_module(PKG + ".models")
    K = import_module(PKG + ".ops.kernels")
    so = import_module(PKG + ".parallel.server_opt")
    if not torch.cuda.is_available():
        print("no GPU: nothing measured", flush=True)
        return 1
    dev = torch.device("cuda")
    model = models.DDoSClassifier(config=models.DistilBertConfig(n_layers=args.layers), device=dev, impl="hip", seed=0)
    A = model.arena
    n = A.numel
    ms_list = [int(m) for m in args.clients.split(",")]
    g = torch.Generator(device=dev).manual_seed(1)
    x0 = A.master.clone()
    live = x0 != 0
    states = [x0 + 1e-3 * torch.randn(n, device=dev, generator=g) * live for _ in range(max(ms_list))]
    grid = K.robust_agg_grid(n)
    counts = torch.empty(K.ROBUST_AGG_COLS * grid, dtype=torch.int32, device=dev)
    print(f"arena: {n} floats ({A.n_params} parameters), {4 * n / 1e6:.1f} MB per fp32 stream; "
          f"grid {grid} blocks x 256 lanes, one float4 per source per lane; {args.reps} repetitions after "
          f"{args.warmup} warm-up, device events around the pass alone", flush=True)

    a = torch.randn(4096, 4096, device=dev, dtype=torch.bfloat16)
    t_end = time.perf_counter() + 1.0  # (working clock)
    while time.perf_counter() < t_end:
        for _ in range(20):
            a = (a @ a).clamp_(-1.0, 1.0)
        torch.cuda.synchronize()

    def timed(fn, prepare=None):
        ms = []
        for i in range(args.warmup + args.reps):
            if prepare is not None:
                prepare()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if i >= args.warmup:
                ms.append(e0.elapsed_time(e1))
        return ms

    def line(name, ms, nbytes):
        med = statistics.median(ms)
        gbs = nbytes / med / 1e6
        print(f"{name:30s} median {med:.4f} ms  min {min(ms):.4f}  max {max(ms):.4f}  {nbytes / 1e6:8.1f} MB  "
              f"{gbs:7.0f} GB/s ({100.0 * gbs / (COPY_TBS * 1e3):.0f} % of {COPY_TBS} TB/s)", flush=True)
        return med

    s0 = 8 * states[0]
    inv = so.f32(1.0 / 8)
    plain = line("plain scale_cast", timed(lambda: K.scale_cast(A.master, A.shadow, inv), lambda: A.master.copy_(s0)),
                 n * (4 + 4 + 2))
    x, m, v = x0.clone(), torch.zeros_like(x0), torch.zeros_like(x0)
    stats = torch.zeros(2 * K.server_opt_grid(n), device=dev)
    b1, b2, tau = so.f32(0.9), so.f32(0.99), so.f32(1e-3)

    def restore():
        A.master.copy_(s0)
        x.copy_(x0)
        m.zero_()
        v.fill_(so.f32(tau * tau))

    server = line("server_opt adam", timed(
        lambda: K.server_opt(A.master, x, m, v, A.shadow, "adam", inv, so.f32(0.01), b1, b2, tau, stats), restore),
        n * (8 * 4 + 2))
    del x, m, v
    print()
    res = {}
    for M in ms_list:
        for k in sorted({0, (M - 1) // 2}):
            res[M, k] = line(f"robust_agg M {M:2d} k {k}", timed(
                lambda: K.robust_agg(states[:M], k, A.master, A.shadow, counts)), n * (4 * M + 4 + 2))
        k = (M - 1) // 2
        res[M, "nocounts"] = line(f"robust_agg M {M:2d} k {k}, no counts", timed(
            lambda: K.robust_agg(states[:M], k, A.master, A.shadow, None)), n * (4 * M + 4 + 2))
    print()
    for M in ms_list:
        k = (M - 1) // 2
        print(f"M {M:2d}: median pass {res[M, k]:.4f} ms = {res[M, k] / plain:.1f} x plain scale_cast, "
              f"{res[M, k] / server:.1f} x server_opt adam; counts {res[M, k] - res[M, 'nocounts']:+.4f} ms")
    sums = counts.view(-1, K.ROBUST_AGG_COLS).sum(dim=0, dtype=torch.int64).tolist()
    print(f"last launch: trimmed share per slot {[round(t / n, 4) for t in sums[:ms_list[-1]]]}, non-finite {sums[-1]}")
    print(f"peak device memory in this process: {torch.cuda.max_memory_allocated() / 1e9:.2f} GB")
    return 0


if __name__ == "__main__":
    sys.exit(main())
