#!/usr/bin/env python3
"""What the FedOpt server step costs per round on the real arena (DistilBERT: 66.4 M floats), three
ways in ONE process:

    fused   ``ops.kernels.server_opt``, one launch per kind (master, x, m[, v] read and written once,
            the bf16 shadow written, the two statistics reduced)
    plain   ``scale_cast(master, shadow, 1 / N)``: plain FedAvg's finalisation, what the round costs
            without a server optimizer
    torch   the same arithmetic as fp32 torch ops on the device (``parallel.server_opt.torch_chain_``,
            plus the copy into the master and the bf16 cast the fused pass includes)

Each repetition restores the master from a saved sum outside the timed region and times the pass
alone with device events; printed: the median / min / max of --reps repetitions after --warmup, the
bytes the pass must move at least, and the GB/s that makes beside the ~6.3 TB/s a float4 copy
reaches on this GPU.  No threshold: the script reports what it measures.

    python3 scripts/server_opt_cost.py > profiles/server_opt_cost.txt
"""
import argparse
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = "detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd"
COPY_TBS = 6.3  # float4 copy, measured (the microarchitecture notes' HBM figure)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--layers", type=int, default=6)
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
    nclients = 8
    g = torch.Generator(device=dev).manual_seed(1)
    x0 = A.master.clone()
    live = x0 != 0
    s0 = nclients * (x0 + 1e-3 * torch.randn(n, device=dev, generator=g) * live)  # the all-reduced sum
    inv = so.f32(1.0 / nclients)
    b1, b2, tau = so.f32(0.9), so.f32(0.99), so.f32(1e-3)
    stats = torch.zeros(2 * K.server_opt_grid(n), device=dev)
    print(f"arena: {n} floats ({A.n_params} parameters), {4 * n / 1e6:.1f} MB per fp32 stream; "
          f"grid {K.server_opt_grid(n)} blocks x 256 lanes, float4 per lane; {args.reps} repetitions after "
          f"{args.warmup} warm-up, device events around the pass alone", flush=True)

    a = torch.randn(4096, 4096, device=dev, dtype=torch.bfloat16)
    t_end = time.perf_counter() + 1.0  # (working clock)
    while time.perf_counter() < t_end:
        for _ in range(20):
            a = (a @ a).clamp_(-1.0, 1.0)
        torch.cuda.synchronize()

    def timed(fn, prepare):
        ms = []
        for i in range(args.warmup + args.reps):
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
        gbs = nbytes / med / 1e6 if nbytes else 0.0
        tail = f"  {nbytes / 1e6:8.1f} MB  {gbs:7.0f} GB/s ({100.0 * gbs / (COPY_TBS * 1e3):.0f} % of {COPY_TBS} TB/s)" \
            if nbytes else "  (a dozen passes and temporaries: no single byte count)"
        print(f"{name:22s} median {med:.4f} ms  min {min(ms):.4f}  max {max(ms):.4f}{tail}", flush=True)
        return med

    res = {}
    x, m, v = x0.clone(), torch.zeros_like(x0), torch.zeros_like(x0)

    def restore(kind):
        def f():
            A.master.copy_(s0)
            x.copy_(x0)
            m.zero_()
            v.fill_(so.f32(tau * tau))
        return f

    res["plain"] = line("plain scale_cast", timed(lambda: K.scale_cast(A.master, A.shadow, inv), restore(None)),
                        n * (4 + 4 + 2))
    for kind in so.KINDS:
        eta = so.f32(1.0 if kind == "avgm" else 0.01)
        vv = None if kind == "avgm" else v
        streams = 3 if kind == "avgm" else 4
        res[kind] = line(f"fused {kind}", timed(
            lambda: K.server_opt(A.master, x, m, vv, A.shadow, kind, inv, eta, b1, b2, tau, stats), restore(kind)),
            n * (8 * streams + 2))
        res[kind + "_nostats"] = line(f"fused {kind}, no stats", timed(
            lambda: K.server_opt(A.master, x, m, vv, A.shadow, kind, inv, eta, b1, b2, tau, None), restore(kind)),
            n * (8 * streams + 2))

        def chain():
            so.torch_chain_(kind, A.master, x, m, vv, inv, eta, b1, b2, tau)
            A.master.copy_(x)
            A.shadow.copy_(x)
        res[kind + "_torch"] = line(f"torch {kind}", timed(chain, restore(kind)), 0)
    print()
    for kind in so.KINDS:
        f, t, p = res[kind], res[kind + "_torch"], res["plain"]
        print(f"{kind:8s} torch chain / fused {t / f:.2f}   fused - plain FedAvg "
              f"{f - p:+.4f} ms per round   statistics {f - res[kind + '_nostats']:+.4f} ms")
    print(f"peak device memory in this process: {torch.cuda.max_memory_allocated() / 1e9:.2f} GB")
    return 0


if __name__ == "__main__":
    sys.exit(main())
