#!/usr/bin/env python3
"""What multi-Krum and the geometric median cost per round on the real arena (DistilBERT: 66.4 M floats),
in ONE process, for M in {2, 4, 8, 16} clients:

    pairdist        ``ops.kernels.robust_pairdist``: M arenas read once, M (M - 1) / 2 sums
    wmean           ``ops.kernels.robust_wmean`` with uniform weights: out + shadow alone, and with the
                    M distances and the non-finite count
    multi_krum      the whole aggregate (pairdist, finalize, wmean) through ``robust_dist_aggregate_``,
                    host read included
    geomed          the whole geometric median at the default 6 iterations (7 passes, 7 finalizers)

each beside the copy rate of this process (``copy_`` of one arena), ``robust_agg`` at the median's k, and
the torch chain of the specification (``torch_multi_krum_`` / ``torch_geometric_median_``) on the device.
Each pass is timed alone with device events (the whole aggregates with the host clock around a
synchronised call); printed: the median / min / max of --reps repetitions after --warmup, the bytes the
pass must move at least, and the GB/s that makes.  No threshold: the script reports what it measures.

    python3 scripts/robust_dist_cost.py > profiles/robust_dist_cost.txt
"""
import argparse
import os
import statistics
import sys
import time
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = "detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd"


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--chain-reps", type=int, default=3)
    ap.add_argument("--layers", type=int, default=6)
    ap.add_argument("--clients", default="2,4,8,16")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from importlib import import_module
    models = import_module(PKG + ".models")
    K = import_module(PKG + ".ops.kernels")
    rd = import_module(PKG + ".parallel.robust_dist")
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
    grid = K.robust_dist_grid(n)
    print(f"arena: {n} floats ({A.n_params} parameters), {4 * n / 1e6:.1f} MB per fp32 stream; "
          f"grid {grid} blocks x 256 lanes, one float4 per source per lane; {args.reps} repetitions after "
          f"{args.warmup} warm-up, device events around the pass alone", flush=True)

    a = torch.randn(4096, 4096, device=dev, dtype=torch.bfloat16)
    t_end = time.perf_counter() + 1.0  # (working clock)
    while time.perf_counter() < t_end:
        for _ in range(20):
            a = (a @ a).clamp_(-1.0, 1.0)
        torch.cuda.synchronize()

    def timed(fn, reps=args.reps, host=False):
        ms = []
        for i in range(args.warmup + reps):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if i >= args.warmup:
                ms.append(1e3 * (time.perf_counter() - t0) if host else e0.elapsed_time(e1))
        return ms

    copy_gbs = [0.0]

    def line(name, ms, nbytes):
        med = statistics.median(ms)
        gbs = nbytes / med / 1e6
        share = f" ({100.0 * gbs / copy_gbs[0]:.0f} % of the copy rate)" if copy_gbs[0] else ""
        print(f"{name:34s} median {med:8.4f} ms  min {min(ms):8.4f}  max {max(ms):8.4f}  {nbytes / 1e6:8.1f} MB  "
              f"{gbs:7.0f} GB/s{share}", flush=True)
        return med

    scratch = torch.empty_like(x0)
    med = line("copy_ of one arena", timed(lambda: scratch.copy_(x0)), 8 * n)
    copy_gbs[0] = 8 * n / med / 1e6
    del scratch
    print()
    ctl = torch.zeros(K.ROBUST_DIST_CTL, device=dev)
    counts = torch.empty(K.ROBUST_AGG_COLS * K.robust_agg_grid(n), dtype=torch.int32, device=dev)
    flat = types.SimpleNamespace(arena=A, mark_shadow_synced=lambda: None)
    res = {}
    for M in ms_list:
        S = states[:M]
        ppart = torch.empty(M * (M - 1) // 2 * grid, dtype=torch.float64, device=dev)
        wpart = torch.empty((M + 1) * grid, dtype=torch.float64, device=dev)
        ctl.zero_()
        ctl[:M] = 1.0 / M
        res[M, "pair"] = line(f"pairdist M {M:2d}", timed(lambda: K.robust_pairdist(S, ppart)), n * 4 * M)
        res[M, "wmean"] = line(f"wmean M {M:2d} out + shadow", timed(
            lambda: K.robust_wmean(S, ctl, A.master, A.shadow, None)), n * (4 * M + 4 + 2))
        res[M, "wmean_d"] = line(f"wmean M {M:2d} out + shadow + dist", timed(
            lambda: K.robust_wmean(S, ctl, A.master, A.shadow, wpart)), n * (4 * M + 4 + 2))
        res[M, "wmean_o"] = line(f"wmean M {M:2d} distances only", timed(
            lambda: K.robust_wmean(S, ctl, None, None, wpart)), n * 4 * M)
        res[M, "agg"] = line(f"robust_agg M {M:2d} k {(M - 1) // 2}", timed(
            lambda: K.robust_agg(S, (M - 1) // 2, A.master, A.shadow, counts)), n * (4 * M + 4 + 2))
        res[M, "krum"] = line(f"multi_krum M {M:2d} (host clock)", timed(
            lambda: rd.robust_dist_aggregate_(flat, S, "multi_krum"), host=True), n * (2 * 4 * M + 4 + 2))
        res[M, "geomed"] = line(f"geomed M {M:2d} 6 it (host clock)", timed(
            lambda: rd.robust_dist_aggregate_(flat, S, "geometric_median"), host=True), n * (7 * 4 * M + 4 + 2))
        f, m = rd.krum_params(M)
        res[M, "krum_t"] = line(f"torch chain multi_krum M {M:2d}", timed(
            lambda: rd.torch_multi_krum_(S, f, m), reps=args.chain_reps, host=True), n * (2 * 4 * M + 4))
        res[M, "geomed_t"] = line(f"torch chain geomed M {M:2d}", timed(
            lambda: rd.torch_geometric_median_(S, 6, 1e-6), reps=args.chain_reps, host=True), n * (7 * 4 * M + 4))
        del ppart, wpart
        print()
    for M in ms_list:
        print(f"M {M:2d}: multi_krum {res[M, 'krum']:.3f} ms = {res[M, 'krum'] / res[M, 'agg']:.1f} x robust_agg (median), "
              f"{res[M, 'krum_t'] / res[M, 'krum']:.0f} x faster than its torch chain; geomed {res[M, 'geomed']:.3f} ms = "
              f"{res[M, 'geomed'] / res[M, 'agg']:.1f} x robust_agg, {res[M, 'geomed_t'] / res[M, 'geomed']:.0f} x faster than "
              f"its torch chain")
    M = max(ms_list)
    pairs = M * (M - 1) // 2
    lane_ops = n * pairs * 3                       # subtract, multiply, add per element and pair
    # 256 CUs x 4 SIMDs x 16 fp32 lanes per clock at 2.4 GHz (the peak vector rate without packed math)
    valu_ms = lane_ops / (256 * 4 * 16 * 2.4e9) * 1e3
    mem_ms = n * 4 * M / copy_gbs[0] / 1e6
    print(f"pairdist M {M}: {lane_ops / 1e9:.1f} G lane-operations = {valu_ms:.3f} ms at the peak fp32 vector rate, "
          f"{n * 4 * M / 1e6:.0f} MB = {mem_ms:.3f} ms at the copy rate, measured {res[M, 'pair']:.3f} ms: the "
          f"{'vector ALU' if valu_ms > mem_ms else 'memory'} term is the larger")
    print(f"peak device memory in this process: {torch.cuda.max_memory_allocated() / 1e9:.2f} GB")
    return 0


if __name__ == "__main__":
    sys.exit(main())
