#!/usr/bin/env python3
"""What secure aggregation costs per round on the real arena (DistilBERT: 66.4 M floats), in ONE process
beside a device copy, the pass a round makes today, and the same arithmetic as a chain of torch ops:

    copy      ``dst.copy_(src)`` of the fp32 arena: the device copy rate of this process
    plain     ``scale_cast(master, shadow, 1 / N)``: plain FedAvg's finalisation
    mask      ``ops.kernels.secagg_mask`` (+ its one-block finalize) without partners (the quantizer alone)
              and at M = 2 / 4 / 8 / 16 clients (P = M - 1 streams per element), at 8 / 12 / 20 ChaCha rounds
    stream    ``ops.kernels.secagg_stream``: the generator alone, one stream, 8 / 12 / 20 rounds
    unmask    ``ops.kernels.secagg_unmask_mean`` with the bf16 shadow, M = 2 / 4 / 8 / 16
    torch     the chains that compute the same thing with torch ops on the device (quantize: sub, mul,
              round, the clamp, the cast, two norms; unmask: the int32 sum, the cast, two muls, the add,
              the shadow) -- torch has no ChaCha, so the masked passes have no chain beside them

Each pass is timed alone with device events; printed: the median / min / max of --reps repetitions
after --warmup, the bytes the pass must move at least and the GB/s that makes as a share of the copy
rate measured here, and for the masked passes the integer lane-operations per second that the time
implies at 976 * rounds / 20 operations per 16-word block (4 adds, 4 xors, 4 rotates per quarter round,
8 quarter rounds per double round, 16 final adds), against the 78.6 T lane-ops/s a vector ALU that
issued every cycle would reach.  No time is fixed in advance; the condition is that the quantizer and
the unmask pass beat their torch chains of this same process (exit status 2 otherwise).

    python3 scripts/secagg_cost.py > profiles/secagg_cost.txt
"""
import argparse
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = "detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd"
PEAK_LANE_OPS = 78.6e12


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--layers", type=int, default=6)
    ap.add_argument("--frac-bits", type=int, default=24)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from importlib import import_module
    models = import_module(PKG + ".models")
    K = import_module(PKG + ".ops.kernels")
    if not torch.cuda.is_available():
        print("no GPU: nothing measured", flush=True)
        return 1
    dev = torch.device("cuda")
    f = args.frac_bits
    model = models.DDoSClassifier(config=models.DistilBertConfig(n_layers=args.layers), device=dev, impl="hip", seed=0)
    A = model.arena
    n = A.numel
    g = torch.Generator(device=dev).manual_seed(1)
    anchor = A.master.clone()
    live = anchor != 0
    w = anchor + 1e-4 * torch.randn(n, device=dev, generator=g) * live
    grid = K.secagg_grid(n)
    words = K.secagg_words(n)
    partial = torch.empty(4 * grid, dtype=torch.float64, device=dev)
    stats = torch.empty(4, dtype=torch.float64, device=dev)
    keys = torch.from_numpy(np.random.default_rng(0).integers(-2 ** 31, 2 ** 31, size=(15, 8), dtype=np.int64)
                            .astype(np.int32)).to(dev)
    print(f"arena: {n} floats ({A.n_params} parameters), {4 * n / 1e6:.1f} MB per fp32 stream, {n // 16} ChaCha blocks "
          f"per stream; grid {grid} blocks x 256 lanes, one float4 per lane per iteration, a quad of lanes per block; "
          f"{f} fraction bits; {args.reps} repetitions after {args.warmup} warm-up, device events around the pass alone",
          flush=True)
    print(f"payload: {4 * words / 1e6:.1f} MB per client (the fp32 master's size plus a 64-byte check block)\n", flush=True)

    a = torch.randn(4096, 4096, device=dev, dtype=torch.bfloat16)
    t_end = time.perf_counter() + 1.0  # (working clock)
    while time.perf_counter() < t_end:
        for _ in range(20):
            a = (a @ a).clamp_(-1.0, 1.0)
        torch.cuda.synchronize()
    del a

    def timed(fn):
        ms = []
        for i in range(args.warmup + args.reps):
            e0_, e1_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0_.record()
            fn()
            e1_.record()
            torch.cuda.synchronize()
            if i >= args.warmup:
                ms.append(e0_.elapsed_time(e1_))
        return ms

    copy_gbs = [None]

    def line(name, ms, nbytes, ops=0.0):
        med = statistics.median(ms)
        gbs = nbytes / med / 1e6
        share = "" if copy_gbs[0] is None else f" ({100.0 * gbs / copy_gbs[0]:.0f} % of the copy rate)"
        alu = "" if not ops else f"  {ops / med / 1e9:6.1f} T lane-ops/s ({100.0 * ops / med / 1e-3 / PEAK_LANE_OPS:.0f} % of 78.6 T)"
        print(f"{name:38s} median {med:.4f} ms  min {min(ms):.4f}  max {max(ms):.4f}  {nbytes / 1e6:8.1f} MB  "
              f"{gbs:7.0f} GB/s{share}{alu}", flush=True)
        return med

    dst = torch.empty_like(w)
    t_copy = line("device copy (fp32 arena)", timed(lambda: dst.copy_(w)), n * 8)
    copy_gbs[0] = n * 8 / t_copy / 1e6
    del dst
    dst = w.clone()
    line("plain scale_cast", timed(lambda: K.scale_cast(dst, A.shadow, 0.125)), n * (4 + 4 + 2))
    del dst
    print()

    lost = []
    payload = torch.empty(words, dtype=torch.int32, device=dev)
    nbytes = n * (4 + 4) + 4 * words   # w, anchor read; the payload written
    t_q = line("secagg_mask without partners", timed(
        lambda: K.secagg_mask(w, anchor, keys[:0], 0, payload, partial, stats, f, 20, 0)), nbytes)
    scale, qmax = 2.0 ** f, float((1 << 27) - 1)

    def quant_chain():
        d = w - anchor
        r = torch.round(d * scale)
        q = r.clamp(-qmax, qmax).to(torch.int32)
        payload[:n].copy_(q)
        e = d - q.to(torch.float32) * (1.0 / scale)
        stats[0] = torch.linalg.vector_norm(d, dtype=torch.float64)
        stats[1] = torch.linalg.vector_norm(e, dtype=torch.float64)

    t_c = line("  torch chain, the quantizer", timed(quant_chain), nbytes)
    print(f"  -> the kernel is {t_c / t_q:.1f} x faster than its torch chain"
          + ("" if t_q < t_c else "   ** SLOWER: condition missed **"), flush=True)
    if not t_q < t_c:
        lost.append("secagg_mask without partners")
    print()
    mask_ms = {}
    for rounds in (20, 12, 8):
        per_block = 976.0 * rounds / 20.0
        for M in (2, 4, 8, 16):
            P = M - 1
            ops = (n + 16) / 16.0 * P * per_block
            mask_ms[(rounds, M)] = line(f"secagg_mask M = {M:2d} (P = {P:2d}), ChaCha{rounds}", timed(
                lambda: K.secagg_mask(w, anchor, keys[:P], 0x2AAA & ((1 << P) - 1), payload, partial, stats, f, rounds, 3)),
                nbytes, ops)
        print()
    so = torch.empty(n, dtype=torch.int32, device=dev)
    for rounds in (20, 12, 8):
        line(f"secagg_stream, ChaCha{rounds}", timed(lambda: K.secagg_stream(so, keys[0], (3, 0, 0), rounds, 0)), 4 * n,
             n / 16.0 * 976.0 * rounds / 20.0)
    del so
    print()
    out = torch.empty(n, device=dev)
    ps = []
    for c in range(16):
        p = torch.empty(words, dtype=torch.int32, device=dev)
        wk = anchor + 1e-4 * (1 + c) * torch.randn(n, device=dev, generator=g) * live
        K.secagg_mask(wk, anchor, keys[:0], 0, p, partial, stats, f, 20, 0)
        ps.append(p)
        del wk
    for M in (2, 4, 8, 16):
        nb = 4 * n * M + n * (4 + 4 + 2)
        t_k = line(f"secagg_unmask_mean M = {M}", timed(
            lambda: K.secagg_unmask_mean(ps[:M], anchor, out, A.shadow, f)), nb)
        inv = 1.0 / M

        def chain():
            s = ps[0][:n].clone()
            for p in ps[1:M]:
                s += p[:n]                      # (int32 adds wrap)
            out.copy_(anchor + (s.to(torch.float32) * (1.0 / scale)) * inv)
            A.shadow.copy_(out)

        t_c = line(f"  torch chain, M = {M}", timed(chain), nb)
        print(f"  -> the kernel is {t_c / t_k:.1f} x faster than its torch chain"
              + ("" if t_k < t_c else "   ** SLOWER: condition missed **"), flush=True)
        if not t_k < t_c:
            lost.append(f"secagg_unmask_mean M = {M}")
    del ps
    model.sync_shadow(force=True)
    print()
    print(f"the copy rate of this process: {copy_gbs[0]:.0f} GB/s ({t_copy:.4f} ms for {n * 8 / 1e6:.1f} MB)")
    print("the hypothesis (arithmetic only: 61 lane-ops per element and partner at 20 rounds, issued at 78.6 T/s, "
          "beside 12 B per element at the copy rate): 0.05 / 0.36 / 0.8 ms at M = 2 / 8 / 16, ALU-bound from about "
          "three partners on")
    print("measured at ChaCha20: " + ", ".join(f"M = {M}: {mask_ms[(20, M)]:.3f} ms" for M in (2, 4, 8, 16))
          + f"; per added partner between M = 8 and M = 16: {(mask_ms[(20, 16)] - mask_ms[(20, 8)]) / 8:.4f} ms")
    print("condition (the quantizer and the unmask pass beat their torch chains in this process): "
          + ("met" if not lost else "MISSED by " + ", ".join(lost)))
    print(f"peak device memory in this process: {torch.cuda.max_memory_allocated() / 1e9:.2f} GB")
    return 2 if lost else 0


if __name__ == "__main__":
    sys.exit(main())
