#!/usr/bin/env python3
"""What the quantized update exchange costs per round on the real arena (DistilBERT: 66.4 M floats),
in ONE process beside a device copy, the pass a round makes today, and the same arithmetic as a chain
of torch ops:

    copy      ``dst.copy_(src)`` of the fp32 arena: the device copy rate of this process
    plain     ``scale_cast(master, shadow, 1 / N)``: plain FedAvg's finalisation
    encode    ``ops.kernels.quant_encode`` (+ its one-block finalize) with a residual, at int8 and int4,
              nearest and stochastic
    decode    ``ops.kernels.quant_decode_mean`` with the bf16 shadow, M = 2 / 4 / 8 / 16, int8 and int4
    torch     the chains that compute the same thing with torch ops on the device (encode: sub, add,
              abs, amax, two divisions, mul, add, floor, clamp, mul, sub, the pack, two norms;
              stochastic: ``torch.rand`` for the uniforms; decode: per payload unpack, scale, add)

Each pass is timed alone with device events; printed: the median / min / max of --reps repetitions
after --warmup, the bytes the pass must move at least, and the GB/s that makes as a share of the copy
rate measured here.  No time is fixed in advance; the condition is that every kernel beats its torch
chain of this same process (exit status 2 otherwise).  The ratios are reported, not asserted.

    python3 scripts/compress_cost.py > profiles/compress_cost.txt
"""
import argparse
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = "detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd"
SEED = 0x5EEDF00DCAFE


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--layers", type=int, default=6)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from importlib import import_module
    models = import_module(PKG + ".models")
    K = import_module(PKG + ".ops.kernels")
    cp = import_module(PKG + ".parallel.compress")
    if not torch.cuda.is_available():
        print("no GPU: nothing measured", flush=True)
        return 1
    dev = torch.device("cuda")
    model = models.DDoSClassifier(config=models.DistilBertConfig(n_layers=args.layers), device=dev, impl="hip", seed=0)
    A = model.arena
    n = A.numel
    g = torch.Generator(device=dev).manual_seed(1)
    anchor = A.master.clone()
    live = anchor != 0
    w = anchor + 1e-4 * torch.randn(n, device=dev, generator=g) * live
    e0 = 1e-6 * torch.randn(n, device=dev, generator=g) * live
    e = e0.clone()
    grid = K.quant_grid(n)
    partial = torch.empty(3 * grid, dtype=torch.float64, device=dev)
    stats = torch.empty(4, dtype=torch.float64, device=dev)
    print(f"arena: {n} floats ({A.n_params} parameters), {4 * n / 1e6:.1f} MB per fp32 stream, {n // 64} groups of 64; "
          f"grid {grid} blocks x 256 lanes, 32 bits of codes per lane per iteration; {args.reps} repetitions after "
          f"{args.warmup} warm-up, device events around the pass alone", flush=True)
    print(f"payload: int8 {4 * K.quant_words(n, 8) / 1e6:.1f} MB ({cp.payload_ratio(8):.2f}x smaller), int4 "
          f"{4 * K.quant_words(n, 4) / 1e6:.1f} MB ({cp.payload_ratio(4):.2f}x smaller)\n", flush=True)

    a = torch.randn(4096, 4096, device=dev, dtype=torch.bfloat16)
    t_end = time.perf_counter() + 1.0  # (working clock)
    while time.perf_counter() < t_end:
        for _ in range(20):
            a = (a @ a).clamp_(-1.0, 1.0)
        torch.cuda.synchronize()
    del a

    def timed(fn, prepare=None):
        ms = []
        for i in range(args.warmup + args.reps):
            if prepare is not None:
                prepare()
            e0_, e1_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0_.record()
            fn()
            e1_.record()
            torch.cuda.synchronize()
            if i >= args.warmup:
                ms.append(e0_.elapsed_time(e1_))
        return ms

    copy_gbs = [None]

    def line(name, ms, nbytes):
        med = statistics.median(ms)
        gbs = nbytes / med / 1e6
        share = "" if copy_gbs[0] is None else f" ({100.0 * gbs / copy_gbs[0]:.0f} % of the copy rate)"
        print(f"{name:38s} median {med:.4f} ms  min {min(ms):.4f}  max {max(ms):.4f}  {nbytes / 1e6:8.1f} MB  "
              f"{gbs:7.0f} GB/s{share}", flush=True)
        return med

    dst = torch.empty_like(w)
    t_copy = line("device copy (fp32 arena)", timed(lambda: dst.copy_(w)), n * 8)
    copy_gbs[0] = n * 8 / t_copy / 1e6
    del dst
    dst = w.clone()
    line("plain scale_cast", timed(lambda: K.scale_cast(dst, A.shadow, 0.125)), n * (4 + 4 + 2))
    del dst
    print()

    def restore():
        e.copy_(e0)

    lost = []
    enc = {}
    for bits in (8, 4):
        words = K.quant_words(n, bits)
        payload = torch.empty(words, dtype=torch.int32, device=dev)
        qmax = float(cp.QMAX[bits])
        nbytes = n * (4 + 4 + 4 + 4) + 4 * words   # w, anchor, residual read; residual, payload written
        for rounding in ("nearest", "stochastic"):
            st = rounding == "stochastic"
            t_k = line(f"quant_encode int{bits} {rounding}", timed(
                lambda: K.quant_encode(w, anchor, e, payload, partial, stats, bits, st, SEED, 0, 0), restore), nbytes)
            enc[(bits, rounding)] = t_k

            def chain():
                v = (w - anchor) + e
                gv = v.view(-1, 64)
                amax = gv.abs().amax(dim=1)
                inv = qmax / amax
                empty = ~torch.isfinite(inv)
                s = torch.where(empty, 0.0, amax / qmax)
                inv = torch.where(empty, 0.0, inv)
                u = torch.rand(n // 64, 64, device=dev) if st else 0.5
                f = torch.floor(gv * inv.unsqueeze(1) + u).clamp_(-qmax, qmax)
                err = gv - s.unsqueeze(1) * f
                e.copy_(err.view(-1))
                if bits == 8:
                    payload[:n // 4].copy_(f.to(torch.int8).view(-1).view(torch.int32))
                else:
                    q = f.to(torch.int32).view(-1, 8) & 15
                    payload[:n // 8].copy_((q << torch.arange(0, 32, 4, device=dev, dtype=torch.int32)).sum(dim=1,
                                                                                                          dtype=torch.int32))
                payload[words - n // 64:].copy_(s.view(torch.int32))
                stats[0] = torch.linalg.vector_norm(v, dtype=torch.float64)
                stats[1] = torch.linalg.vector_norm(err, dtype=torch.float64)

            t_c = line(f"  torch chain, int{bits} {rounding}", timed(chain, restore), nbytes)
            print(f"  -> the kernel is {t_c / t_k:.1f} x faster than its torch chain"
                  + ("" if t_k < t_c else "   ** SLOWER: condition missed **"), flush=True)
            if not t_k < t_c:
                lost.append(f"quant_encode int{bits} {rounding}")
        del payload
    print()
    out = torch.empty(n, device=dev)
    for bits in (8, 4):
        words = K.quant_words(n, bits)
        qmax = float(cp.QMAX[bits])
        ps = []
        for c in range(16):
            p = torch.empty(words, dtype=torch.int32, device=dev)
            wk = anchor + 1e-4 * (1 + c) * torch.randn(n, device=dev, generator=g) * live
            K.quant_encode(wk, anchor, None, p, partial, stats, bits, False, SEED, 0, c)
            ps.append(p)
            del wk
        for M in (2, 4, 8, 16):
            nbytes = 4 * words * M + n * (4 + 4 + 2)
            t_k = line(f"quant_decode_mean int{bits} M = {M}", timed(
                lambda: K.quant_decode_mean(ps[:M], anchor, out, A.shadow, bits)), nbytes)
            inv = 1.0 / M

            def chain():
                acc = torch.zeros(n // 64, 64, device=dev)
                for p in ps[:M]:
                    s = p[words - n // 64:].view(torch.float32)
                    if bits == 8:
                        q = p[:n // 4].view(torch.int8).to(torch.float32)
                    else:
                        u = (p[:n // 8].unsqueeze(1) >> torch.arange(0, 32, 4, device=dev, dtype=torch.int32)) & 15
                        q = torch.where(u >= 8, u - 16, u).to(torch.float32)
                    acc = acc + q.view(-1, 64) * s.unsqueeze(1)
                out.copy_(anchor + acc.view(-1) * inv)
                A.shadow.copy_(out)

            t_c = line(f"  torch chain, int{bits} M = {M}", timed(chain), nbytes)
            print(f"  -> the kernel is {t_c / t_k:.1f} x faster than its torch chain"
                  + ("" if t_k < t_c else "   ** SLOWER: condition missed **"), flush=True)
            if not t_k < t_c:
                lost.append(f"quant_decode_mean int{bits} M = {M}")
        del ps
    model.sync_shadow(force=True)
    print()
    print(f"the copy rate of this process: {copy_gbs[0]:.0f} GB/s ({t_copy:.4f} ms for {n * 8 / 1e6:.1f} MB)")
    print(f"stochastic rounding adds {enc[(8, 'stochastic')] - enc[(8, 'nearest')]:+.4f} ms at int8 and "
          f"{enc[(4, 'stochastic')] - enc[(4, 'nearest')]:+.4f} ms at int4 (one Philox4x32-10 block per float4)")
    print("condition (every kernel beats its torch chain in this process): "
          + ("met" if not lost else "MISSED by " + ", ".join(lost)))
    print(f"peak device memory in this process: {torch.cuda.max_memory_allocated() / 1e9:.2f} GB")
    return 2 if lost else 0


if __name__ == "__main__":
    sys.exit(main())
