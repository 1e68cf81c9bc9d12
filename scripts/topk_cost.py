#!/usr/bin/env python3
"""What the top-k sparsified update exchange costs per round on the real arena (DistilBERT: 66.4 M
floats), in ONE process beside a device copy and the same arithmetic as a chain of torch ops:

    copy      ``dst.copy_(src)`` of the fp32 arena: the device copy rate of this process
    encode    ``ops.kernels.topk_encode`` (its whole sequence of launches) with a residual, at densities
              0.1 / 0.01 / 0.001
    passes    the device time of each launch of one encode at density 0.01 (torch.profiler's kernel
              records), with the bytes the pass must move and their share of the copy rate
    decode    ``ops.kernels.topk_decode_mean`` with the bf16 shadow, M = 2 / 4 / 8 / 16 at density 0.01
    torch     the chains that compute the same thing with torch ops on the device (encode: sub, add,
              abs, ``topk``, a sort of the indices, gather, the residual by scatter, the chunk offsets by
              ``bincount`` + ``cumsum``, the index pack, two norms; decode: per payload a scatter-add of
              its entries into a dense accumulator).  The chain does not break ties by index and does
              not treat inf / NaN: it does less than the kernel.

Each pass is timed alone with device events; printed: the median / min / max of --reps repetitions
after --warmup (the torch chains: --chain-reps), the bytes the pass must move at least, and the GB/s
that makes as a share of the copy rate measured here.  No time is fixed in advance; the condition is
that every kernel beats its torch chain of this same process (exit status 2 otherwise).  The ratios
are reported, not asserted.

    python3 scripts/topk_cost.py > profiles/topk_cost.txt
"""
import argparse
import os
import re
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = "detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd"
CHUNK = 4096


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--chain-reps", type=int, default=5)
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
    C = (n + CHUNK - 1) // CHUNK
    g = torch.Generator(device=dev).manual_seed(1)
    anchor = A.master.clone()
    live = anchor != 0
    # a round's update: dense over the encoder, and only one word-embedding row in eight touched
    name, (off, shape) = next((k, v) for k, v in A.offsets.items() if "word" in k)
    rows = torch.rand(shape[0], device=dev, generator=g) < 0.125
    touched = live.clone()
    touched[off:off + shape[0] * shape[1]] &= rows.repeat_interleave(shape[1])
    w = anchor + 1e-4 * torch.randn(n, device=dev, generator=g) * touched
    e0 = 1e-6 * torch.randn(n, device=dev, generator=g) * touched
    e = e0.clone()
    del live, rows
    work = torch.empty(K.topk_work_bytes(n), dtype=torch.uint8, device=dev)
    stats = torch.empty(8, dtype=torch.float64, device=dev)
    print(f"arena: {n} floats ({A.n_params} parameters), {4 * n / 1e6:.1f} MB per fp32 stream, {C} chunks of {CHUNK}; "
          f"update exactly zero at {100.0 * float((~touched).float().mean()):.1f} % of the elements ({name}: one row in "
          f"eight touched); grid {K.topk_grid(n)} blocks x 256 lanes; {args.reps} repetitions ({args.chain_reps} for a torch "
          f"chain) after {args.warmup} warm-up, device events around the pass alone", flush=True)
    for d in (0.1, 0.01, 0.001):
        k = cp.topk_k(n, d)
        print(f"payload at density {d:g}: k = {k}, {4 * K.topk_words(n, k) / 1e6:.2f} MB "
              f"({n / K.topk_words(n, k):.1f}x smaller)", flush=True)
    print(flush=True)

    a = torch.randn(4096, 4096, device=dev, dtype=torch.bfloat16)
    t_end = time.perf_counter() + 1.0  # (working clock)
    while time.perf_counter() < t_end:
        for _ in range(20):
            a = (a @ a).clamp_(-1.0, 1.0)
        torch.cuda.synchronize()
    del a

    def timed(fn, prepare=None, reps=None):
        ms = []
        reps = args.reps if reps is None else reps
        warm = args.warmup if reps == args.reps else 1
        for i in range(warm + reps):
            if prepare is not None:
                prepare()
            e0_, e1_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0_.record()
            fn()
            e1_.record()
            torch.cuda.synchronize()
            if i >= warm:
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
    print(flush=True)

    def restore():
        e.copy_(e0)

    lost = []
    for d in (0.1, 0.01, 0.001):
        k = cp.topk_k(n, d)
        words = K.topk_words(n, k)
        payload = torch.empty(words, dtype=torch.int32, device=dev)
        # hist<0>: w, anchor, e read, v written; hist<1>, hist<2>, count: v read; emit: v read, e' and payload written
        nbytes = n * 4 * (4 + 3 + 2) + 4 * words
        t_k = line(f"topk_encode density {d:g}", timed(lambda: K.topk_encode(w, anchor, e, payload, work, stats, k), restore),
                   nbytes)

        def chain():
            v = (w - anchor) + e
            idx = torch.topk(v.abs(), k, sorted=False).indices
            idx = torch.sort(idx).values
            val = v[idx]
            err = v.clone()
            err[idx] = 0.0
            e.copy_(err)
            payload[1:C + 1].copy_(torch.cumsum(torch.bincount(idx // CHUNK, minlength=C), 0))
            payload[C + 1:C + 1 + k].copy_(val.view(torch.int32))
            loc = torch.zeros(2 * ((k + 1) // 2), dtype=torch.int64, device=dev)
            loc[:k] = idx % CHUNK
            payload[C + 1 + k:].copy_(loc[0::2] | (loc[1::2] << 16))
            stats[0] = torch.linalg.vector_norm(v, dtype=torch.float64)
            stats[1] = torch.linalg.vector_norm(err, dtype=torch.float64)

        t_c = line(f"  torch chain, density {d:g}", timed(chain, restore, args.chain_reps), nbytes)
        print(f"  -> the kernels are {t_c / t_k:.1f} x faster than their torch chain"
              + ("" if t_k < t_c else "   ** SLOWER: condition missed **"), flush=True)
        if not t_k < t_c:
            lost.append(f"topk_encode density {d:g}")
        del payload
    print(flush=True)

    # each launch of one encode at density 0.01, from the profiler's kernel records
    k = cp.topk_k(n, 0.01)
    words = K.topk_words(n, k)
    payload = torch.empty(words, dtype=torch.int32, device=dev)
    must = {"topk_hist_kernel<0>": 16 * n, "topk_hist_kernel<1>": 4 * n, "topk_hist_kernel<2>": 4 * n,
            "topk_count_kernel": 4 * n, "topk_emit_kernel": 8 * n + 4 * words}
    try:
        from torch.profiler import ProfilerActivity, profile
        restore()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(5):
                K.topk_encode(w, anchor, e, payload, work, stats, k)
                restore()
            torch.cuda.synchronize()
        rows_ = [ev for ev in prof.key_averages() if "topk_" in ev.key or "emset" in ev.key]
        print("per launch of topk_encode at density 0.01 (mean device time over 5 calls; bytes the pass must move):",
              flush=True)
        total = 0.0
        for ev in sorted(rows_, key=lambda ev: ev.key):
            us = float(getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0.0)) / max(ev.count, 1)
            found = re.search(r"topk_\w+(<\d+>)?", ev.key)
            short = found.group(0) if found else ev.key[:44]
            total += us * ev.count / 5.0
            nb = must.get(short)
            tail = ""
            if nb is not None:
                gbs = nb / us / 1e3
                tail = f"  {nb / 1e6:8.1f} MB  {gbs:7.0f} GB/s ({100.0 * gbs / copy_gbs[0]:.0f} % of the copy rate)"
            print(f"  {short:44s} x{ev.count // 5:<2d} {us:10.1f} us{tail}", flush=True)
        print(f"  sum of the launches: {total / 1e3:.4f} ms per encode", flush=True)
    except Exception as exc:  # (no kernel records on this build: the totals above stand alone)
        print(f"per-launch times not available: {type(exc).__name__}: {exc}", flush=True)
    print(flush=True)

    out = torch.empty(n, device=dev)
    ps = []
    for c in range(16):
        p = torch.empty(words, dtype=torch.int32, device=dev)
        wk = anchor + 1e-4 * (1 + c) * torch.randn(n, device=dev, generator=g) * touched
        K.topk_encode(wk, anchor, None, p, work, stats, k)
        ps.append(p)
        del wk
    for M in (2, 4, 8, 16):
        nbytes = 4 * words * M + n * (4 + 4 + 2)
        t_k = line(f"topk_decode_mean M = {M}", timed(lambda: K.topk_decode_mean(ps[:M], anchor, out, A.shadow, k)), nbytes)
        inv = 1.0 / M

        def chain():
            acc = torch.zeros(n, device=dev)
            for p in ps[:M]:
                offs = p[:C + 1].to(torch.int64)
                chunk = torch.repeat_interleave(torch.arange(C, device=dev), offs[1:] - offs[:-1])
                wd = p[C + 1 + k:].to(torch.int64) & 0xFFFFFFFF
                loc = torch.stack([wd & 0xFFFF, wd >> 16], dim=1).reshape(-1)[:k]
                acc.index_add_(0, chunk * CHUNK + loc, p[C + 1:C + 1 + k].view(torch.float32))
            out.copy_(anchor + acc * inv)
            A.shadow.copy_(out)

        t_c = line(f"  torch chain, M = {M}", timed(chain, None, args.chain_reps), nbytes)
        print(f"  -> the kernel is {t_c / t_k:.1f} x faster than its torch chain"
              + ("" if t_k < t_c else "   ** SLOWER: condition missed **"), flush=True)
        if not t_k < t_c:
            lost.append(f"topk_decode_mean M = {M}")
    del ps
    model.sync_shadow(force=True)
    print(flush=True)
    print(f"the copy rate of this process: {copy_gbs[0]:.0f} GB/s ({t_copy:.4f} ms for {n * 8 / 1e6:.1f} MB)")
    print("condition (every kernel beats its torch chain in this process): "
          + ("met" if not lost else "MISSED by " + ", ".join(lost)))
    print(f"peak device memory in this process: {torch.cuda.max_memory_allocated() / 1e9:.2f} GB")
    return 2 if lost else 0


if __name__ == "__main__":
    sys.exit(main())
