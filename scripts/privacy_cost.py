#!/usr/bin/env python3
"""What client-level privacy costs per round on the real arena (DistilBERT: 66.4 M floats), in ONE
process beside the pass a round makes today and beside the same arithmetic as a chain of torch ops:

    norm     ``ops.kernels.privacy_norm``: w and the anchor read once, one double per block, then the
             one-block finalize (both launches timed together)
    apply    ``ops.kernels.privacy_apply``, in place with the bf16 shadow: unclipped and clipped at
             sigma = 0, and clipped at sigma > 0 (the pass a private round makes)
    gauss    ``ops.kernels.privacy_gauss``: the generator alone (Philox4x32-10 + Box-Muller), 4 bytes
             stored per value
    plain    ``scale_cast(master, shadow, 1 / N)``: plain FedAvg's finalisation
    torch    sub, norm, mul, add, randn, mul, add, to(bfloat16) on the device, the clip factor kept on
             the device (no host sync: the chain at its best)

Each pass is timed alone with device events; printed: the median / min / max of --reps repetitions
after --warmup, the bytes the pass must move at least, and the GB/s that makes beside the 6.29 TB/s a
float4 copy reaches on this GPU.  Last, the largest deviation of ``privacy_gauss`` from its fp64 host
mirror over 2^20 draws (the figure tests/test_privacy_gpu.py's tolerance is four times of).  No
threshold: the script reports what it measures.

    python3 scripts/privacy_cost.py > profiles/privacy_cost.txt
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
    pv = import_module(PKG + ".parallel.privacy")
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
    w0 = anchor + 1e-4 * torch.randn(n, device=dev, generator=g) * live
    w = A.master
    grid = K.privacy_grid(n)
    partial = torch.empty(grid, dtype=torch.float64, device=dev)
    print(f"arena: {n} floats ({A.n_params} parameters), {4 * n / 1e6:.1f} MB per fp32 stream; "
          f"grid {grid} blocks x 256 lanes, one float4 per lane per iteration; {args.reps} repetitions after "
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
        print(f"{name:34s} median {med:.4f} ms  min {min(ms):.4f}  max {max(ms):.4f}  {nbytes / 1e6:8.1f} MB  "
              f"{gbs:7.0f} GB/s ({100.0 * gbs / (COPY_TBS * 1e3):.0f} % of {COPY_TBS} TB/s)", flush=True)
        return med

    def restore():
        w.copy_(w0)

    restore()
    stats = torch.empty(4, device=dev)
    K.privacy_norm(w, anchor, partial, stats, 1e9)
    norm = float(stats[0])
    clip = 0.5 * norm
    sigma = pv.f32(1.0 * clip / 8 ** 0.5)  # z = 1 over 8 sampled clients
    st_open, st_clip = torch.empty(4, device=dev), torch.empty(4, device=dev)
    K.privacy_norm(w, anchor, partial, st_open, 2.0 * norm)
    K.privacy_norm(w, anchor, partial, st_clip, clip)
    print(f"update norm {norm:.6g}; clipped passes use C = {clip:.6g} (stats {st_clip.tolist()}), noisy ones sigma = "
          f"{sigma:.6g}\n", flush=True)

    plain = line("plain scale_cast", timed(lambda: K.scale_cast(w, A.shadow, 0.125), restore), n * (4 + 4 + 2))
    t_norm = line("privacy_norm (+ finalize)", timed(lambda: K.privacy_norm(w, anchor, partial, stats, clip), restore),
                  n * 8)
    line("privacy_apply unclipped, sigma 0", timed(
        lambda: K.privacy_apply(w, anchor, A.shadow, st_open, 0.0, SEED, 0, 0), restore), n * (4 + 4 + 2))
    t_clip = line("privacy_apply clipped, sigma 0", timed(
        lambda: K.privacy_apply(w, anchor, A.shadow, st_clip, 0.0, SEED, 0, 0), restore), n * (8 + 4 + 2))
    line("privacy_apply unclipped, sigma > 0", timed(
        lambda: K.privacy_apply(w, anchor, A.shadow, st_open, sigma, SEED, 0, 0), restore), n * (4 + 4 + 2))
    t_noise = line("privacy_apply clipped, sigma > 0", timed(
        lambda: K.privacy_apply(w, anchor, A.shadow, st_clip, sigma, SEED, 0, 0), restore), n * (8 + 4 + 2))
    out = torch.empty(n, device=dev)
    t_gauss = line("privacy_gauss", timed(lambda: K.privacy_gauss(out, SEED, 0, 0)), n * 4)

    def both():
        K.privacy_norm(w, anchor, partial, stats, clip)
        K.privacy_apply(w, anchor, A.shadow, stats, sigma, SEED, 0, 0)

    t_both = line("norm + apply (a private round)", timed(both, restore), n * (8 + 8 + 4 + 2))
    del out
    clip_t = torch.tensor(clip, device=dev)
    sigma_t = torch.tensor(sigma, device=dev)

    def chain():
        d = torch.sub(w, anchor)
        nrm = torch.linalg.vector_norm(d)
        scale = (clip_t / nrm).clamp(max=1.0)
        u = anchor + d * scale
        u = u + torch.randn(n, device=dev) * sigma_t
        w.copy_(u)
        A.shadow.copy_(u.to(torch.bfloat16))

    t_chain = line("torch chain on the device", timed(chain, restore), n * (8 + 8 + 4 + 2))
    model.sync_shadow(force=True)
    print()
    print(f"a private round's two passes: {t_both:.4f} ms = {t_both / plain:.1f} x plain scale_cast, "
          f"{t_chain / t_both:.1f} x faster than the torch chain ({t_chain:.4f} ms); alone: norm {t_norm:.4f} + apply "
          f"{t_noise:.4f} ms")
    store_ms = n * 4 / (COPY_TBS * 1e9)
    print(f"the generator alone takes {t_gauss:.4f} ms for {n * 4 / 1e6:.1f} MB stored, {t_gauss / store_ms:.1f} x the "
          f"{store_ms:.4f} ms those bytes take at {COPY_TBS} TB/s: it is ALU-bound; inside apply the noise adds "
          f"{t_noise - t_clip:+.4f} ms to the clipped pass ({t_clip:.4f} -> {t_noise:.4f} ms), so apply with noise is "
          + ("ALU-bound too" if t_noise > 1.25 * t_clip else "still bound by its memory traffic"))
    for first4 in (0, (1 << 32) - 8):
        got = torch.empty(1 << 20, device=dev)
        K.privacy_gauss(got, SEED, 2, 3, first4)
        want = pv.torch_gauss(1 << 20, SEED, 2, 3, first4).to(dev)
        print(f"privacy_gauss against its fp64 host mirror, 2^20 draws at first4 = {first4}: max |difference| = "
              f"{float((got.double() - want.double()).abs().max()):.3e} (condition: <= 2e-5)")
    print(f"peak device memory in this process: {torch.cuda.max_memory_allocated() / 1e9:.2f} GB")
    return 0


if __name__ == "__main__":
    sys.exit(main())
