#!/usr/bin/env python3
"""What the FedProx proximal term costs per training step: the graphed bs32 / seq128 / 6-layer step
(the model and batch shape of scripts/lr_schedule_step_cost.py), plain Adam as in the benchmark
(no weight decay: the sparse word rows and the rest of the step inside the all-layer dW launch), in
three arms in ONE process

    off     prox_mu = 0
    prox    prox_mu = 0.01 (every Adam launch also reads the anchor: +4 B per parameter)
    off_b   a second prox_mu = 0 model and optimizer, built after the other two: what two
            identically configured arms differ by in one process (their buffers lie elsewhere)

timed with device events in interleaved windows  O P O' O P O' ...  of --steps steps each, --windows
windows per arm.  Printed: every window, each arm's mean, and the term's cost (prox - off) beside
the spread of the two off arms.  No threshold: the script reports what it measures.

    python3 scripts/fedprox_step_cost.py > profiles/fedprox_step_cost.txt
"""
import argparse
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = "detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd"


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--windows", type=int, default=8, help="timed windows per arm")
    ap.add_argument("--steps", type=int, default=20, help="steps per window")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--layers", type=int, default=6)
    ap.add_argument("--mu", type=float, default=0.01)
    ap.add_argument("--reverse", action="store_true", help="build and time the arms in the opposite order")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from importlib import import_module
    engine = import_module(PKG + ".engine")
    models = import_module(PKG + ".models")
    if not torch.cuda.is_available():
        print("no GPU: nothing measured", flush=True)
        return 1
    dev = torch.device("cuda")
    B, S = 32, 128

    def batch(seed):
        g = torch.Generator().manual_seed(seed)
        ids = torch.randint(1000, 2000, (B, S), generator=g)
        lens = torch.randint(S // 3, S + 1, (B,), generator=g)
        mask = (torch.arange(S)[None] < lens[:, None]).long()
        ids = ids * mask
        ids[:, 0] = 101
        return ids.to(dev), mask.to(dev), torch.randint(0, 2, (B,), generator=g).to(dev), int(lens.sum())

    warm = [batch(1000 + i) for i in range(max(2, args.warmup))]
    timed = [batch(2000 + i) for i in range(args.steps)]

    def arm(mu):
        model = models.DDoSClassifier(config=models.DistilBertConfig(n_layers=args.layers), device=dev, impl="hip",
                                      seed=0)
        opt = engine.ArenaAdam(model, lr=2e-5, prox_mu=mu)
        model.train()
        step = engine.GraphedTrainStep(engine.make_step_fn(model, opt), warmup=2, bucket=model.packed_rows)
        for b in warm[:2]:
            step(*b)
        primed = set()
        for b in timed + warm:  # every bucket captured before the first window
            key = step._key(b[0], b[3])
            if key not in step.graphs and key not in primed:
                primed.add(key)
                step(*b)
        torch.cuda.synchronize()
        return model, opt, step

    kinds = {"off": 0.0, "prox": args.mu, "off_b": 0.0}
    arms = {name: arm(kinds[name]) for name in (reversed(list(kinds)) if args.reverse else kinds)}
    a = torch.randn(4096, 4096, device=dev, dtype=torch.bfloat16)
    t_end = time.perf_counter() + 1.0  # (working clock)
    while time.perf_counter() < t_end:
        for _ in range(20):
            a = (a @ a).clamp_(-1.0, 1.0)
        torch.cuda.synchronize()

    def window(step):
        for b in warm[2:]:
            step(*b)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for b in timed:
            loss = step(*b)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / len(timed), float(loss)

    res = {name: [] for name in arms}
    for w in range(max(3, args.windows)):
        for name, (_, _, step) in arms.items():
            ms, loss = window(step)
            res[name].append(ms)
            print(f"window {w} {name:6s} {ms:.4f} ms/step  loss {loss:.6f}", flush=True)
    print()
    nparam = 0
    for name, (model, opt, step) in arms.items():
        nparam = model.arena.numel
        print(f"{name:6s} graphs {len(step.graphs)}  graph_error {step.failed}  fused {opt.can_fuse()}  "
              f"prox_mu {opt.prox_mu}  anchor {'yes' if opt.anchor is not None else 'no'}  "
              f"steps taken {int(opt.step_t.item())}")
    mean = {}
    for name in kinds:
        r = res[name]
        mean[name] = statistics.mean(r)
        print(f"{name:6s} mean {mean[name]:.4f} ms/step  min {min(r):.4f}  max {max(r):.4f}  "
              f"stdev {statistics.stdev(r):.4f}  (n = {len(r)} windows of {len(timed)} steps)")
    off, offb, px = mean["off"], mean["off_b"], mean["prox"]
    base = 0.5 * (off + offb)
    print(f"off_b - off   {offb - off:+.4f} ms/step ({100.0 * (offb - off) / off:+.3f} %)   <- identical arms")
    print(f"prox - off    {px - off:+.4f} ms/step ({100.0 * (px - off) / off:+.3f} %)")
    print(f"prox - off_b  {px - offb:+.4f} ms/step ({100.0 * (px - offb) / offb:+.3f} %)")
    print(f"prox - mean(off, off_b)  {px - base:+.4f} ms/step ({100.0 * (px - base) / base:+.3f} %)")
    print(f"anchor reads: at most {4 * nparam / 1e6:.1f} MB per step ({nparam} parameters x 4 B; word rows "
          f"without Adam state are skipped with the rest of their traffic)")
    lo, hi = min(off, offb), max(off, offb)
    where = "within" if lo <= px <= hi else "OUTSIDE"
    print(f"finding: the prox arm's mean lies {where} the two off arms' means [{lo:.4f}, {hi:.4f}]")
    return 0


if __name__ == "__main__":
    sys.exit(main())
