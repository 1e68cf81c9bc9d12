#!/usr/bin/env python3
"""What a learning-rate schedule costs per training step: the graphed bs32 / seq128 / 6-layer step
(the model and batch shape of scripts/adamw_step_cost.py), AdamW 0.01 with the HF no-decay group
(sparse word rows with the lazy row decay), in two arms in ONE process

    constant   schedule="constant"
    linear     schedule="linear" (warmup 1000 of 100000 steps: the rate never reaches 0 here)

timed with device events in interleaved windows  C L C L ...  of --steps steps each, --windows
windows per arm.  Printed: every window, both arms' means, the spread of the constant arm's
repeated windows, and whether the scheduled arm's mean lies within that spread.  A third arm,
constant_b, is a second constant-schedule model and optimizer built after the other two: what two
identically configured arms differ by in one process (their buffers lie elsewhere), to read the
scheduled arm's difference against.

    python3 scripts/lr_schedule_step_cost.py > profiles/lr_schedule_step_cost.txt
"""
import argparse
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = "detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd"
NO_DECAY = ("bias", "LayerNorm", "layer_norm")


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--windows", type=int, default=8, help="timed windows per arm")
    ap.add_argument("--steps", type=int, default=20, help="steps per window")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--layers", type=int, default=6)
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

    def arm(**sched):
        model = models.DDoSClassifier(config=models.DistilBertConfig(n_layers=args.layers), device=dev, impl="hip",
                                      seed=0)
        opt = engine.ArenaAdam(model, lr=2e-5, weight_decay=0.01, decoupled=True, no_decay=NO_DECAY, **sched)
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

    kinds = {"constant": {}, "linear": dict(schedule="linear", warmup_steps=1000, total_steps=100000),
             "constant_b": {}}
    arms = {name: arm(**kinds[name]) for name in (reversed(list(kinds)) if args.reverse else kinds)}
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
            print(f"window {w} {name:10s} {ms:.4f} ms/step  loss {loss:.6f}", flush=True)
    print()
    for name, (model, opt, step) in arms.items():
        print(f"{name:10s} graphs {len(step.graphs)}  graph_error {step.failed}  lazy {opt.lazy_active()}  "
              f"sched {opt.sched_args()}  steps taken {int(opt.step_t.item())}")
    c, s = res["constant"], res["linear"]
    cm, sm = statistics.mean(c), statistics.mean(s)
    print(f"constant  mean {cm:.4f} ms/step  min {min(c):.4f}  max {max(c):.4f}  stdev {statistics.stdev(c):.4f}  "
          f"(n = {len(c)} windows of {len(timed)} steps)")
    print(f"linear    mean {sm:.4f} ms/step  min {min(s):.4f}  max {max(s):.4f}  stdev {statistics.stdev(s):.4f}")
    b = res["constant_b"]
    bm = statistics.mean(b)
    print(f"constant_b mean {bm:.4f} ms/step  min {min(b):.4f}  max {max(b):.4f}  stdev {statistics.stdev(b):.4f}")
    print(f"constant_b - constant  {bm - cm:+.4f} ms/step ({100.0 * (bm - cm) / cm:+.3f} %)  "
          f"linear - constant_b  {sm - bm:+.4f} ms/step")
    inside = min(c) <= sm <= max(c)
    print(f"linear - constant  {sm - cm:+.4f} ms/step ({100.0 * (sm - cm) / cm:+.3f} %)")
    if inside:
        print("finding: the scheduled arm's mean lies within the constant arm's window-to-window spread "
              f"[{min(c):.4f}, {max(c):.4f}]")
    else:
        edge = max(c) if sm > max(c) else min(c)
        print("finding: the scheduled arm's mean lies OUTSIDE the constant arm's window-to-window spread "
              f"[{min(c):.4f}, {max(c):.4f}] by {sm - edge:+.4f} ms/step")
    return 0


if __name__ == "__main__":
    sys.exit(main())
