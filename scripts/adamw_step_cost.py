#!/usr/bin/env python3
"""What AdamW costs per training step: the graphed bs32 / seq128 / 6-layer step, timed with
device events (warm-up 5, 20 steps, like bench.py's window) in three arms

    wd0    weight_decay = 0 (the default step)
    lazy   AdamW 0.01, HF no-decay group, sparse word rows with the lazy row decay
    dense  AdamW 0.01, HF no-decay group, dense word table (sparse_word_grad = False)

interleaved A B C A B C ... for --passes passes; the medians over the passes are reported.  Every
arm of every pass is a child process of its own under its own time limit, and the script stops at
the first child that fails.  --baseline-tree PATH interleaves the wd0 arm of another checkout of
this repository (the parent commit, built) as a fourth arm, to see that the default step did not
move.

    python3 scripts/adamw_step_cost.py --passes 3 [--baseline-tree ../parent] > profiles/adamw_step_cost.txt
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = "detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd"
NO_DECAY = ("bias", "LayerNorm", "layer_norm")


def child(arm: str, tree: str, steps: int, warmup: int, layers: int) -> None:
    sys.path.insert(0, tree)
    import torch
    from importlib import import_module
    engine = import_module(PKG + ".engine")
    models = import_module(PKG + ".models")
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

    model = models.DDoSClassifier(config=models.DistilBertConfig(n_layers=layers), device=dev, impl="hip", seed=0)
    if arm == "wd0":
        opt = engine.ArenaAdam(model, lr=2e-5)
    else:
        opt = engine.ArenaAdam(model, lr=2e-5, weight_decay=0.01, decoupled=True, no_decay=NO_DECAY)
        if arm == "dense":
            model.sparse_word_grad = False
            model._hip_cache = None
    model.train()
    step = engine.GraphedTrainStep(engine.make_step_fn(model, opt), warmup=2, bucket=model.packed_rows)
    warm = [batch(1000 + i) for i in range(warmup)]
    timed = [batch(2000 + i) for i in range(steps)]
    for b in warm[:2]:
        step(*b)
    primed = set()
    for b in timed + warm:  # every bucket captured before the window
        key = step._key(b[0], b[3])
        if key not in step.graphs and key not in primed:
            primed.add(key)
            step(*b)
    torch.cuda.synchronize()
    a = torch.randn(4096, 4096, device=dev, dtype=torch.bfloat16)
    t_end = time.perf_counter() + 1.0  # (working clock)
    while time.perf_counter() < t_end:
        for _ in range(20):
            a = (a @ a).clamp_(-1.0, 1.0)
        torch.cuda.synchronize()
    for b in warm[2:]:
        step(*b)
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    evs[0].record()
    for i, b in enumerate(timed):
        loss = step(*b)
        evs[i + 1].record()
    torch.cuda.synchronize()
    per = [evs[i].elapsed_time(evs[i + 1]) for i in range(steps)]
    sparse = bool(getattr(model, "sparse_word_grad", False))
    print(json.dumps({"arm": arm, "ms_per_step": round(evs[0].elapsed_time(evs[-1]) / steps, 4),
                      "median_step_ms": round(statistics.median(per), 4), "graphs": len(step.graphs),
                      "graph_error": step.failed, "sparse_word_grad": sparse,
                      "lazy": bool(getattr(opt, "lazy_active", lambda: False)()),
                      "loss": round(float(loss), 6)}), flush=True)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--layers", type=int, default=6)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child process")
    ap.add_argument("--baseline-tree", default=None, help="another built checkout: its wd0 arm joins the rotation")
    ap.add_argument("--child", nargs=2, metavar=("ARM", "TREE"), default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(args.child[0], args.child[1], args.steps, args.warmup, args.layers)
        return 0
    arms = [("wd0", ROOT), ("lazy", ROOT), ("dense", ROOT)]
    if args.baseline_tree:
        arms.append(("baseline-wd0", os.path.abspath(args.baseline_tree)))
    results = {name: [] for name, _ in arms}
    for p in range(max(3, args.passes)):
        for name, tree in arms:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", name.split("-")[-1], tree, "--steps",
                   str(args.steps), "--warmup", str(args.warmup), "--layers", str(args.layers)]
            try:
                out = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout, cwd=tree)
            except subprocess.TimeoutExpired:
                print(f"pass {p} arm {name}: no result within {args.timeout} s -- stopping", flush=True)
                return 1
            if out.returncode != 0:
                print(f"pass {p} arm {name}: exit status {out.returncode} -- stopping\n{out.stderr[-2000:]}", flush=True)
                return 1
            rec = json.loads(out.stdout.strip().splitlines()[-1])
            results[name].append(rec)
            print(f"pass {p} {name:13s} {json.dumps(rec)}", flush=True)
    print()
    med = {}
    for name, recs in results.items():
        v = sorted(r["ms_per_step"] for r in recs)
        med[name] = statistics.median(v)
        print(f"{name:13s} ms/step median {med[name]:.4f}  min {v[0]:.4f}  max {v[-1]:.4f}  (n = {len(v)})")
    print(f"lazy - dense  {med['lazy'] - med['dense']:+.4f} ms/step   lazy - wd0  {med['lazy'] - med['wd0']:+.4f} ms/step")
    if "baseline-wd0" in med:
        print(f"wd0 - baseline-wd0  {med['wd0'] - med['baseline-wd0']:+.4f} ms/step")
    return 0


if __name__ == "__main__":
    sys.exit(main())
