#!/usr/bin/env python3
"""One lying client against the plain mean, the trimmed mean and the median: 8 virtual clients x 3
rounds on the "calibrated" data profile (i.i.d. overlapping 10 % samples, plain Adam at lr 2e-5, bs16,
a fresh client optimizer every round), client 4 (index 3) sending ``-4 w`` every round
(``--poison-client 3 --poison-kind scale --poison-scale -4``), one arm after another in one process:

    mean                the plain mean (what every path took before)
    trimmed_mean:0.2    k = floor(0.2 * 8) = 1
    median              k = 3

Per arm and round: the aggregate's accuracy / F1 pooled over the 8 clients' test splits and, for the
robust arms, each client's trimmed share (honest expectation 2k / M).  ONE seed per arm: a record of
what comes out, not a bar.

    python3 scripts/robust_agg_poison.py > profiles/robust_agg_poison.txt
"""
import argparse
import os
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = "detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd"
ARMS = "mean,trimmed_mean:0.2,median"


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--arms", default=ARMS, help="comma-separated aggregator[:trim_ratio]")
    ap.add_argument("--clients", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--rows", type=int, default=225_745)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--data-profile", default="calibrated")
    ap.add_argument("--poison-client", type=int, default=3)
    ap.add_argument("--poison-kind", default="scale")
    ap.add_argument("--poison-scale", type=float, default=-4.0)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        os.environ.pop(k, None)
    import torch
    from importlib import import_module
    config = import_module(PKG + ".config")
    data = import_module(PKG + ".data")
    runner = import_module(PKG + ".fed.runner")
    if not torch.cuda.is_available():
        print("no GPU: nothing measured", flush=True)
        return 1
    frame = data.generate_cicids2017(args.rows, seed=0, profile=args.data_profile)
    print(f"# {args.clients} virtual clients x {args.rounds} rounds, data profile {args.data_profile!r} "
          f"({args.rows} rows, each client samples 10 %), {args.epochs} local epoch(s) at bs16, lr 2e-5; client "
          f"{args.poison_client + 1} sends a poisoned update every round ({args.poison_kind}, {args.poison_scale:g})",
          flush=True)
    for arm in args.arms.split(","):
        agg, _, ratio = arm.partition(":")
        with tempfile.TemporaryDirectory() as out:
            cfg = config.FedConfig(out_dir=out, synthetic_rows=args.rows, data_profile=args.data_profile,
                                   epochs=args.epochs, rounds=args.rounds, num_clients=args.clients, plots=False,
                                   resume=False, save_checkpoints=False, verbose=False, heartbeat_s=0.0,
                                   aggregator=agg, trim_ratio=float(ratio) if ratio else 0.2,
                                   poison_client=args.poison_client, poison_kind=args.poison_kind,
                                   poison_scale=args.poison_scale)
            client = runner.FederatedClient(cfg, frame=frame).setup()
            t0 = time.perf_counter()
            res = runner.run_virtual_clients(client, args.clients, rounds=args.rounds,
                                             progress=lambda msg: print(f"[{arm}] {msg}", file=sys.stderr, flush=True))
            wall = time.perf_counter() - t0
            client.log.close()
        print(f"--aggregator {agg}" + (f" --trim-ratio {float(ratio):g}" if ratio else "") + f"   [{wall:.0f} s]",
              flush=True)
        for h in res["rounds"]:
            (tn, fp), (fn, tp) = h["aggregated_confusion"]
            tot = max(tp + tn + fp + fn, 1)
            f1 = tp / max(tp + 0.5 * (fp + fn), 1e-30)
            local = [round(c["local_test"]["accuracy"], 2) for c in h["clients"]]
            print(f"  round {h['round']}: pooled aggregated accuracy {100.0 * (tp + tn) / tot:.3f} %  F1 {f1:.5f}  "
                  f"confusion [[tn {tn}, fp {fp}], [fn {fn}, tp {tp}]]  fedavg {h['fedavg_ms']:.2f} ms", flush=True)
            print(f"           local test accuracy per client {local}", flush=True)
            if "trimmed_share" in h:
                print(f"           k {h['k']}, trimmed share per client {[round(s, 4) for s in h['trimmed_share']]} "
                      f"(honest expectation {2 * h['k'] / args.clients:.4f})", flush=True)
        del client, res
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
