#!/usr/bin/env python3
"""What client-level privacy costs in accuracy: 8 virtual clients x 3 rounds on the "calibrated" data
profile (i.i.d. overlapping 10 % samples, plain Adam at lr 2e-5, bs16, a fresh client optimizer every
round), one arm after another in one process:

    off       no privacy (``privacy_clip`` 0): the run whose update norms set the clip bound
    z = ...   ``--privacy-clip C --privacy-noise z`` for each z of --noise, C = the median
              ``l2_local_to_start`` of the unclipped run

Per arm and round: the aggregate's accuracy / F1 pooled over the 8 clients' test splits, how many
clients were clipped, the std each client added, and the (epsilon, delta) spent so far (an upper bound:
no subsampling amplification is credited).  ONE seed per arm: a record of what comes out, not a bar.

    python3 scripts/privacy_utility.py --rows 60000 --epochs 1 > profiles/privacy_utility.txt
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = "detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd"


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--noise", default="0,0.1,0.3,1.0", help="comma-separated noise multipliers z")
    ap.add_argument("--clients", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--rows", type=int, default=225_745)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--data-profile", default="calibrated")
    ap.add_argument("--delta", type=float, default=1e-5)
    ap.add_argument("--seed", type=int, default=1, help="privacy_seed of every private arm")
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
          f"({args.rows} rows, each client samples 10 %), {args.epochs} local epoch(s) at bs16, lr 2e-5; delta "
          f"{args.delta:g}, privacy_seed {args.seed}", flush=True)

    def run(tag, **kw):
        with tempfile.TemporaryDirectory() as out:
            cfg = config.FedConfig(out_dir=out, synthetic_rows=args.rows, data_profile=args.data_profile,
                                   epochs=args.epochs, rounds=args.rounds, num_clients=args.clients, plots=False,
                                   resume=False, save_checkpoints=False, verbose=False, heartbeat_s=0.0, **kw)
            client = runner.FederatedClient(cfg, frame=frame).setup()
            t0 = time.perf_counter()
            res = runner.run_virtual_clients(client, args.clients, rounds=args.rounds,
                                             progress=lambda msg: print(f"[{tag}] {msg}", file=sys.stderr, flush=True))
            wall = time.perf_counter() - t0
            client.log.close()
        del client
        torch.cuda.empty_cache()
        return res, wall

    def show(res):
        for h in res["rounds"]:
            (tn, fp), (fn, tp) = h["aggregated_confusion"]
            tot = max(tp + tn + fp + fn, 1)
            f1 = tp / max(tp + 0.5 * (fp + fn), 1e-30)
            norms = [c["update_l2"] if "update_l2" in c else c["l2_local_to_start"] for c in h["clients"]]
            tail = ""
            if "privacy_epsilon" in h:
                tail = (f"  clipped {sum(c['clipped'] == 1 for c in h['clients'])}/{len(h['clients'])}  sigma per client "
                        f"{h['clients'][0]['privacy_sigma']:.4g}  epsilon <= {h['privacy_epsilon']:.4g}")
            print(f"  round {h['round']}: pooled aggregated accuracy {100.0 * (tp + tn) / tot:.3f} %  F1 {f1:.5f}  "
                  f"confusion [[tn {tn}, fp {fp}], [fn {fn}, tp {tp}]]{tail}", flush=True)
            print(f"           update norm per client before clipping {[round(x, 4) for x in norms]}", flush=True)

    res, wall = run("off")
    norms = [c["l2_local_to_start"] for h in res["rounds"] for c in h["clients"]]
    C = float(statistics.median(norms))
    print(f"privacy off   [{wall:.0f} s]", flush=True)
    show(res)
    print(f"C = the median l2_local_to_start of that run's {len(norms)} client updates = {C:.6g} "
          f"(min {min(norms):.4g}, max {max(norms):.4g})", flush=True)
    for z in (float(x) for x in args.noise.split(",")):
        res, wall = run(f"z={z:g}", privacy_clip=C, privacy_noise=z, privacy_delta=args.delta, privacy_seed=args.seed)
        print(f"--privacy-clip {C:.6g} --privacy-noise {z:g}   [{wall:.0f} s]", flush=True)
        show(res)
    return 0


if __name__ == "__main__":
    sys.exit(main())
