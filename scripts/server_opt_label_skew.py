#!/usr/bin/env python3
"""FedOpt server optimizers on the label-skew partition: 8 virtual clients x 3 rounds, the protocol of
profiles/fedprox_label_skew.txt (225,745 synthetic rows, each client draws 10 %, 90 % DDoS for clients
1, 3, 5, 7 and 10 % for the others, 3 local epochs per round at bs16, lr 2e-5, plain Adam, a fresh client
optimizer every round) on the "calibrated" data profile, one arm after another in one process:

    fedavg              the plain mean
    avgm                server momentum, server_lr 1.0
    adam / yogi         at server_lr 1e-3, 3e-3, 1e-2

Per arm and round: the aggregate's accuracy / F1 pooled over the 8 clients' test splits, the l2 norm of
the pseudo-gradient (avg - global) and of the server step, and the clients' mean drift from the round's
start.  ONE seed per arm: a record of what comes out, not a bar.

    python3 scripts/server_opt_label_skew.py [--arms fedavg,avgm,adam:1e-3,...] >> profiles/server_opt_label_skew.txt
"""
import argparse
import os
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = "detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd"
ARMS = "fedavg,avgm,adam:1e-3,adam:3e-3,adam:1e-2,yogi:1e-3,yogi:3e-3,yogi:1e-2"


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--arms", default=ARMS, help="comma-separated kind[:server_lr]")
    ap.add_argument("--clients", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--rows", type=int, default=225_745)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--skew", type=float, default=0.9)
    ap.add_argument("--data-profile", default="calibrated")
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
    print(f"# {args.clients} virtual clients x {args.rounds} rounds, label_skew {args.skew}, data profile "
          f"{args.data_profile!r} ({args.rows} rows), {args.epochs} local epochs at bs16, lr 2e-5", flush=True)
    for arm in args.arms.split(","):
        kind, _, lr = arm.partition(":")
        with tempfile.TemporaryDirectory() as out:
            cfg = config.FedConfig(out_dir=out, synthetic_rows=args.rows, data_profile=args.data_profile,
                                   partition="label_skew", partition_skew=args.skew, epochs=args.epochs,
                                   rounds=args.rounds, num_clients=args.clients, plots=False, resume=False,
                                   save_checkpoints=False, verbose=False, heartbeat_s=0.0, server_opt=kind,
                                   server_lr=float(lr) if lr else 1.0)
            client = runner.FederatedClient(cfg, frame=frame).setup()
            t0 = time.perf_counter()
            res = runner.run_virtual_clients(client, args.clients, rounds=args.rounds,
                                             progress=lambda msg: print(f"[{arm}] {msg}", file=sys.stderr, flush=True))
            wall = time.perf_counter() - t0
            client.log.close()
        srv = client.server
        head = f"--server-opt {kind}" + (f" --server-lr {srv.lr:g} (betas ({srv.b1:g}, {srv.b2:g}), tau {srv.tau:g})"
                                         if srv is not None else "")
        print(f"{head}   [{wall:.0f} s]", flush=True)
        for h in res["rounds"]:
            (tn, fp), (fn, tp) = h["aggregated_confusion"]
            tot = max(tp + tn + fp + fn, 1)
            f1 = tp / max(tp + 0.5 * (fp + fn), 1e-30)
            drift = sum(c["l2_local_to_start"] for c in h["clients"]) / len(h["clients"])
            local = [round(c["local_test"]["accuracy"], 2) for c in h["clients"]]
            norms = (f"  |avg - global| {h['delta_l2']:.4f}  |server step| {h['step_l2']:.4f}" if "delta_l2" in h else "")
            print(f"  round {h['round']}: pooled aggregated accuracy {100.0 * (tp + tn) / tot:.3f} %  F1 {f1:.5f}  "
                  f"confusion [[tn {tn}, fp {fp}], [fn {fn}, tp {tp}]]  mean ||w_local - w_global|| {drift:.4f}"
                  f"{norms}  steps/client {h['clients'][0]['train']['steps']}", flush=True)
            print(f"           local test accuracy per client {local}", flush=True)
        del client, res
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
