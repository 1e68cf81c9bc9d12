#!/usr/bin/env python3
"""One lying client against the plain mean, the median, multi-Krum and the geometric median: 8 virtual
clients x 3 rounds on the "calibrated" data profile (i.i.d. overlapping 10 % samples, plain Adam at lr 2e-5,
bs16, a fresh client optimizer every round), client 4 (index 3) sending ``-4 w`` every round
(``--poison-client 3 --poison-kind scale --poison-scale -4``), one arm after another in one process:

    mean                the plain mean
    median              the coordinate-wise median, k = 3
    multi_krum          f = (8 - 3) // 2 = 2, m = 6
    geometric_median    6 Weiszfeld iterations, nu 1e-6

and one more run of the two distance-based arms with TWO liars of 8 (``--second-liar``, client 7: the
configuration names one poisoner, so for that run the script answers ``utils.faults.poisoned`` itself).

Per arm and round: the aggregate's accuracy / F1 pooled over the 8 clients' test splits and, for the
distance-based arms, the poisoner's score rank (1 = lowest score) or its final weight beside the uniform
1 / M.  ONE seed per arm: a record of what comes out, not a bar.

    python3 scripts/robust_dist_poison.py > profiles/robust_dist_poison.txt
"""
import argparse
import os
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = "detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd"
ARMS = "mean,median,multi_krum,geometric_median,multi_krum+2,geometric_median+2"


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--arms", default=ARMS, help="comma-separated aggregator[+2] (+2: the second liar joins)")
    ap.add_argument("--clients", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--rows", type=int, default=225_745)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--data-profile", default="calibrated")
    ap.add_argument("--poison-client", type=int, default=3)
    ap.add_argument("--second-liar", type=int, default=6)
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
    faults = import_module(PKG + ".utils.faults")
    if not torch.cuda.is_available():
        print("no GPU: nothing measured", flush=True)
        return 1
    frame = data.generate_cicids2017(args.rows, seed=0, profile=args.data_profile)
    print(f"# {args.clients} virtual clients x {args.rounds} rounds, data profile {args.data_profile!r} "
          f"({args.rows} rows, each client samples 10 %), {args.epochs} local epoch(s) at bs16, lr 2e-5; client "
          f"{args.poison_client + 1} sends a poisoned update every round ({args.poison_kind}, {args.poison_scale:g}); "
          f"in the +2 arms client {args.second_liar + 1} does too", flush=True)
    one_liar = faults.poisoned
    sig = lambda v, d=4: float(f"{v:.{d}g}")  # noqa: E731
    for arm in args.arms.split(","):
        agg, _, two = arm.partition("+")
        liars = [args.poison_client] + ([args.second_liar] if two else [])
        faults.poisoned = (lambda cfg, c, r: c in liars) if two else one_liar
        with tempfile.TemporaryDirectory() as out:
            cfg = config.FedConfig(out_dir=out, synthetic_rows=args.rows, data_profile=args.data_profile,
                                   epochs=args.epochs, rounds=args.rounds, num_clients=args.clients, plots=False,
                                   resume=False, save_checkpoints=False, verbose=False, heartbeat_s=0.0,
                                   aggregator=agg, poison_client=args.poison_client, poison_kind=args.poison_kind,
                                   poison_scale=args.poison_scale)
            client = runner.FederatedClient(cfg, frame=frame).setup()
            t0 = time.perf_counter()
            res = runner.run_virtual_clients(client, args.clients, rounds=args.rounds,
                                             progress=lambda msg: print(f"[{arm}] {msg}", file=sys.stderr, flush=True))
            wall = time.perf_counter() - t0
            client.log.close()
        faults.poisoned = one_liar
        print(f"--aggregator {agg}" + (f"   (liars: clients {[c + 1 for c in liars]})" if two else "") + f"   [{wall:.0f} s]",
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
            rep = h.get("robust")
            if rep is not None and rep["kind"] == "multi_krum":
                order = sorted(range(rep["clients"]), key=lambda i: (rep["scores"][i], i))
                print(f"           f {rep['f']}, m {rep['m']}, rejected clients {[c + 1 for c in rep['rejected']]}; scores "
                      f"{[sig(s) for s in rep['scores']]}; score rank of the liar(s) "
                      f"{[order.index(c) + 1 for c in liars]} of {rep['clients']}", flush=True)
            if rep is not None and rep["kind"] == "geometric_median":
                print(f"           weights {[round(w, 5) for w in rep['weights']]} (uniform {1.0 / rep['clients']:.5f}); "
                      f"final weight of the liar(s) {[sig(rep['weights'][c]) for c in liars]}; objective "
                      f"{[sig(o, 5) for o in rep['objective']]}", flush=True)
        del client, res
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
