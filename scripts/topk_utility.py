#!/usr/bin/env python3
"""What the top-k sparsified update exchange costs in accuracy: 8 virtual clients x 3 rounds on the
"calibrated" data profile (i.i.d. overlapping 10 % samples, plain Adam at lr 2e-5, bs16, a fresh client
optimizer every round) -- the protocol of scripts/compress_utility.py -- one arm after another in one
process:

    off                      the fp32 exchange (``compress`` "none")
    topk d                   ``--compress topk --compress-density d`` with error feedback (the default),
                             d = 0.1 / 0.01 / 0.001
    topk d, no EF            ``--compress-error-feedback false``: what is not sent is dropped every round

Per arm and round: the aggregate's accuracy / F1 pooled over the 8 clients' test splits, the payload
per client, and the measured ``quant_error_l2 / update_l2`` (the share of the update's norm held back)
and threshold of every client (with error feedback the update includes the carried residual).  ONE
seed per arm: a record of what comes out, not a bar.

    python3 scripts/topk_utility.py --rows 60000 --epochs 1 > profiles/topk_utility.txt
"""
import argparse
import os
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = "detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd"


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--clients", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--rows", type=int, default=225_745)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--data-profile", default="calibrated")
    ap.add_argument("--densities", type=float, nargs="+", default=[0.1, 0.01, 0.001])
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
          f"({args.rows} rows, each client samples 10 %), {args.epochs} local epoch(s) at bs16, lr 2e-5; one seed",
          flush=True)

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
        accs = []
        for h in res["rounds"]:
            (tn, fp), (fn, tp) = h["aggregated_confusion"]
            tot = max(tp + tn + fp + fn, 1)
            f1 = tp / max(tp + 0.5 * (fp + fn), 1e-30)
            accs.append(100.0 * (tp + tn) / tot)
            print(f"  round {h['round']}: pooled aggregated accuracy {accs[-1]:.3f} %  F1 {f1:.5f}  "
                  f"confusion [[tn {tn}, fp {fp}], [fn {fn}, tp {tp}]]  exchange {h['fedavg_ms']:.2f} ms", flush=True)
            if "quant_error_l2" in h:
                ratios = [c["quant_error_l2"] / c["update_l2"] for c in h["clients"]]
                print(f"           payload {h['payload_bytes']} B per client ({h['compress_ratio']:.2f}x smaller), "
                      f"{h['clients'][0]['sent']} entries each, bad elements {h['bad_elems']}; held back / update_l2 per "
                      f"client {[round(x, 5) for x in ratios]}", flush=True)
                print(f"           update_l2 per client {[round(c['update_l2'], 4) for c in h['clients']]}; threshold "
                      f"{[float(format(c['threshold'], '.3g')) for c in h['clients']]}", flush=True)
            else:
                print(f"           update norm per client {[round(c['l2_local_to_start'], 4) for c in h['clients']]}",
                      flush=True)
        return accs

    arms = [("off", {})]
    for d in args.densities:
        arms.append((f"topk {d:g}", dict(compress="topk", compress_density=d)))
        arms.append((f"topk {d:g}, no error feedback", dict(compress="topk", compress_density=d,
                                                           compress_error_feedback=False)))
    table = []
    for tag, kw in arms:
        res, wall = run(tag, **kw)
        print(f"compress {tag}   [{wall:.0f} s]", flush=True)
        table.append((tag, show(res)))
    print()
    base = table[0][1]
    for tag, accs in table:
        print(f"{tag:32s} " + "  ".join(f"{a:.3f} %" for a in accs)
              + ("" if tag == "off" else "   vs off: " + "  ".join(f"{a - b:+.3f}" for a, b in zip(accs, base))), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
