#!/usr/bin/env python3
"""What secure aggregation costs in accuracy: 8 virtual clients x 3 rounds on the "calibrated" data profile
(i.i.d. overlapping 10 % samples, plain Adam at lr 2e-5, bs16, a fresh client optimizer every round) --
the protocol of scripts/privacy_utility.py and scripts/compress_utility.py -- one arm after another in
one process:

    off                      the fp32 exchange
    secagg                   ``--secagg true`` (24 fraction bits, ChaCha20)
    privacy                  ``--privacy-clip C --privacy-noise z`` without secure aggregation, C the median
                             update norm of the ``off`` arm
    secagg + privacy         the same with ``--secagg true``

Per arm and round: the aggregate's accuracy / F1 pooled over the 8 clients' test splits, the payload per
client, the pooled fixed-point error and every client's ``quant_error_l2 / update_l2``; at the end the
largest difference between the final weights of an arm with secure aggregation and of its arm without.
The expectation is equality up to the fixed-point error (at most 2^-25 per element and round before the
next round's training amplifies it); what is seen is reported.  ONE seed per arm: a record, not a bar.

    python3 scripts/secagg_utility.py --rows 60000 --epochs 1 > profiles/secagg_utility.txt
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
    ap.add_argument("--clients", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--rows", type=int, default=225_745)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--data-profile", default="calibrated")
    ap.add_argument("--noise", type=float, default=0.1, help="the noise multiplier z of the private arms")
    ap.add_argument("--seed", type=int, default=1, help="privacy_seed of the private arms")
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
            final = client.model.arena.master.detach().clone()
            client.log.close()
        del client
        torch.cuda.empty_cache()
        return res, wall, final

    def show(res):
        accs = []
        for h in res["rounds"]:
            (tn, fp), (fn, tp) = h["aggregated_confusion"]
            tot = max(tp + tn + fp + fn, 1)
            f1 = tp / max(tp + 0.5 * (fp + fn), 1e-30)
            accs.append(100.0 * (tp + tn) / tot)
            tail = f"  epsilon <= {h['privacy_epsilon']:.4g}" if "privacy_epsilon" in h else ""
            print(f"  round {h['round']}: pooled aggregated accuracy {accs[-1]:.3f} %  F1 {f1:.5f}  "
                  f"confusion [[tn {tn}, fp {fp}], [fn {fn}, tp {tp}]]  exchange {h['fedavg_ms']:.2f} ms{tail}", flush=True)
            if "masked_with" in h:
                ratios = [c["quant_error_l2"] / c["update_l2"] for c in h["clients"]]
                print(f"           payload {h['payload_bytes']} B per client under {h['masked_with']} pair streams, clamped "
                      f"{h['clamped']}, bad {h['bad_elems']}, pooled fixed-point error {h['quant_error_l2']:.4g}; "
                      f"quant_error_l2 / update_l2 per client {[float(f'{x:.3g}') for x in ratios]}", flush=True)
        return accs

    table, finals = [], {}
    res, wall, finals["off"] = run("off")
    norms = [c["l2_local_to_start"] for h in res["rounds"] for c in h["clients"]]
    C = float(statistics.median(norms))
    print(f"secagg off   [{wall:.0f} s]", flush=True)
    table.append(("off", show(res)))
    print(f"C = the median l2_local_to_start of that run's {len(norms)} client updates = {C:.6g}", flush=True)
    priv = dict(privacy_clip=C, privacy_noise=args.noise, privacy_seed=args.seed)
    for tag, kw in (("secagg", dict(secagg=True)), ("privacy", priv), ("secagg + privacy", dict(secagg=True, **priv))):
        res, wall, finals[tag] = run(tag, **kw)
        print(f"{tag} ({', '.join(f'{k}={v:g}' if isinstance(v, float) else f'{k}={v}' for k, v in kw.items())})   "
              f"[{wall:.0f} s]", flush=True)
        table.append((tag, show(res)))
    print()
    for tag, accs in table:
        print(f"{tag:20s} " + "  ".join(f"{a:.3f} %" for a in accs), flush=True)
    for on, off in (("secagg", "off"), ("secagg + privacy", "privacy")):
        d = (finals[on].double() - finals[off].double()).abs()
        print(f"final weights, {on!r} against {off!r}: max |difference| {float(d.max()):.3e}, "
              f"rms {float(d.square().mean().sqrt()):.3e} (one fixed-point step is {2.0 ** -24:.3e})", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
