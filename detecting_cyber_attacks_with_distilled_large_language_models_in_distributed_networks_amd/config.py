"""Typed run configuration: one dataclass + CLI flags + env overrides.

The reference has no config system; its literals live in module constants and
inside ``main`` (client1.py:22-23, :356-358, :370-372, :380; server.py:10-13).
Every such literal becomes a field here whose default is the reference value,
so "parity mode" needs no flags.  Per-client variation (client2.py is a copy of
client1.py with seed 43) is derived from the rank: ``seed = base_seed + client_id``.

Env overrides: any field can be set with ``FEDDDOS_<FIELD>`` (upper case).
"""
from __future__ import annotations

import argparse
import dataclasses
import os
from dataclasses import dataclass, field
from typing import Optional


_OPTIONAL_INTS = ("drop_client", "drop_round", "num_clients", "poison_client", "poison_round", "privacy_seed",
                  "secagg_seed", "byzantine", "krum_select")


@dataclass
class FedConfig:
    # --- data (client1.py:23, :84-93, :356) -------------------------------------------
    csv_path: Optional[str] = None          # None -> synthetic CICIDS2017-shaped data
    synthetic_rows: int = 225_745           # full Friday-DDoS file size
    # synthetic generator setting (data/synthetic.py PROFILES): "default" (saturates near 99.95 %),
    # "calibrated" (local models near the reference's 99.05 %), "hard" (numerics tests, ~95 %)
    data_profile: str = "default"
    data_fraction: float = 0.1              # client1.py:23
    base_seed: int = 42                     # client1.py:89 (client2.py:84 uses 43)
    partition: str = "iid_overlap"          # "iid_overlap" (reference) | "disjoint" | "label_skew" (non-IID)
    partition_skew: float = 0.9             # label_skew: DDoS share of even clients (odd: 1 - it); in [0.5, 1)
    max_len: int = 128                      # client1.py:27
    # --- model (client1.py:53-65) ---------------------------------------------------
    model_path: Optional[str] = None        # optional HF distilbert dir; None -> random init
    head_dropout: float = 0.3               # client1.py:57
    hidden_dropout: float = 0.1
    attention_dropout: float = 0.1
    # --- training (client1.py:370-380) ------------------------------------------------
    batch_size: int = 16                    # client1.py:370 (bench uses 32, BASELINE.json)
    eval_batch_size: int = 16
    epochs: int = 3                         # client1.py:380
    lr: float = 2e-5                        # client1.py:380
    betas: tuple = (0.9, 0.999)
    eps: float = 1e-8
    weight_decay: float = 0.0
    decoupled_weight_decay: bool = False    # AdamW when True
    no_decay: str = ""                      # comma-separated name substrings excluded from weight decay
    # learning-rate schedule (engine/optim.py): "constant" | "linear" (warmup, then linear decay to 0:
    # HF get_linear_schedule_with_warmup) | "constant_with_warmup"
    lr_schedule: str = "constant"
    warmup_ratio: float = 0.0               # warmup as a share of the schedule's steps
    warmup_steps: int = 0                   # wins over warmup_ratio when > 0
    # "round": every round's fresh Adam restarts the ramp over that round's steps;
    # "run": one ramp over rounds x steps per round (round r starts at offset r x steps per round)
    lr_schedule_scope: str = "round"
    # FedProx (engine/optim.py): mu / 2 * ||w - w_global||^2 added to every client's loss, w_global the
    # round's starting weights -- holds local epochs on a skewed shard near the global model.  0: off
    prox_mu: float = 0.0
    impl: str = "auto"                      # "hip" | "torch" | "auto" (hip on GPU)
    use_graph: bool = True                  # capture the train step in a HIP graph
    # --- federation (server.py:10-13) -------------------------------------------------
    rounds: int = 1
    num_clients: Optional[int] = None       # None -> world size / gpus_per_client
    gpus_per_client: int = 1                # >1: each client is k data-parallel GPUs (parallel/dp.py)
    dp_graph: bool = False                  # capture data-parallel steps (collectives) in the HIP graph
    weighted_fedavg: bool = False           # reference is unweighted (server.py:73-76)
    # FedOpt server optimizer (parallel/server_opt.py; Reddi et al., "Adaptive Federated Optimization"):
    # avg - w_global is a pseudo-gradient for a server-side momentum / Adagrad / Adam / Yogi step.
    # "fedavg": the plain mean (reference).  server_lr 1.0 suits "avgm"; the adaptive kinds want ~1e-2
    server_opt: str = "fedavg"              # "fedavg" | "avgm" | "adagrad" | "adam" | "yogi"
    server_lr: float = 1.0
    server_betas: tuple = (0.9, 0.99)
    server_tau: float = 1e-3                # adaptivity floor: v starts at tau^2
    # Byzantine-robust aggregation (parallel/robust.py; Yin et al., ICML 2018): per coordinate the k
    # lowest and k highest client values are dropped.  "mean": the plain mean (reference);
    # "trimmed_mean": k = floor(trim_ratio * M) of the M participating clients; "median": k = (M - 1) // 2
    # Distance-based kinds (parallel/robust_dist.py): "multi_krum" (Blanchard et al., NeurIPS 2017) averages the
    # m clients closest to their M - f - 2 nearest neighbours and names the rest; "geometric_median" (RFA,
    # Pillutla et al. 2022) runs smoothed Weiszfeld iterations and gives every client a weight
    aggregator: str = "mean"                # "mean" | "trimmed_mean" | "median" | "multi_krum" | "geometric_median"
    trim_ratio: float = 0.2                 # trimmed_mean: share trimmed at each end, in [0, 0.5)
    byzantine: Optional[int] = None         # multi_krum: f, the liars to tolerate; None: (M - 3) // 2 of the live M
    krum_select: Optional[int] = None       # multi_krum: m, the clients averaged; None: M - f (1: Krum proper)
    geomed_iters: int = 6                   # geometric_median: Weiszfeld iterations
    geomed_nu: float = 1e-6                 # geometric_median: smoothing, the floor of a distance
    # Client-level differential privacy (parallel/privacy.py; DP-FedAvg, McMahan et al., ICLR 2018): every
    # sampled client clips its round update w - w_global to L2 norm privacy_clip and adds
    # N(0, (privacy_noise * privacy_clip)^2 / M) before the exchange, M the round's sampled clients.  0: off
    privacy_clip: float = 0.0               # C, the bound on a client's update norm
    privacy_noise: float = 0.0              # z, the noise multiplier: the sum carries std z * C
    privacy_delta: float = 1e-5             # the delta of the reported (epsilon, delta)
    privacy_seed: Optional[int] = None      # None: 64 bits of os.urandom per process; an int: fixed (tests)
    # Quantized update exchange (parallel/compress.py; QSGD, Alistarh et al. 2017; error feedback,
    # Karimireddy et al. 2019): a client sends w - w_global as int8 / int4 codes with one fp32 scale per 64
    # elements, and keeps what the rounding lost for its next update.  "none": the fp32 exchange (reference)
    # "topk" (Aji & Heafield 2017; Lin et al. 2018; Stich et al. 2018): only the floor(compress_density * n)
    # largest-magnitude entries of the update leave, as exact fp32 values with 16-bit chunk-local indices
    compress: str = "none"                  # "none" | "int8" | "int4" | "topk"
    compress_error_feedback: bool = True    # carry the quantization error into the next round's update
    compress_rounding: str = "nearest"      # "nearest" | "stochastic" (unbiased; Philox keyed by base_seed)
    compress_density: float = 0.01          # topk: the share of the update's entries sent, in (0, 0.5]
    # Secure aggregation (parallel/secagg.py; Bonawitz et al., CCS 2017): a client sends w - w_global as
    # 32-bit fixed point under one ChaCha stream per live partner (pair keys by X25519), added with
    # opposite signs by the two ends of a pair: the streams cancel in the sum and nowhere else
    secagg: bool = False                    # False: the fp32 exchange (reference)
    secagg_frac_bits: int = 24              # fraction bits of the fixed point, 8 .. 30
    secagg_chacha_rounds: int = 20          # 8 | 12 | 20
    secagg_seed: Optional[int] = None       # None: private keys from os.urandom; an int: derived (tests)
    participation: float = 1.0              # fraction of clients aggregated per round
    timeout_s: float = 300.0                # server.py:10 / client1.py:22
    heartbeat_s: float = 1.0                # failure detection (parallel/health.py); 0 disables
    heartbeat_stale_s: float = 10.0         # a peer silent this long is declared dead
    transport: str = "collective"           # "collective" (RCCL/gloo all-reduce) | "tcp" (reference framing; weights-only payload)
    comm: str = "torch"                     # collective backend: "torch" (torch.distributed) | "rccl" (NativeComm)
    server_host: str = "localhost"          # client1.py:276,314
    port_receive: int = 12345               # server.py:11
    port_send: int = 12346                  # server.py:12
    gzip_level: int = 1                     # tcp payload compression (reference: 9)
    # --- outputs ------------------------------------------------------------------------
    out_dir: str = "."
    plots: bool = True
    plot_dpi: int = 0                       # 0: reference per-client DPI (client 1 default, client 2: 300)
    resume: bool = True                     # client1.py:375-377 loads clientN_model.pth
    save_optimizer: bool = False
    save_checkpoints: bool = True           # clientN_model.pth / ddos_distilbert_model.pth (bench: off)
    # --- fault injection -------------------------------------------------
    drop_client: Optional[int] = None       # client whose update is dropped ...
    drop_round: Optional[int] = None        # ... at this round
    # a client that lies (utils/faults.py poison_): its master is replaced just before the exchange
    poison_client: Optional[int] = None     # the client that lies ...
    poison_round: Optional[int] = None      # ... at this round (None: every round)
    poison_kind: str = "scale"              # "scale" (master *= poison_scale) | "noise" | "nan"
    poison_scale: float = -4.0              # scale: the factor; noise: sigma = |poison_scale|
    # --- distillation extension (BASELINE.json config 5) ------------------------------
    teacher: Optional[str] = None           # "bert-base" -> KD from a 12-layer teacher
    kd_temperature: float = 2.0
    # loss = alpha CE + (1 - alpha) T^2 KL(teacher || student).  Measured on the config-5 protocol
    # (seq256 bs64, 3 teacher + 3 student epochs, 4,515 test rows; profiles/r3_kd_sweep.txt):
    # alpha 0.5 -> student F1 0.9888, 0.9 -> 0.9988 (teacher 0.9990)
    kd_alpha: float = 0.9
    verbose: bool = True
    extra: dict = field(default_factory=dict)

    def client_seed(self, client_id: int) -> int:
        return self.base_seed + client_id

    @classmethod
    def from_env(cls, base: Optional["FedConfig"] = None) -> "FedConfig":
        cfg = base or cls()
        for f in dataclasses.fields(cls):
            key = "FEDDDOS_" + f.name.upper()
            if key in os.environ:
                setattr(cfg, f.name, _coerce(f, os.environ[key], getattr(cfg, f.name)))
        return cfg

    @classmethod
    def add_cli(cls, parser: argparse.ArgumentParser) -> argparse.ArgumentParser:
        for f in dataclasses.fields(cls):
            if f.name == "extra":
                continue
            name = "--" + f.name.replace("_", "-")
            default = f.default if f.default is not dataclasses.MISSING else None
            if isinstance(default, bool):
                parser.add_argument(name, dest=f.name, default=None,
                                    type=lambda s: s.lower() in ("1", "true", "yes", "on"),
                                    metavar="BOOL")
            elif isinstance(default, tuple):
                parser.add_argument(name, dest=f.name, default=None, type=float, nargs=len(default))
            else:
                typ = type(default) if default is not None else str
                if f.name in _OPTIONAL_INTS:
                    typ = int
                parser.add_argument(name, dest=f.name, default=None, type=typ)
        return parser

    @classmethod
    def from_args(cls, ns: argparse.Namespace) -> "FedConfig":
        cfg = cls.from_env()
        for f in dataclasses.fields(cls):
            v = getattr(ns, f.name, None)
            if v is not None:
                setattr(cfg, f.name, tuple(v) if isinstance(f.default, tuple) else v)
        return cfg


def _coerce(f, raw: str, current):
    if isinstance(current, bool):
        return raw.lower() in ("1", "true", "yes", "on")
    if isinstance(current, int):
        return int(raw)
    if isinstance(current, float):
        return float(raw)
    if isinstance(current, tuple):
        return tuple(float(x) for x in raw.split(","))
    if current is None and f.name in _OPTIONAL_INTS:
        return int(raw)
    return raw
