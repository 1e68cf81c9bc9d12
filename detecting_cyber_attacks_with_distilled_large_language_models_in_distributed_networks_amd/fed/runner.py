"""Federated round orchestration: one process per GPU = one client.

Reference flow per client (client1.py:353-411) + server (server.py:116-137):
  preprocess -> split 60/20/20 -> train 3 epochs -> eval val/test -> save CSV +
  clientN_model.pth -> upload (TCP, gzip) -> server averages -> download ->
  eval val/test of the aggregate -> CSV + plots -> save clientN_model.pth.

Here the upload/average/download triple is ``fedavg_`` (one RCCL all-reduce of
the fp32 arena, ``parallel/fedavg.py``) and the server's duties (writing
``ddos_distilbert_model.pth``, the cross-client report) fall to rank 0.  Extras
over the reference: R rounds in-process, resume from the round sidecar,
sample-weighted FedAvg, seeded partial participation, fault injection, a
cross-client JSON report gathered with an all-gather, and clients that span
``gpus_per_client`` data-parallel GPUs (parallel/dp.py; replica 0 of each
client does the client's file output).
"""
from __future__ import annotations

import json
import math
import os
import time
from typing import Dict, List, Optional

import torch

from ..config import FedConfig
from ..data import DeviceLoader, WordPieceTokenizer, build_client_data, generate_cicids2017
from ..engine import ArenaAdam, evaluate_model, train_model
from ..models import DDoSClassifier, DistilBertConfig
from ..parallel import comm, health
from ..parallel.dp import DPShardLoader, GradSync, dp_seed_offset, make_topology
from ..parallel.compress import check_compress_config, make_compressor
from ..parallel.fedavg import broadcast_model, fedavg_
from ..parallel.privacy import check_privacy_config, make_privatizer
from ..parallel.secagg import check_secagg_config, make_secagg
from ..parallel.robust import DIST_AGGREGATORS, check_robust_config, make_robust, most_trimmed, robust_aggregate_
from ..parallel.server_opt import check_server_config, make_server_optimizer
from ..utils import checkpoint as ck
from ..utils import faults
from ..utils.logging import TagLogger
from ..utils.metrics import save_metrics
from ..utils.timers import PhaseTimer


def _schedule_kwargs(cfg: FedConfig, round_index: int = 0, rounds: int = 1,
                     steps_per_round: Optional[int] = None) -> Dict:
    """``ArenaAdam``'s schedule keywords for the configuration (``--lr-schedule linear --warmup-ratio
    0.1``).  Scope "round": the ramp covers one round's steps -- the total is left to ``train_model``
    (epochs x batches).  Scope "run": one ramp over ``rounds * steps_per_round`` steps, round
    ``round_index`` starting at offset ``round_index * steps_per_round`` (derived from the round
    index alone, so a resumed job needs no saved state)."""
    if cfg.lr_schedule == "constant":
        return {}
    if cfg.lr_schedule_scope not in ("round", "run"):
        raise ValueError(f"lr_schedule_scope must be 'round' or 'run', got {cfg.lr_schedule_scope!r}")
    kw = {"schedule": cfg.lr_schedule, "warmup_steps": cfg.warmup_steps, "warmup_ratio": cfg.warmup_ratio}
    if cfg.lr_schedule_scope == "run" and steps_per_round:
        kw["total_steps"] = int(rounds) * int(steps_per_round)
        kw["step_offset"] = int(round_index) * int(steps_per_round)
    return kw


def make_optimizer(model, cfg: FedConfig, round_index: int = 0, rounds: int = 1,
                   steps_per_round: Optional[int] = None) -> ArenaAdam:
    """The client optimizer of a run: Adam / AdamW with the configuration's hyper-parameters, its
    no-decay parameter group (``--no-decay bias,LayerNorm,layer_norm``) and its learning-rate
    schedule (``_schedule_kwargs``; round_index / rounds / steps_per_round matter to scope "run"),
    and the FedProx term (``--prox-mu``).  Its anchor is the model's weights when the optimizer's
    ``reset_state()`` runs: every caller builds the optimizer and resets it with the round's starting
    weights loaded (the broadcast init, the aggregate a resumed job loads, or the last round's
    aggregate -- which a client dropped from that round's average receives too)."""
    return ArenaAdam(model, lr=cfg.lr, betas=cfg.betas, eps=cfg.eps, weight_decay=cfg.weight_decay,
                     decoupled=cfg.decoupled_weight_decay, prox_mu=cfg.prox_mu,
                     no_decay=tuple(x.strip() for x in cfg.no_decay.split(",") if x.strip()),
                     **_schedule_kwargs(cfg, round_index, rounds, steps_per_round))


def make_teacher_optimizer(teacher, cfg: FedConfig) -> ArenaAdam:
    """The teacher's plain Adam; with a configured schedule, the same schedule over the teacher's
    own step count (``train_model`` fills in the total).  No proximal term: the teachers stay local,
    there is no global teacher to stay near."""
    if cfg.lr_schedule == "constant":
        return ArenaAdam(teacher, lr=cfg.lr)
    return ArenaAdam(teacher, lr=cfg.lr, **_schedule_kwargs(cfg))


def _metrics_record(m) -> Dict:
    return {"accuracy": float(m[0]), "loss": float(m[1]), "precision": float(m[2]), "recall": float(m[3]),
            "f1": float(m[4]), "confusion_matrix": [[int(x) for x in row] for row in m[5]]}


class FederatedClient:
    def __init__(self, cfg: FedConfig, frame=None, model_config: Optional[DistilBertConfig] = None):
        self.cfg = cfg
        self.di = comm.init_distributed(timeout_s=cfg.timeout_s)
        self.topo = make_topology(cfg.gpus_per_client)
        self.idx = self.topo.client_idx              # 0-based client index
        self.client_id = self.idx + 1                # reference naming: Client 1, Client 2, ...
        self.num_clients = cfg.num_clients or self.topo.num_clients
        self.writer = self.topo.dp_rank == 0         # replica 0 writes the client's files
        os.makedirs(cfg.out_dir, exist_ok=True)
        sfx = "" if self.writer else f"_replica{self.topo.dp_rank}"
        self.log = TagLogger.for_client(self.client_id, enabled=cfg.verbose and self.writer,
                                        jsonl_path=os.path.join(cfg.out_dir, f"client{self.client_id}{sfx}_log.jsonl"))
        self.timer = PhaseTimer()
        self.device = self.di.device
        self.frame = frame
        self.model_config = model_config or DistilBertConfig()

    # ------------------------------------------------------------------ setup
    def setup(self):
        cfg, log = self.cfg, self.log
        check_server_config(cfg)  # (an unknown kind, a bad value, or transport=tcp: refused before any work)
        check_robust_config(cfg)  # (likewise: an unknown aggregator, tcp, weighted_fedavg)
        check_privacy_config(cfg, self.topo.gpus_per_client)  # (a bad clip / noise / delta, weighted_fedavg, replicas)
        check_compress_config(cfg, self.topo.gpus_per_client)  # (an unknown width, tcp, a robust aggregator, ...)
        check_secagg_config(cfg, self.topo.gpus_per_client, self.num_clients)  # (tcp, a robust aggregator, compress, ...)
        log.phase("Starting client")
        with self.timer("preprocess"):
            if self.frame is None:
                if cfg.csv_path:
                    import pandas as pd
                    self.frame = pd.read_csv(cfg.csv_path)
                else:
                    # Same seeded synthetic file on every client (they sample it independently).
                    self.frame = generate_cicids2017(cfg.synthetic_rows, seed=0, profile=cfg.data_profile)
            self.tokenizer = WordPieceTokenizer.from_pretrained(cfg.model_path)
            self.data = build_client_data(self.frame, self.idx, cfg.data_fraction, cfg.base_seed, cfg.max_len,
                                          self.tokenizer, cfg.partition, self.num_clients, log=log,
                                          partition_skew=cfg.partition_skew)
        dev = self.device
        self.train_loader = DeviceLoader(self.data.train, cfg.batch_size, shuffle=True, device=dev,
                                         seed=cfg.client_seed(self.idx))
        if self.topo.dp:
            self.train_loader = DPShardLoader(self.train_loader, self.topo.dp_rank, self.topo.gpus_per_client)
        self.val_loader = DeviceLoader(self.data.val, cfg.eval_batch_size, device=dev)
        self.test_loader = DeviceLoader(self.data.test, cfg.eval_batch_size, device=dev)
        mc = self.model_config
        mc.dropout, mc.attention_dropout = cfg.hidden_dropout, cfg.attention_dropout
        self.model = DDoSClassifier(cfg.model_path, config=mc, device=dev, impl=cfg.impl, seed=0,
                                    head_dropout=cfg.head_dropout)
        self.comm = None
        if cfg.comm == "rccl" and dev.type == "cuda":
            from ..parallel.rccl import NativeComm
            self.comm = NativeComm()
            log.info(f"native RCCL communicator: {self.comm.world_size} ranks")
        # Identical start for every client: rank 0's weights win.
        broadcast_model(self.model, comm=self.comm)
        self.grad_sync = None
        self.dp_comm = None
        if self.topo.dp:
            dp_seed_offset(self.model, self.topo.dp_rank)
            # opt-in (FEDDDOS_DP_NATIVE=1) until the graph-captured exchange has run on >= 2 GPUs
            # (ADVICE r3); the default is torch.distributed's eager async all-reduces
            if dev.type == "cuda" and self.di.backend == "nccl" and os.environ.get("FEDDDOS_DP_NATIVE", "0") == "1":
                # the client's replicas exchange over a framework RCCL communicator of their own
                # group: stream-ordered collectives, so the data-parallel step is graph-captured
                from ..parallel.rccl import NativeComm
                self.dp_comm = NativeComm(group=self.topo.dp_group)
            self.grad_sync = GradSync(self.model, self.topo.dp_group, self.topo.gpus_per_client,
                                      max_rows=cfg.batch_size * cfg.max_len, ncomm=self.dp_comm)
            log.info(f"data-parallel client: replica {self.topo.dp_rank + 1}/{self.topo.gpus_per_client}")
        self.teacher = None
        if cfg.teacher:
            from ..models.bert import BertTeacherClassifier, bert_base_config
            self.teacher = BertTeacherClassifier(cfg.extra.get("teacher_path"), config=bert_base_config(),
                                                 device=dev, impl=cfg.impl)
            broadcast_model(self.teacher, comm=self.comm)
        self.teacher_sync = None
        if self.teacher is not None and self.topo.dp:
            # the teacher fine-tune is data-parallel too, so every replica distils from the same teacher
            dp_seed_offset(self.teacher, self.topo.dp_rank)
            self.teacher_sync = GradSync(self.teacher, self.topo.dp_group, self.topo.gpus_per_client,
                                         max_rows=cfg.batch_size * cfg.max_len, ncomm=self.dp_comm)
        self.start_round = 0
        self.history: List[Dict] = []
        if cfg.resume:
            self._resume()
        # FedOpt server optimizer (parallel/server_opt.py; None: plain FedAvg).  Built with the round's
        # starting weights loaded -- the broadcast init or the aggregate a resumed job loads -- which
        # become its x; a resumed job then restores the moments that go with that aggregate.
        self.server = make_server_optimizer(self.model, cfg, log=log)
        if self.server is not None:
            log.info(f"server optimizer: {self.server.kind} (lr {self.server.lr:g}, betas "
                     f"({self.server.b1:g}, {self.server.b2:g}), tau {self.server.tau:g})")
            if self.start_round > 0:
                self._resume_server()
        # Byzantine-robust aggregator (parallel/robust.py; None: the plain mean, today's path)
        self.robust = make_robust(cfg, self.topo.gpus_per_client)
        if self.robust is not None:
            log.info(f"robust aggregation: {self.robust.aggregator}"
                     + (f" (trim_ratio {self.robust.trim_ratio:g})" if self.robust.aggregator == "trimmed_mean" else "")
                     + _dist_setup_note(self.robust))
        # Client-level differential privacy (parallel/privacy.py; None: privacy_clip == 0, today's path)
        self.privacy = make_privatizer(cfg, self.topo.gpus_per_client)
        if self.privacy is not None:
            log.info(_privacy_line(self.privacy, cfg.rounds))
        # Quantized update exchange (parallel/compress.py; None: compress == "none", today's path)
        self.compress = make_compressor(cfg, self.topo.gpus_per_client)
        if self.compress is not None:
            log.info(_compress_line(self.compress))
        # Secure aggregation (parallel/secagg.py; None: secagg off, today's path): a fresh key pair per
        # process -- so also after an elastic restart -- and one all-gather of the public keys
        self.secagg = make_secagg(cfg, self.topo.gpus_per_client, self.num_clients, log=log.info)
        if self.secagg is not None:
            if self.di.distributed:
                self.secagg.setup_keys(self.idx, self.num_clients, comm=self.comm, device=dev)
            else:  # (one process: its own client, or every virtual client -- which hides nothing)
                self.secagg.setup_keys(range(self.num_clients), self.num_clients)
            log.info(_secagg_line(self.secagg, self.num_clients))
        self._round_anchor = None  # the round's starting weights: what privacy, compression and secagg measure against
        self.health = None
        if self.di.distributed and cfg.heartbeat_s > 0 and cfg.transport != "tcp":
            self.health = health.start(cfg.heartbeat_s, cfg.heartbeat_stale_s, cfg.timeout_s)
        restarts = int(os.environ.get("TORCHELASTIC_RESTART_COUNT", "0"))
        if restarts:
            log.info(f"elastic restart #{restarts}: resuming at round {self.start_round + 1}")
            if self.compress is not None and self.compress.error_feedback:
                self.compress.reset()
                log.info(("sparsification" if self.compress.bits is None else "quantization")
                         + " residual lost with the restarted process: error feedback starts again from zero")
        log.info(f"data: {len(self.data.train)} train / {len(self.data.val)} val / {len(self.data.test)} test rows "
                 f"(sampled {self.data.n_rows}), impl={self.model.impl}, device={dev}")
        return self

    def _resume(self):
        """Pick ONE resume round for the whole world and start every client from that round's
        aggregate.

        The source of truth is the round tag of ``ddos_distilbert_model.pth``, which rank 0
        writes right after FedAvg and before any client records the round in its fed_state.
        Rank 0 can tag round r+1 only after every client has finished round r, so after a crash
        the tag is the last round whose aggregate exists, whatever each client's own sidecar
        says.  Rank 0 -- the rank that loads and broadcasts the aggregate -- decides, and its
        round is broadcast, so a rank that cannot see the file (a per-node out_dir) follows
        rank 0 instead of restarting the world from scratch.  An out_dir written before the
        tag existed (aggregate on disk, no tag) resumes from rank 0's sidecar
        ``completed_rounds``, with a warning.  A client's own ``clientN_model.pth`` is never the
        resume point of a collective run: after a crash inside a round it holds that round's
        LOCAL model (fed/runner.py run_round saves it before FedAvg).  Single-process runs with
        no sidecar keep the reference behaviour of loading it (client1.py:375-377: re-running
        the script is the next round)."""
        cfg, log = self.cfg, self.log
        st = ck.load_fed_state(cfg.out_dir, self.client_id)
        start = 0
        if self.di.is_main or not self.di.distributed:
            start = ck.load_global_round(cfg.out_dir)
            legacy = int((st or {}).get("completed_rounds", 0))
            if start == 0 and os.path.exists(ck.global_ckpt_path(cfg.out_dir)):
                if legacy > 0:
                    log.info(f"[WARN] {ck.global_ckpt_path(cfg.out_dir)} has no round tag (written by an older "
                             f"version): resuming from the client sidecar's {legacy} completed round(s)")
                    start = legacy
                else:
                    log.info(f"[WARN] {ck.global_ckpt_path(cfg.out_dir)} has no round tag and no sidecar "
                             f"records a completed round: starting from round 1")
        if self.di.distributed:
            start = int(comm.broadcast_float(float(start), src=0))
        if start > 0:
            path = ck.global_ckpt_path(cfg.out_dir)
            if self.di.is_main or not self.di.distributed:
                ck.load_model(self.model, path)
            broadcast_model(self.model, comm=self.comm)
            self.start_round = start
            self.history = [h for h in (st or {}).get("history", []) if int(h.get("round", 0)) <= start]
            done = int((st or {}).get("completed_rounds", 0))
            if done != start:
                log.info(f"client sidecar says {done} completed round(s); the aggregate says {start}")
            log.info(f"loading pre-trained model from {path} (aggregate of round {start})")
        elif st is None and not self.di.distributed:
            path = ck.client_ckpt_path(cfg.out_dir, self.client_id)
            if ck.load_model(self.model, path):
                log.info(f"loading pre-trained model from {path}")

    def _resume_server(self):
        """The server optimizer's moments of the aggregate ``_resume`` loaded: rank 0 reads
        ``ddos_distilbert_server_opt.pth`` and broadcasts m / v (through the native communicator when
        it is configured).  A missing file or one of another kind fails the job on every rank -- rank
        0's verdict is broadcast first, so no rank is left waiting in a collective."""
        import torch.distributed as dist
        cfg, server = self.cfg, self.server
        err = ""
        if self.di.is_main or not self.di.distributed:
            try:
                ck.load_server_opt(server, cfg.out_dir)
            except RuntimeError as e:
                err = str(e)
        if self.di.distributed:
            if comm.broadcast_float(1.0 if err else 0.0, src=0) != 0.0:
                raise RuntimeError(err or "rank 0 could not restore the server optimizer state (see its log)")
            server.rounds = int(comm.broadcast_float(float(server.rounds), src=0))
            for t in (server.m, server.v):
                if t is None:
                    continue
                if self.comm is not None:
                    self.comm.broadcast_(t, root=0)
                else:
                    dist.broadcast(t, src=0)
        elif err:
            raise RuntimeError(err)
        self.log.info(f"server optimizer state restored from {ck.server_opt_path(cfg.out_dir)} "
                      f"({server.rounds} step(s) so far)")

    # ------------------------------------------------------------------ one round
    def run_round(self, r: int) -> Dict:
        cfg, log, model = self.cfg, self.log, self.model
        log.phase(f"Starting round {r + 1}/{cfg.rounds}")
        opt = make_optimizer(model, cfg, r, cfg.rounds, cfg.epochs * len(self.train_loader))
        opt.reset_state()  # a fresh Adam every round (client1.py:380), "has state" row flags included
        if self.privacy is not None or self.compress is not None or self.secagg is not None:
            # the round's starting weights: what the update is measured (clipped, quantized, masked) against
            if self._round_anchor is None:
                self._round_anchor = torch.empty_like(model.arena.master)
            with torch.no_grad():
                self._round_anchor.copy_(model.arena.master)
        opt_path = os.path.join(cfg.out_dir, f"client{self.client_id}_optim.pth")
        if cfg.save_optimizer and r == self.start_round:
            ck.load_optimizer(opt, opt_path)
        teacher_test = None
        if self.teacher is not None and r == self.start_round:
            # Local teacher fine-tune (BERT-base, same kernels), then distil into the student.
            log.info("training BERT-base teacher")
            t_opt = make_teacher_optimizer(self.teacher, cfg)
            with self.timer("teacher"):
                train_model(self.teacher, self.train_loader, None, t_opt, int(cfg.extra.get("teacher_epochs", cfg.epochs)),
                            log=log, use_graph=cfg.use_graph and (self.teacher_sync is None or cfg.dp_graph
                                                                  or self.teacher_sync.capturable),
                            grad_sync=self.teacher_sync)
            with self.timer("eval"):
                teacher_test = _metrics_record(evaluate_model(self.teacher, self.test_loader, log=log,
                                                              name="Teacher test"))
            self.teacher.eval()
        with self.timer("train"):
            use_graph = cfg.use_graph and (self.grad_sync is None or cfg.dp_graph or self.grad_sync.capturable)
            tr = train_model(model, self.train_loader, None, opt, cfg.epochs, log=log, use_graph=use_graph,
                             teacher=self.teacher, kd_temperature=cfg.kd_temperature, kd_alpha=cfg.kd_alpha,
                             grad_sync=self.grad_sync)
        log.info("evaluating local model on validation set...")
        with self.timer("eval"):
            val_local = evaluate_model(model, self.val_loader, log=log, name="Validation")
            log.info("evaluating local model on test set...")
            local = evaluate_model(model, self.test_loader, log=log, name="Test")
        sfx = "" if r == 0 else f"_round{r + 1}"
        if self.writer:
            save_metrics(local, os.path.join(cfg.out_dir, f"client{self.client_id}_local_metrics{sfx}.csv"), log)
            if cfg.save_checkpoints:
                ck.save_model(model, ck.client_ckpt_path(cfg.out_dir, self.client_id))
            if cfg.save_optimizer:
                ck.save_optimizer(opt, opt_path)

        # ---- FedAvg (replaces send_model -> server aggregate -> receive_aggregated_model)
        part = faults.participants(r, self.num_clients, cfg.participation, cfg.base_seed)
        contributes = self.idx in part and not faults.dropped(cfg, self.idx, r)
        weight = float(len(self.data.train)) if cfg.weighted_fedavg else 1.0
        weight /= self.topo.gpus_per_client  # k identical replicas per client share its weight
        faults.maybe_kill(self.idx, r, cfg.out_dir, self.topo.dp_rank, phase="fedavg")
        if self.health is not None:
            try:  # every client alive and here, or fail fast naming the dead rank
                self.health.barrier(f"fedavg/{r}")
            except health.PeerFailure as e:
                log.info(f"[ERROR] {e}; aborting round {r + 1} (restart resumes from the last completed round)")
                raise
        priv = None
        if self.privacy is not None and self.idx in part:
            # what is sent is the privatized copy (the local metrics and clientN_model.pth above describe
            # the trained weights); privatize, then poison: a liar lies whatever the protocol
            A = model.arena
            priv = self.privacy.privatize_(A.master, self._round_anchor, self.idx, r, len(part), shadow=A.shadow,
                                           arena=A)
            if A.shadow is not None:
                model.mark_shadow_synced()
            else:
                model.sync_shadow(force=True)
            priv = _privacy_fields(priv, self.privacy, r + 1)
            log.info(f"privatized update: |w - w_global| = {priv['update_l2']:.6g} (clipped={priv['clipped']}), "
                     f"sigma = {priv['privacy_sigma']:.6g}, epsilon <= {priv['privacy_epsilon']:.6g} at delta "
                     f"{self.privacy.delta:g} after {r + 1} round(s) (an upper bound: no subsampling amplification)")
        if self.privacy is not None:
            lost = [c for c in part if faults.dropped(cfg, c, r)]
            if lost:
                log.info(f"[WARN] sampled client(s) {[c + 1 for c in lost]} dropped from round {r + 1}: the sum "
                         f"carries less noise than the accountant assumes")
        if faults.poison_(model.arena.master, cfg, self.idx, r):  # (this client lies: utils/faults.py)
            log.info(f"[FAULT] sending a poisoned update ({cfg.poison_kind})")
        with self.timer("fedavg"):
            t0 = time.perf_counter()
            if cfg.transport == "tcp":
                # one upload per client (its replica 0, as the reference's one process per
                # client); the other replicas take the aggregate from it
                total_w = self._tcp_exchange(contributes) if self.topo.dp_rank == 0 else 0.0
                if self.topo.dp:
                    total_w = self._dp_share_model(total_w)
            elif self.robust is not None:
                total_w = fedavg_(model, participate=contributes, comm=self.comm, server=self.server,
                                  robust=self.robust)
            elif self.compress is not None:
                # privatize, then poison, then encode: quantizing a privatized update is post-processing
                total_w = fedavg_(model, participate=contributes, comm=self.comm, server=self.server,
                                  compress=self.compress, anchor=self._round_anchor, client=self.idx, round=r)
            elif self.secagg is not None:
                # privatize, then poison, then mask: what leaves is the fixed-point update under the pair streams
                total_w = fedavg_(model, participate=contributes, comm=self.comm, server=self.server,
                                  secagg=self.secagg, anchor=self._round_anchor, client=self.idx, round=r)
            else:
                total_w = fedavg_(model, weight=weight, participate=contributes, comm=self.comm, server=self.server)
            if model.device.type == "cuda":
                torch.cuda.synchronize()
            t_fed = time.perf_counter() - t0
        log.info(f"updated with aggregated model (participated={contributes}, total weight={total_w:g}, "
                 f"{t_fed * 1e3:.2f} ms)")
        norms = self.server.last if self.server is not None and total_w > 0 else None
        if norms is not None:
            log.info(f"server {self.server.kind} step: |avg - global| = {norms['delta_l2']:.6g}, "
                     f"|step| = {norms['step_l2']:.6g}")
        trim = self.robust.last if self.robust is not None and total_w > 0 else None
        if trim is not None:
            log.info(_robust_line(trim))
        comp = _compress_fields(self.compress.last) if self.compress is not None and self.compress.last else None
        if comp is not None:
            log.info(_compress_sent_line(comp))
        sec = _secagg_fields(self.secagg.last) if self.secagg is not None and self.secagg.last else None
        if sec is not None:
            log.info(_secagg_sent_line(sec))
        if self.di.is_main and cfg.save_checkpoints:
            # weights, the server optimizer's moments, then the round tag (_resume)
            ck.save_global(model, cfg.out_dir, r + 1, server=self.server)
        faults.maybe_kill(self.idx, r, cfg.out_dir, self.topo.dp_rank, phase="post_fedavg")
        log.info("evaluating aggregated model on validation set...")
        with self.timer("eval"):
            val_agg = evaluate_model(model, self.val_loader, log=log, name="Validation")
            log.info("evaluating aggregated model on test set...")
            agg = evaluate_model(model, self.test_loader, log=log, name="Test")
        if self.writer:
            save_metrics(agg, os.path.join(cfg.out_dir, f"client{self.client_id}_aggregated_metrics{sfx}.csv"), log)
        if cfg.plots and self.writer:
            with self.timer("plot"):
                from ..utils.plots import plot_evaluation, reference_dpi
                dpi = cfg.plot_dpi if cfg.plot_dpi > 0 else reference_dpi(self.client_id)
                plot_evaluation(local, agg, os.path.join(cfg.out_dir, f"client{self.client_id}_plots"),
                                f"Client {self.client_id}", dpi=dpi, log=log)
        if self.writer and cfg.save_checkpoints:
            ck.save_model(model, ck.client_ckpt_path(cfg.out_dir, self.client_id))
        rec = {"round": r + 1, "train": tr, "fedavg_ms": t_fed * 1e3, "participated": contributes,
               "local_val": _metrics_record(val_local), "local_test": _metrics_record(local),
               "aggregated_val": _metrics_record(val_agg), "aggregated_test": _metrics_record(agg)}
        if teacher_test is not None:
            rec["teacher_test"] = teacher_test
        if norms is not None:
            rec.update(delta_l2=norms["delta_l2"], step_l2=norms["step_l2"])
        if trim is not None:
            rec.update(_robust_fields(trim))
        if comp is not None:  # (after the trim keys, before privacy's: update_l2 is privacy's when both are on)
            rec.update(comp)
        if sec is not None:  # (likewise: update_l2 is privacy's when both are on)
            rec.update(sec)
        if priv is not None:
            rec.update(priv)
        elif self.privacy is not None:  # (not sampled this round: nothing of this client was released)
            rec.update(privacy_epsilon=self.privacy.epsilon(r + 1))
        self.history.append(rec)
        if self.writer:
            ck.save_fed_state(cfg.out_dir, self.client_id, {"completed_rounds": r + 1, "history": self.history})
        return rec

    def _tcp_exchange(self, contributes: bool) -> float:
        """Reference protocol: upload to the FedAvg server, download the mean (client1.py:391-395)."""
        from ..parallel import transport as tp
        cfg, log = self.cfg, self.log
        if contributes:
            ok = tp.send_model(self.model.state_dict(), cfg.server_host, cfg.port_receive, cfg.gzip_level,
                               cfg.timeout_s, log)
            if not ok:
                log.info("skipping aggregated model evaluation due to send failure")
                return 0.0
        agg = tp.receive_aggregated_model(cfg.server_host, cfg.port_send, timeout=cfg.timeout_s, log=log)
        if agg is None:
            log.info("skipping aggregated model evaluation due to connection failure")
            return 0.0
        self.model.load_state_dict(agg)
        return float(self.num_clients)

    def _dp_share_model(self, total_w: float) -> float:
        """Replica 0 of this client -> the client's other replicas: weights + FedAvg weight."""
        import torch.distributed as dist
        A = self.model.arena
        src = self.topo.client_ranks(self.topo.client_idx)[0]
        dist.broadcast(A.master, src=src, group=self.topo.dp_group)
        t = torch.tensor([total_w], dtype=torch.float64, device=A.device)
        dist.broadcast(t, src=src, group=self.topo.dp_group)
        if hasattr(self.model, "sync_shadow"):
            self.model.sync_shadow(force=True)
        return float(t.item())

    # ------------------------------------------------------------------ all rounds
    def run(self) -> Dict:
        self.setup()
        try:
            for r in range(self.start_round, self.cfg.rounds):
                self.run_round(r)
            report = self.report()
        finally:
            health.stop()
        self.log.phase("Client shutdown")
        return report

    def report(self) -> Dict:
        """Cross-client summary on rank 0 (gathered with an all-gather of small vectors)."""
        last = self.history[-1] if self.history else None
        vec = [0.0] * 8
        if last:
            a, l_ = last["aggregated_test"], last["local_test"]
            vec = [a["accuracy"], a["f1"], a["precision"], a["recall"], l_["accuracy"], l_["f1"],
                   last["train"]["batches_per_sec"], last["fedavg_ms"]]
        allv = comm.all_gather_floats(vec)[::self.topo.gpus_per_client]  # replica 0 of each client
        rep = {"clients": [{"client": i + 1, "aggregated_test_accuracy": v[0], "aggregated_test_f1": v[1],
                            "aggregated_test_precision": v[2], "aggregated_test_recall": v[3],
                            "local_test_accuracy": v[4], "local_test_f1": v[5], "train_batches_per_sec": v[6],
                            "fedavg_ms": v[7]} for i, v in enumerate(allv)],
               "rounds": self.cfg.rounds, "world_size": self.di.world_size,
               "gpus_per_client": self.topo.gpus_per_client, "phases_s": self.timer.summary()}
        if getattr(self, "privacy", None) is not None:
            # spent over the whole run, without subsampling amplification: an upper bound
            rep.update(privacy_epsilon=self.privacy.epsilon(self.cfg.rounds), privacy_delta=self.privacy.delta,
                       privacy_clip=self.privacy.clip, privacy_noise=self.privacy.noise_multiplier)
        robust = getattr(self, "robust", None)
        if robust is not None and robust.last is not None and "kind" in robust.last:
            rep["robust"] = robust.last  # the last round's multi-Krum / geometric-median report
        if self.di.is_main:
            path = os.path.join(self.cfg.out_dir, "federated_report.json")
            with open(path, "w") as f:
                json.dump(rep, f, indent=1)
            self.log.info(f"federated report written to {path}")
        return rep


def _privacy_line(privacy, rounds: int) -> str:
    """One log line for a private run: the mechanism and what ``rounds`` rounds of it spend."""
    return (f"client-level privacy: clip C = {privacy.clip:g}, noise multiplier z = {privacy.noise_multiplier:g} "
            f"(each of a round's M sampled clients adds N(0, (z C)^2 / M)); {rounds} round(s) spend epsilon <= "
            f"{privacy.epsilon(rounds):.6g} at delta {privacy.delta:g} (an upper bound: no subsampling "
            f"amplification is credited)")


def _privacy_fields(rep: Dict, privacy, rounds_done: int) -> Dict:
    """A record's privacy keys from ``Privatizer.privatize_``'s report."""
    return {"update_l2": rep["update_l2"], "clipped": rep["clipped"], "privacy_sigma": rep["sigma"],
            "privacy_epsilon": privacy.epsilon(rounds_done)}


def _compress_line(compress) -> str:
    """One log line for a job with the quantized or sparsified exchange."""
    from ..parallel.compress import TopKCompressor, payload_ratio
    if isinstance(compress, TopKCompressor):
        return (f"sparsified update exchange: {compress.describe()}, error feedback "
                f"{'on' if compress.error_feedback else 'off'} (about 6 bytes per sent entry)")
    return (f"quantized update exchange: {compress.describe()}, {compress.rounding} rounding, error feedback "
            f"{'on' if compress.error_feedback else 'off'} (payload {payload_ratio(compress.bits):.2f}x smaller than fp32)")


def _compress_fields(rep: Dict) -> Dict:
    """A record's compression keys from ``Compressor.encode_``'s (or ``TopKCompressor.encode_``'s) report."""
    out = {"compress_ratio": rep["ratio"], "payload_bytes": rep["payload_bytes"], "update_l2": rep["update_l2"],
           "quant_error_l2": rep["error_l2"]}
    if "bad_groups" in rep:
        out["bad_groups"] = rep["bad_groups"]
    else:  # top-k: the norm held back, the elements left out, the entries sent and the smallest of them
        out.update(bad_elems=rep["bad_elems"], sent=rep["sent"], threshold=rep["threshold"])
    return out


def _compress_sent_line(comp: Dict) -> str:
    if "sent" in comp:
        return (f"sparsified update: {comp['sent']} entries >= {comp['threshold']:.6g} in {comp['payload_bytes']} B "
                f"({comp['compress_ratio']:.2f}x smaller), |update| = {comp['update_l2']:.6g}, |held back| = "
                f"{comp['quant_error_l2']:.6g}"
                + (f", [WARN] {comp['bad_elems']} element(s) with inf / NaN left out" if comp["bad_elems"] else ""))
    return (f"quantized update: {comp['payload_bytes']} B sent ({comp['compress_ratio']:.2f}x smaller), |update| = "
            f"{comp['update_l2']:.6g}, |quantization error| = {comp['quant_error_l2']:.6g}"
            + (f", [WARN] {comp['bad_groups']} group(s) with inf / NaN sent as zero" if comp["bad_groups"] else ""))


def _secagg_line(secagg, n_clients: int) -> str:
    """One log line for a job with secure aggregation."""
    return (f"secure aggregation: {secagg.describe()}, pairwise X25519 keys among {n_clients} client(s); "
            f"honest-but-curious participants, no dropout recovery (parallel/secagg.py states the limits)")


def _secagg_fields(rep: Dict) -> Dict:
    """A record's secure-aggregation keys from ``SecureAggregator.mask_``'s report."""
    return {"payload_bytes": rep["payload_bytes"], "update_l2": rep["update_l2"], "quant_error_l2": rep["error_l2"],
            "clamped": rep["clamped"], "bad_elems": rep["bad_elems"], "masked_with": rep["masked_with"]}


def _secagg_sent_line(sec: Dict) -> str:
    return (f"masked update: {sec['payload_bytes']} B sent under {sec['masked_with']} pair stream(s), |update| = "
            f"{sec['update_l2']:.6g}, |fixed-point error| = {sec['quant_error_l2']:.6g}"
            + (f", [WARN] {sec['clamped']} element(s) clamped at +-2^27 steps" if sec["clamped"] else "")
            + (f", [WARN] {sec['bad_elems']} element(s) with inf / NaN sent as zero" if sec["bad_elems"] else ""))


def _trim_line(trim: Dict) -> str:
    """One log line for a robust round: the most-trimmed slot (the j-th participating client, in
    client order) and its share; honest i.i.d. clients sit near 2k / M each."""
    j, share = most_trimmed(trim)
    return (f"robust aggregate of {trim['clients']} client(s), k = {trim['k']}: most trimmed is participant "
            f"{j + 1} with share {share:.4f} (honest expectation {2 * trim['k'] / max(trim['clients'], 1):.4f})")


def _dist_setup_note(robust) -> str:
    if robust.aggregator == "multi_krum":
        f = "(M - 3) // 2" if robust.byzantine is None else str(robust.byzantine)
        return f" (byzantine f = {f}, krum_select m = {'M - f' if robust.krum_select is None else robust.krum_select})"
    if robust.aggregator == "geometric_median":
        return f" ({robust.geomed_iters} Weiszfeld iterations, nu {robust.geomed_nu:g})"
    return ""


def _robust_fields(trim: Dict) -> Dict:
    """A record's robust-aggregation keys: the trimmed shares of the coordinate-wise kinds, the whole
    report (under ``robust``) of the distance-based ones."""
    if "kind" in trim:
        return {"robust": trim}
    return {"trimmed_share": trim["trimmed_share"], "k": trim["k"]}


def _robust_line(trim: Dict) -> str:
    """One log line for a robust round, by the report's kind: the rejected participants (multi-Krum), the
    lowest-weight participant beside the uniform 1 / M (geometric median), or ``_trim_line``."""
    kind = trim.get("kind")
    if kind == "multi_krum":
        rej = ", ".join(f"{j + 1} (score {trim['scores'][j]:.6g})" for j in trim["rejected"]) or "none"
        return (f"multi-Krum of {trim['clients']} client(s), f = {trim['f']}, m = {trim['m']}: rejected "
                f"participant(s) {rej}")
    if kind == "geometric_median":
        w = trim["weights"]
        j = min(range(len(w)), key=lambda i: (w[i], i))
        return (f"geometric median of {trim['clients']} client(s), {trim['iters']} iteration(s): lowest weight is "
                f"participant {j + 1} with {w[j]:.6f} (uniform {1.0 / max(trim['clients'], 1):.6f})")
    return _trim_line(trim)


@torch.no_grad()
def _average_masters(model, states: List[torch.Tensor], server=None) -> Optional[Dict]:
    """``fedavg_``'s arithmetic in one process: the SUM of the clients' fp32 masters (what the
    all-reduce computes; for two clients a + b is exact in any order), then the fused 1/N scale +
    bf16 shadow refresh (``scale_cast``) on GPU -- or, with a server optimizer, its step on that sum
    (``ServerOptimizer.apply_``, whose norms are returned)."""
    A = model.arena
    A.master.copy_(states[0])
    for s in states[1:]:
        A.master.add_(s)
    if server is not None:
        return server.apply_(model, float(len(states)))
    if A.master.is_cuda:
        from ..ops import kernels as K
        K.scale_cast(A.master, A.shadow, 1.0 / len(states))
        model.mark_shadow_synced()
    else:
        A.master.mul_(1.0 / len(states))
        model.sync_shadow(force=True)


def warm_start(client: "FederatedClient", epochs: int = 1, rows: int = 225_745, seed: int = 1,
               profile: str = "default", fraction: float = 0.1) -> Dict:
    """A shared "pretrained" starting point for every client (the reference fine-tunes a PRETRAINED
    DistilBERT, client1.py:56, so its clients start near one point; no weights can be downloaded
    here): ``client.model`` is trained ``epochs`` epochs on a public synthetic sample -- a separate
    file (generator seed ``seed``, profile ``profile``) that no client samples from -- with a fresh
    Adam.  The model's dropout counters are then reset, so the federated clients start exactly as
    they would from a loaded checkpoint.  Returns the training record and the public test metrics."""
    cfg, model = client.cfg, client.model
    frame = generate_cicids2017(rows, seed=seed, profile=profile)
    data = build_client_data(frame, 0, fraction, cfg.base_seed + 1000, cfg.max_len, client.tokenizer)
    dev = model.device
    loader = DeviceLoader(data.train, cfg.batch_size, shuffle=True, device=dev, seed=cfg.base_seed + 1000)
    opt = make_optimizer(model, cfg)
    opt.reset_state()
    tr = train_model(model, loader, None, opt, epochs, log=client.log, use_graph=cfg.use_graph)
    test = _metrics_record(evaluate_model(model, DeviceLoader(data.test, cfg.eval_batch_size, device=dev),
                                          name="Public warm-start test"))
    opt.reset_state()  # (also clears the "has Adam state" word-row flags)
    with torch.no_grad():
        model.rng.zero_()
    model.torch_counter = 0
    if getattr(client, "server", None) is not None:
        client.server.reset(model)  # the server optimizer starts from the warm weights, moments cleared
    return {"train": tr, "public_test": test, "rows": rows, "seed": seed, "profile": profile,
            "train_rows": len(data.train)}


def _pooled(recs, key: str):
    return [[sum(r[key]["confusion_matrix"][i][j] for r in recs if len(r[key]["confusion_matrix"]) == 2)
             for j in range(2)] for i in range(2)]


def run_virtual_clients(client: "FederatedClient", n_clients: int = 2, rounds: int = 1,
                        progress=None) -> Dict:
    """``rounds`` FedAvg rounds of ``n_clients`` federated clients on THIS process's device, the
    clients trained one after another (a 1-GPU job: ``bench.py`` quality half with
    ``--virtual-clients N --rounds R``, ``cli launch --virtual-clients``).

    Reference protocol (client1.py / client2.py + server.py:67-79): client k samples its own 10 %
    of the file with seed 42 + k (client1.py:89, client2.py:84), every client starts from the same
    weights (round 1: the model's broadcast init; round r > 1: round r-1's aggregate --
    the reference's next round is a re-run of the scripts that loads the aggregate,
    client1.py:375-377), trains ``cfg.epochs`` local epochs with a FRESH Adam (client1.py:380
    re-creates it every run), is evaluated on its test split, the server averages the fp32 state
    dicts (unweighted mean; ``_average_masters`` = fedavg_'s sum + ``scale_cast``) and every client
    then evaluates the aggregate on its own test split (client1_aggregated_metrics.csv).

    Each virtual client keeps, across rounds, exactly the state a real client process keeps in
    ``FederatedClient.run`` (one process per client): its shuffling loader (the epoch permutations
    continue) and its dropout counters (``model.rng`` / ``torch_counter``), so for the same config
    the R-round virtual run equals the N-rank collective ``run_federated`` run bit for bit
    (tests/test_virtual_rounds.py, N = 2, R = 2 on gloo).

    With a server optimizer (``cfg.server_opt``, parallel/server_opt.py) the job's ``client.server`` --
    the object ``run_round`` hands to ``fedavg_`` -- makes its step on the same sum instead of the 1/N
    scale, and each round's record carries its ``delta_l2`` / ``step_l2``
    (tests/test_server_opt_cpu.py: equal to the 2-rank gloo run bit for bit).

    With a robust aggregator (``cfg.aggregator``, parallel/robust.py) ``robust_aggregate_`` takes the
    place of ``_average_masters`` -- the call ``fedavg_(..., robust=)`` makes on the gathered rows -- and
    each round's record carries ``trimmed_share`` / ``k`` (tests/test_robust_agg_cpu.py: equal to the
    3-rank gloo run bit for bit); the distance-based kinds (parallel/robust_dist.py) go through
    ``robust.aggregate_`` and the record carries their report under ``robust``
    (tests/test_robust_dist_cpu.py).  A poisoned client (``cfg.poison_client``, utils/faults.py) sends a
    changed copy of its weights; its local metrics are those of the weights it trained.

    With client-level privacy (``cfg.privacy_clip``, parallel/privacy.py) every client's copy is clipped
    and noised against the round's start before it is aggregated (and before a poisoner changes it) --
    the call ``run_round`` makes on its master -- and each client record carries ``update_l2`` /
    ``clipped`` / ``privacy_sigma`` / ``privacy_epsilon``, the round record ``privacy_epsilon``
    (tests/test_privacy_cpu.py: equal to the 2-rank gloo run bit for bit under a fixed seed).

    With the quantized exchange (``cfg.compress``, parallel/compress.py) every client's copy -- after
    privacy and poisoning -- is encoded against the round's start with the client's own residual (the
    job's ``client.compress`` keeps one per virtual client), and ``decode_mean_`` of the payloads takes the
    place of ``_average_masters``: the calls ``fedavg_(..., compress=)`` makes.  Each client record carries
    ``compress_ratio`` / ``payload_bytes`` / ``update_l2`` / ``quant_error_l2`` / ``bad_groups``
    (tests/test_compress_cpu.py: equal to the 2-rank gloo run bit for bit).

    With secure aggregation (``cfg.secagg``, parallel/secagg.py) every client's copy -- after privacy and
    poisoning -- is masked against the round's start with its own key pair (the job's ``client.secagg`` holds
    one per virtual client: the arithmetic is exercised, nothing is hidden), and ``unmask_mean_`` of the
    payloads takes the place of ``_average_masters``: the calls ``fedavg_(..., secagg=)`` makes.  Each client
    record carries ``payload_bytes`` / ``update_l2`` / ``quant_error_l2`` / ``clamped`` / ``bad_elems`` /
    ``masked_with`` (tests/test_secagg_cpu.py: equal to the 2-rank gloo run bit for bit).

    Returns ``rounds`` (one record per round: per-client local / aggregated metrics, the pooled
    aggregated confusion, the FedAvg time) plus the LAST round's ``clients`` /
    ``aggregated_confusion`` / ``fedavg_ms`` at the top level (the 1-round API of earlier rounds).

    With a teacher (the distillation extension, BASELINE.json config 5) every virtual client does
    what ``run_round`` does for a real one: in its first round the shared BERT-base teacher init is
    fine-tuned on the client's own split (``teacher_epochs``) and kept for the later rounds (the
    teachers stay local, as in run_round), then the client's student is distilled from it; the
    students are averaged.  Each first-round record then also holds the client's ``teacher_test``."""
    cfg, model = client.cfg, client.model
    if client.di.distributed:
        raise RuntimeError("virtual clients run in a single-process job (world size 1)")
    teacher = client.teacher
    dev = model.device
    A = model.arena
    glob = A.master.detach().clone()  # what every client starts the round from
    # the job's FedOpt server optimizer (None: plain FedAvg) -- the object run_round hands to fedavg_
    server = getattr(client, "server", None)
    if server is not None and not torch.equal(server.x, glob):
        # the weights were replaced after setup() (a checkpoint loaded by hand): the server's x is the
        # global model by definition, and moments of other weights mean nothing
        client.log.info("[WARN] the model changed since the server optimizer was built: server state reset")
        server.reset(model)
    robust = make_robust(cfg)  # (None: the plain mean -- _average_masters, untouched)
    # the job's Privatizer (None: privacy_clip == 0) -- one object, so one seed, for every virtual client
    privacy = getattr(client, "privacy", None)
    # the job's Compressor (None: compress == "none") -- it keeps one residual per virtual client
    compress = getattr(client, "compress", None)
    if compress is not None and robust is not None:
        raise ValueError("compress needs aggregator='mean'")
    # the job's SecureAggregator (None: secagg off) -- one key pair per virtual client, all in this process
    secagg = getattr(client, "secagg", None)
    if secagg is not None:
        if robust is not None or compress is not None:
            raise ValueError("secagg needs aggregator='mean' and compress='none'")
        if sorted(secagg.private) != list(range(n_clients)):
            secagg.setup_keys(range(n_clients), n_clients)
    t_init = teacher.arena.master.detach().clone() if teacher is not None else None
    say = progress or (lambda msg: None)
    # per-client state that survives the rounds (a real client's process keeps it)
    cs = []
    for v in range(n_clients):
        data = build_client_data(client.frame, v, cfg.data_fraction, cfg.base_seed, cfg.max_len, client.tokenizer,
                                 cfg.partition, n_clients, partition_skew=cfg.partition_skew)
        cs.append({"data": data,
                   "loader": DeviceLoader(data.train, cfg.batch_size, shuffle=True, device=dev,
                                          seed=cfg.client_seed(v)),
                   "test": DeviceLoader(data.test, cfg.eval_batch_size, device=dev),
                   "rng": model.rng.detach().clone(), "torch_counter": model.torch_counter, "teacher": None})
    hist = []
    for r in range(rounds):
        locals_, recs, payloads = [], [], []
        for v, c in enumerate(cs):
            data, loader, test = c["data"], c["loader"], c["test"]
            rec = {"client": v + 1, "round": r + 1, "train_rows": len(data.train), "test_rows": len(data.test)}
            t0 = time.perf_counter()
            if teacher is not None:
                if c["teacher"] is None:
                    with torch.no_grad():
                        teacher.arena.master.copy_(t_init)
                    teacher.sync_shadow(force=True)
                    t_opt = make_teacher_optimizer(teacher, cfg)
                    t_opt.reset_state()
                    teacher.train()
                    rec["teacher_train"] = train_model(
                        teacher, loader, None, t_opt, int(cfg.extra.get("teacher_epochs", cfg.epochs)),
                        log=client.log, use_graph=cfg.use_graph)
                    rec["teacher_test"] = _metrics_record(evaluate_model(teacher, test,
                                                                         name=f"Client {v + 1} teacher test"))
                    c["teacher"] = teacher.arena.master.detach().clone()
                    del t_opt
                else:
                    with torch.no_grad():
                        teacher.arena.master.copy_(c["teacher"])
                    teacher.sync_shadow(force=True)
                teacher.eval()
            with torch.no_grad():
                A.master.copy_(glob)
                model.rng.copy_(c["rng"])
            model.torch_counter = c["torch_counter"]
            model.sync_shadow(force=True)
            opt = make_optimizer(model, cfg, r, rounds, cfg.epochs * len(loader))
            opt.reset_state()  # (also clears the sparse word rows' "has Adam state" flags)
            tr = train_model(model, loader, None, opt, cfg.epochs, log=client.log, use_graph=cfg.use_graph,
                             teacher=teacher, kd_temperature=cfg.kd_temperature, kd_alpha=cfg.kd_alpha)
            with torch.no_grad():
                c["rng"].copy_(model.rng)
            c["torch_counter"] = model.torch_counter
            local = _metrics_record(evaluate_model(model, test, name=f"Client {v + 1} local test"))
            locals_.append(A.master.detach().clone())
            if privacy is not None:  # (clip + noise against the round's start; then a liar may still lie)
                rec.update(_privacy_fields(privacy.privatize_(locals_[-1], glob, v, r, n_clients, arena=A), privacy,
                                           r + 1))
            faults.poison_(locals_[-1], cfg, v, r)  # (a lying client: what it sends, not what it evaluated)
            if compress is not None:  # (what leaves the client: codes and scales of its update + residual)
                payloads.append(compress.encode_(locals_[-1], glob, v, r))
                for key, val in _compress_fields(compress.last).items():
                    rec.setdefault(key, val)  # (update_l2 stays privacy's when both are on)
            if secagg is not None:  # (what leaves the client: its fixed-point update under the pair streams)
                payloads.append(secagg.mask_(locals_[-1], glob, v, r, range(n_clients)))
                for key, val in _secagg_fields(secagg.last).items():
                    rec.setdefault(key, val)
            rec.update({"train": tr, "train_wall_s": time.perf_counter() - t0, "local_test": local})
            # client drift: how far the local epochs moved this client from the round's start
            rec["l2_local_to_start"] = float((locals_[-1] - glob).norm())
            recs.append(rec)
            del opt
            say(f"round {r + 1}/{rounds} client {v + 1}/{n_clients}: local acc {local['accuracy']:.3f} % "
                f"f1 {local['f1']:.5f} ({tr['steps']} steps, {time.perf_counter() - t0:.1f} s)")
        t0 = time.perf_counter()
        norms = trim = None
        if robust is not None:
            if robust.aggregator in DIST_AGGREGATORS:
                trim = robust.aggregate_(model, locals_, server)
            else:
                trim = robust_aggregate_(model, locals_, robust.k(len(locals_)), server)
            norms = server.last if server is not None else None
        elif compress is not None:
            compress.decode_mean_(model, payloads, glob, server)
            norms = server.last if server is not None else None
            del payloads
        elif secagg is not None:
            secagg.unmask_mean_(model, payloads, glob, server, round=r)
            norms = server.last if server is not None else None
            del payloads
        elif server is None:
            _average_masters(model, locals_)
        else:
            norms = _average_masters(model, locals_, server)
        if dev.type == "cuda":
            torch.cuda.synchronize()
        fed_ms = 1e3 * (time.perf_counter() - t0)
        agg = A.master.detach()
        for rec, c, loc in zip(recs, cs, locals_):
            rec["aggregated_test"] = _metrics_record(evaluate_model(model, c["test"], name=f"Client {rec['client']} "
                                                                                           "aggregated test"))
            rec["rel_l2_local_to_aggregate"] = float((loc - agg).norm() / loc.norm().clamp_min(1e-30))
        glob = agg.clone()
        del locals_
        pooled = _pooled(recs, "aggregated_test")
        hist.append({"round": r + 1, "clients": recs, "fedavg_ms": fed_ms, "aggregated_confusion": pooled,
                     "local_confusion": _pooled(recs, "local_test")})
        if norms is not None:  # the server step: how far the average drifted, how far the server moved
            hist[-1].update(delta_l2=norms["delta_l2"], step_l2=norms["step_l2"])
        if trim is not None:  # how often each client's value was the one trimmed (parallel/robust.py)
            hist[-1].update(_robust_fields(trim))
            client.log.info(_robust_line(trim))
            say(f"round {r + 1}/{rounds} " + _robust_line(trim))
        if compress is not None:
            up = math.sqrt(sum(c["update_l2"] ** 2 for c in recs)) if privacy is None else None
            er = math.sqrt(sum(c["quant_error_l2"] ** 2 for c in recs))
            hist[-1].update(compress_ratio=recs[0]["compress_ratio"], payload_bytes=recs[0]["payload_bytes"],
                            quant_error_l2=er)
            if "bad_groups" in recs[0]:
                hist[-1].update(bad_groups=sum(c["bad_groups"] for c in recs))
                say(f"round {r + 1}/{rounds} quantized exchange: {compress.describe()}, {recs[0]['payload_bytes']} B per "
                    f"client ({recs[0]['compress_ratio']:.2f}x smaller), pooled |quantization error| = {er:.6g}"
                    + (f" of |update| = {up:.6g}" if up is not None else ""))
            else:
                hist[-1].update(bad_elems=sum(c["bad_elems"] for c in recs), sent=sum(c["sent"] for c in recs))
                say(f"round {r + 1}/{rounds} sparsified exchange: {compress.describe()}, {recs[0]['payload_bytes']} B per "
                    f"client ({recs[0]['compress_ratio']:.2f}x smaller), pooled |held back| = {er:.6g}"
                    + (f" of |update| = {up:.6g}" if up is not None else ""))
        if secagg is not None:
            er = math.sqrt(sum(c["quant_error_l2"] ** 2 for c in recs))
            hist[-1].update(payload_bytes=recs[0]["payload_bytes"], quant_error_l2=er,
                            clamped=sum(c["clamped"] for c in recs), bad_elems=sum(c["bad_elems"] for c in recs),
                            masked_with=recs[0]["masked_with"])
            say(f"round {r + 1}/{rounds} secure aggregation: {secagg.describe()}, {recs[0]['payload_bytes']} B per "
                f"client under {recs[0]['masked_with']} pair stream(s), pooled |fixed-point error| = {er:.6g}")
        if privacy is not None:
            hist[-1].update(privacy_epsilon=privacy.epsilon(r + 1))
            say(f"round {r + 1}/{rounds} privacy: epsilon <= {hist[-1]['privacy_epsilon']:.6g} at delta "
                f"{privacy.delta:g} (an upper bound: no subsampling amplification), clipped "
                f"{[c['clipped'] for c in recs]}")
        (tn, fp), (fn, tp) = pooled
        say(f"round {r + 1}/{rounds} aggregate: pooled acc {100.0 * (tp + tn) / max(tp + tn + fp + fn, 1):.3f} %")
    last = hist[-1]
    return {"clients": last["clients"], "fedavg_ms": last["fedavg_ms"],
            "aggregated_confusion": last["aggregated_confusion"], "rounds": hist}


def run_federated(cfg: FedConfig, frame=None, model_config: Optional[DistilBertConfig] = None) -> Dict:
    client = FederatedClient(cfg, frame, model_config)
    try:
        return client.run()
    finally:
        client.log.close()
