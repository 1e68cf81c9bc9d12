"""FedOpt server optimizers: FedAvgM, FedAdagrad, FedAdam, FedYogi.

Reddi et al., "Adaptive Federated Optimization" (ICLR 2021); FedAvgM: Hsu et al., "Measuring the
Effects of Non-Identical Data Distribution for Federated Visual Classification".  The round's
weighted mean is not taken as the new global model; ``avg - w_global`` is a pseudo-gradient and the
server makes an optimizer step of its own with it.  Per element, with ``s`` the all-reduced weighted
sum (``arena.master`` after the all-reduce), ``inv = float32(1 / total_weight)``, ``x`` the server's
current global weights and ``m`` / ``v`` its moments::

    avg   = s * inv
    d     = avg - x
    avgm    : m = b1*m + d                         ; x' = x + eta*m
    adagrad : m = b1*m + (1-b1)*d ; v = v + d*d
    adam    : m = b1*m + (1-b1)*d ; v = b2*v + (1-b2)*d*d
    yogi    : m = b1*m + (1-b1)*d ; v = v - (1-b2)*d*d*sign(v - d*d)
    adaptive: x' = x + eta * m / (sqrt(v) + tau)

No bias correction (as in the paper); ``m0 = 0``, ``v0 = tau^2``.  Everything is fp32: the
hyper-parameters are rounded to fp32 first, ``1 - b`` is the fp32 difference, and every product, sum,
quotient and root is rounded on its own in the order ``torch_chain_`` spells out.  On the GPU the
whole step is ONE launch (``ops.kernels.server_opt``: the pass ``scale_cast`` makes for plain FedAvg,
with three more streams) that also writes the bf16 shadow and the two norms a round logs; on the CPU
it is ``torch_chain_`` itself.  An alignment pad of the arena has ``s = x = m = +0``, so ``d = +0``
and it stays ``+0``.

Every rank holds the same server state and applies the same step to the same all-reduced sum, so the
ranks stay identical as they do after ``scale_cast``; a dropped / non-participating client contributes
weight 0 and still makes the server step.

Memory: ``x``, ``m`` and ``v`` are flat fp32 tensors shaped like ``arena.master`` -- for DistilBERT
(66.4 M parameters) 3 x 265 MB = +0.8 GB per rank (``avgm`` keeps no ``v``: +0.53 GB).
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence

import torch

KINDS = ("avgm", "adagrad", "adam", "yogi")
ADAPTIVE = ("adagrad", "adam", "yogi")


def f32(value: float) -> float:
    """``value`` rounded to fp32, as a Python float (what a kernel argument of type float holds)."""
    return float(torch.tensor(float(value), dtype=torch.float32).item())


def one_minus_f32(b: float) -> float:
    """``1 - b`` as the kernel forms it: the fp32 difference of fp32 values."""
    return float((torch.tensor(1.0, dtype=torch.float32) - torch.tensor(float(b), dtype=torch.float32)).item())


def hyper_f32(lr, betas, tau):
    """(lr, b1, b2, tau) checked and rounded to fp32; a ValueError names what is out of range."""
    try:
        b1, b2 = (float(b) for b in betas)
        lr, tau = float(lr), float(tau)
    except (TypeError, ValueError):
        raise ValueError(f"server_lr / server_tau must be numbers and server_betas two numbers, got "
                         f"{lr!r}, {tau!r}, {betas!r}") from None
    if not (math.isfinite(lr) and lr > 0.0):
        raise ValueError(f"server_lr must be finite and > 0, got {lr!r}")
    if not (math.isfinite(tau) and tau > 0.0):
        raise ValueError(f"server_tau must be finite and > 0, got {tau!r}")
    if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
        raise ValueError(f"server_betas must lie in [0, 1), got {(b1, b2)!r}")
    out = f32(lr), f32(b1), f32(b2), f32(tau)
    if not (out[0] > 0.0 and out[3] > 0.0 and out[1] < 1.0 and out[2] < 1.0 and math.isfinite(out[0])):
        raise ValueError("server optimizer hyper-parameters leave their range when rounded to fp32")
    return out


@torch.no_grad()
def torch_chain_(kind: str, s: torch.Tensor, x: torch.Tensor, m: torch.Tensor, v: Optional[torch.Tensor],
                 inv: float, eta: float, b1: float, b2: float, tau: float):
    """The specification, literally: one server step as torch ops in the tensors' dtype (fp32 in
    production; the tests also run it in fp64 as the exact reference), every op rounded on its own.
    ``s`` is the weighted sum; ``x``, ``m``, ``v`` are updated in place.  Returns ``d`` and ``x' - x``.
    The scalars must already be fp32 values (``f32``)."""
    c1, c2 = one_minus_f32(b1), one_minus_f32(b2)
    avg = s * inv
    d = avg - x
    if kind == "avgm":
        m.mul_(b1)
        m.add_(d)
        step = m * eta
    else:
        t = d * c1
        m.mul_(b1)
        m.add_(t)
        d2 = d * d
        if kind == "adagrad":
            v.add_(d2)
        elif kind == "adam":
            t2 = d2 * c2
            v.mul_(b2)
            v.add_(t2)
        elif kind == "yogi":
            sg = torch.sign(v - d2)
            t2 = d2 * c2
            t2.mul_(sg)
            v.sub_(t2)
        else:
            raise ValueError(f"unknown server optimizer {kind!r}")
        den = torch.sqrt(v)
        den.add_(tau)
        step = m * eta
        step.div_(den)
    xn = x + step
    dx = xn - x
    x.copy_(xn)
    return d, dx


class ServerOptimizer:
    """The server's optimizer state for one model: ``x`` (the global weights the clients started the
    round from), ``m`` and -- for the adaptive kinds -- ``v``, each a flat fp32 tensor like
    ``model.arena.master`` on its device (+0.8 GB per rank for DistilBERT; see the module docstring).

    ``apply_(model, total_weight)`` turns the weighted SUM in ``arena.master`` into the new global
    model.  ``x`` always equals the global model, so it is not part of ``state_dict()``."""

    def __init__(self, model, kind: str, lr: float = 1.0, betas: Sequence[float] = (0.9, 0.99), tau: float = 1e-3):
        if kind not in KINDS:
            raise ValueError(f"server_opt must be one of fedavg, {', '.join(KINDS)}; got {kind!r}")
        self.kind = kind
        self.adaptive = kind in ADAPTIVE
        self.lr, self.b1, self.b2, self.tau = hyper_f32(lr, betas, tau)
        master = model.arena.master
        self.x = torch.empty_like(master)
        self.m = torch.empty_like(master)
        self.v = torch.empty_like(master) if self.adaptive else None
        self.rounds = 0
        self.last: Optional[Dict[str, float]] = None  # the norms of the latest step
        self._stats = None
        if master.is_cuda:
            from ..ops import kernels as K
            self._stats = torch.zeros(2 * K.server_opt_grid(master.numel()), dtype=torch.float32,
                                      device=master.device)
        self.reset(model)

    @torch.no_grad()
    def reset(self, model):
        """Start over from the model's current weights: ``x`` <- master, ``m`` <- 0, ``v`` <- tau^2."""
        self.x.copy_(model.arena.master)
        self.m.zero_()
        if self.v is not None:
            # (fp32 tau * tau, a pad's v included: nothing reads a pad's v but its own recurrence)
            self.v.fill_(f32(self.tau * self.tau))
        self.rounds = 0

    @torch.no_grad()
    def apply_(self, model, total_weight: float) -> Dict[str, float]:
        """``arena.master`` holds the weighted sum of the clients' weights and ``total_weight`` their
        total weight: make the server step, leave the new global model in the master (and the bf16
        shadow), and return the l2 norms of the pseudo-gradient and of the step."""
        A = model.arena
        total = float(total_weight)
        if not (math.isfinite(total) and total > 0.0):
            raise ValueError(f"server step with total weight {total_weight!r}")
        inv = f32(1.0 / total)
        if A.master.is_cuda:
            from ..ops import kernels as K
            K.server_opt(A.master, self.x, self.m, self.v, A.shadow, self.kind, inv, self.lr, self.b1, self.b2,
                         self.tau, self._stats)
            model.mark_shadow_synced()
            sums = self._stats.view(-1, 2).sum(dim=0, dtype=torch.float64).tolist()
        else:
            d, dx = torch_chain_(self.kind, A.master, self.x, self.m, self.v, inv, self.lr, self.b1, self.b2,
                                 self.tau)
            A.master.copy_(self.x)
            model.sync_shadow(force=True)
            sums = [float(d.double().square().sum()), float(dx.double().square().sum())]
        self.rounds += 1
        self.last = {"delta_l2": math.sqrt(sums[0]), "step_l2": math.sqrt(sums[1])}
        return self.last

    # ------------------------------------------------------------------ persistence
    def state_dict(self) -> Dict:
        sd = {"kind": self.kind, "lr": self.lr, "betas": [self.b1, self.b2], "tau": self.tau,
              "rounds": int(self.rounds), "m": self.m.detach().to("cpu").clone()}
        if self.v is not None:
            sd["v"] = self.v.detach().to("cpu").clone()
        return sd

    @torch.no_grad()
    def load_state_dict(self, sd: Dict):
        """Moments and round count of a saved state (``x`` is the global model: ``reset`` snapshots it
        and this call leaves it alone).  The kind and the moments' size must match; a changed
        rate / beta / tau is the configuration's to decide and is kept."""
        if sd.get("kind") != self.kind:
            raise ValueError(f"server optimizer state is of kind {sd.get('kind')!r}, this job runs {self.kind!r}")
        if self.adaptive != ("v" in sd) or tuple(sd["m"].shape) != tuple(self.m.shape) or (
                self.adaptive and tuple(sd["v"].shape) != tuple(self.v.shape)):
            raise ValueError("server optimizer state does not fit this model")
        self.m.copy_(sd["m"])
        if self.v is not None:
            self.v.copy_(sd["v"])
        self.rounds = int(sd.get("rounds", 0))


def check_server_config(cfg) -> Optional[str]:
    """The configuration's server optimizer kind (None for plain FedAvg), or a ValueError for an
    unknown kind or a transport it does not run over.  Needs no model: callers refuse a bad
    configuration before any work."""
    kind = str(cfg.server_opt).lower()
    if kind == "fedavg":
        return None
    if kind not in KINDS:
        raise ValueError(f"server_opt must be one of fedavg, {', '.join(KINDS)}; got {cfg.server_opt!r}")
    if getattr(cfg, "transport", "collective") == "tcp":
        raise ValueError(f"server_opt={kind!r} needs transport='collective': the reference-compatible TCP server "
                         f"keeps the reference's plain mean")
    hyper_f32(cfg.server_lr, cfg.server_betas, cfg.server_tau)
    return kind


def make_server_optimizer(model, cfg, log=None) -> Optional[ServerOptimizer]:
    """The configuration's server optimizer (``--server-opt adam --server-lr 1e-2``), or None for
    plain FedAvg (``server_opt="fedavg"``: today's ``scale_cast`` path, untouched)."""
    kind = check_server_config(cfg)
    if kind is None:
        return None
    server = ServerOptimizer(model, kind, lr=cfg.server_lr, betas=cfg.server_betas, tau=cfg.server_tau)
    if server.adaptive and server.lr >= 1.0 and log is not None:
        log.info(f"[WARN] server_opt={kind} with server_lr={server.lr:g}: the adaptive server optimizers move every "
                 f"weight by about server_lr per round; try --server-lr 1e-2")
    return server
