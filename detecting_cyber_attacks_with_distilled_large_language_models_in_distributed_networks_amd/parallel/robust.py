"""Byzantine-robust aggregation: coordinate-wise trimmed mean and median.

Yin et al., "Byzantine-Robust Distributed Learning: Towards Optimal Statistical Rates" (ICML 2018).
The plain mean lets one faulty or hostile client own the global model (one NaN client makes every
weight NaN; one client sending ``-4 w`` cancels four honest ones).
Here, per coordinate, the ``k`` lowest and ``k`` highest of the ``M`` participating clients' values
are dropped and the rest averaged -- any ``k`` liars per coordinate cannot move the result outside
the honest clients' range.

Specification (``torch_robust_`` is it, literally; the HIP kernel equals it bit for bit).  Inputs:
``M >= 1`` flat fp32 vectors of equal length ``n`` and a trim count ``0 <= 2k < M``.

* Total order: the key of a float with bits ``b`` (int32) is ``b ^ ((b >> 31) & 0x7fffffff)``,
  compared as a signed int: ``-NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN``.  Ties are broken by
  the client's slot index, so the order is total for any input whatever.
* Per coordinate: sort the M (key, slot) pairs ascending, drop the k lowest and the k highest, sum
  the remaining ``M - 2k`` values in ascending order in fp32 (``acc = s[k]; acc = acc + s[k+1]; ...``,
  every addition rounded on its own), ``out = acc * float32(1 / (M - 2k))``.
* ``k = 0`` is the mean summed in sorted order; ``k = (M - 1) // 2`` the median (odd M: the middle
  value times 1; even M: ``(a + b) * 0.5``).
* ``trimmed[j]`` (int64): at how many coordinates slot j's value was dropped.  ``nonfinite``: how
  many outputs are not finite.  For honest i.i.d. clients each slot's trimmed share is about
  ``2k / M``; a poisoner's approaches 1 -- the report is an attack detector of its own.

On the GPU the whole aggregate is ONE launch (``ops.kernels.robust_agg``, csrc/kernels/robust_agg.hip)
that reads the M arenas once and writes the new master, the bf16 shadow and the counts; on the CPU it
is ``torch_robust_`` itself.  An alignment pad (every client ``+0``) stays ``+0``.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import torch

AGGREGATORS = ("mean", "trimmed_mean", "median", "multi_krum", "geometric_median")
DIST_AGGREGATORS = ("multi_krum", "geometric_median")  # judged by L2 distance: parallel/robust_dist.py
MAX_GPU_CLIENTS = 16  # the kernel's instantiations: 2 <= M <= 16
_CHUNK = 1 << 22      # coordinates per pass of the reference (bounds its int64 temporaries)


def f32(value: float) -> float:
    """``value`` rounded to fp32, as a Python float."""
    return float(torch.tensor(float(value), dtype=torch.float32).item())


@torch.no_grad()
def torch_robust_(states: Sequence[torch.Tensor], k: int) -> Tuple[torch.Tensor, torch.Tensor, int]:
    """The specification as torch ops, on the states' device: ``(out, trimmed, nonfinite)`` -- the
    fp32 aggregate, the int64 per-slot trimmed counts and the number of non-finite outputs."""
    M = len(states)
    k = int(k)
    if M < 1 or M > 32:
        raise ValueError(f"robust aggregation takes 1 .. 32 clients, got {M}")
    if not 0 <= 2 * k < M:
        raise ValueError(f"trim count k = {k} needs 0 <= 2k < M = {M}")
    n = states[0].numel()
    dev = states[0].device
    for s in states:
        if s.dtype != torch.float32 or s.dim() != 1 or s.numel() != n or s.device != dev:
            raise ValueError("robust aggregation takes flat fp32 tensors of one length on one device")
    inv = f32(1.0 / (M - 2 * k))
    out = torch.empty(n, dtype=torch.float32, device=dev)
    trimmed = torch.zeros(M, dtype=torch.int64, device=dev)
    slot_col = torch.arange(M, dtype=torch.int64, device=dev).unsqueeze(1)
    for a in range(0, n, _CHUNK):
        b = min(n, a + _CHUNK)
        X = torch.stack([s[a:b] for s in states])                       # [M, c]
        bits = X.view(torch.int32).to(torch.int64)
        key = bits ^ ((bits >> 31) & 0x7FFFFFFF)
        comp = (key << 5) | slot_col
        order = torch.sort(comp, dim=0).values
        slot = order & 31
        srt = torch.gather(X, 0, slot)                                   # the values, ascending
        acc = srt[k].clone()
        for j in range(k + 1, M - k):
            acc = acc + srt[j]
        out[a:b] = acc * inv
        if k:
            cut = torch.cat([slot[:k], slot[M - k:]]).reshape(-1)
            trimmed += torch.bincount(cut, minlength=M)
    nonfinite = int((~torch.isfinite(out)).sum())
    return out, trimmed, nonfinite


def trim_count(M: int, aggregator: str, trim_ratio: float = 0.2) -> int:
    """The k of ``M`` participating clients: "median" -> (M - 1) // 2, "trimmed_mean" ->
    floor(trim_ratio * M) (a ValueError when that leaves nothing: 2k >= M), "mean" -> 0."""
    M = int(M)
    if M < 1:
        raise ValueError(f"robust aggregation of {M} clients")
    if aggregator == "median":
        return (M - 1) // 2
    if aggregator == "mean":
        return 0
    if aggregator in DIST_AGGREGATORS:
        raise ValueError(f"aggregator {aggregator!r} has no trim count: it judges whole updates by their distance")
    if aggregator != "trimmed_mean":
        raise ValueError(f"aggregator must be one of {', '.join(AGGREGATORS)}; got {aggregator!r}{_krum_hint(aggregator)}")
    r = _check_ratio(trim_ratio)
    k = int(math.floor(r * M))
    if 2 * k >= M:
        raise ValueError(f"trim_ratio={r!r} trims {k} of {M} clients at each end and leaves none")
    return k


def _krum_hint(aggregator) -> str:
    return " (Krum proper is aggregator='multi_krum' with krum_select=1)" if str(aggregator).lower() == "krum" else ""


def _check_ratio(trim_ratio) -> float:
    try:
        r = float(trim_ratio)
    except (TypeError, ValueError):
        raise ValueError(f"trim_ratio must be a number in [0, 0.5), got {trim_ratio!r}") from None
    if not (math.isfinite(r) and 0.0 <= r < 0.5):
        raise ValueError(f"trim_ratio must lie in [0, 0.5), got {trim_ratio!r}")
    return r


@dataclass
class RobustAggregator:
    """What ``fedavg_(..., robust=)`` takes: the aggregator ("trimmed_mean" | "median" | "multi_krum" |
    "geometric_median"), its parameters, and how many consecutive ranks make one client.  ``last`` is the
    latest round's report (``robust_aggregate_``'s or ``robust_dist_aggregate_``'s dict), as
    ``ServerOptimizer.last`` holds its norms."""
    aggregator: str
    trim_ratio: float = 0.2
    gpus_per_client: int = 1
    last: Optional[Dict] = None
    byzantine: Optional[int] = None    # multi_krum: f (None: the most Krum tolerates for the round's M)
    krum_select: Optional[int] = None  # multi_krum: m (None: M - f)
    geomed_iters: int = 6
    geomed_nu: float = 1e-6

    def k(self, M: int) -> int:
        return trim_count(M, self.aggregator, self.trim_ratio)

    def aggregate_(self, model, states: Sequence[torch.Tensor], server=None) -> Dict:
        """The round's aggregate of ``states`` into the model (and the server step, if any): the
        coordinate-wise kinds through ``robust_aggregate_`` with this round's ``k``, the distance-based
        ones through ``robust_dist_aggregate_``.  Returns the round's report."""
        if self.aggregator in DIST_AGGREGATORS:
            from .robust_dist import robust_dist_aggregate_
            return robust_dist_aggregate_(model, states, self.aggregator, server, self.byzantine, self.krum_select,
                                          self.geomed_iters, self.geomed_nu)
        return robust_aggregate_(model, states, self.k(len(states)), server)


def check_robust_config(cfg) -> Optional[str]:
    """The configuration's robust aggregator (None for the plain mean), or a ValueError for an
    unknown aggregator, a bad ``trim_ratio``, or a setting it does not run with.  Needs no model:
    callers refuse a bad configuration before any work."""
    agg = str(getattr(cfg, "aggregator", "mean")).lower()
    if agg not in AGGREGATORS:
        raise ValueError(f"aggregator must be one of {', '.join(AGGREGATORS)}; got {cfg.aggregator!r}{_krum_hint(agg)}")
    if agg == "mean":
        return None
    if agg == "trimmed_mean":
        _check_ratio(cfg.trim_ratio)
    if agg in DIST_AGGREGATORS:
        _check_dist_fields(cfg)
    if getattr(cfg, "transport", "collective") == "tcp":
        raise ValueError(f"aggregator={agg!r} needs transport='collective': the reference-compatible TCP server "
                         f"keeps the reference's plain mean")
    if getattr(cfg, "weighted_fedavg", False):
        raise ValueError(f"aggregator={agg!r} does not take weighted_fedavg=True: order statistics are unweighted")
    return agg


def _check_dist_fields(cfg) -> None:
    f, m = getattr(cfg, "byzantine", None), getattr(cfg, "krum_select", None)
    if f is not None and int(f) < 0:
        raise ValueError(f"byzantine must be >= 0, got {f!r}")
    if m is not None and int(m) < 1:
        raise ValueError(f"krum_select must be >= 1, got {m!r}")
    if int(getattr(cfg, "geomed_iters", 6)) < 1:
        raise ValueError(f"geomed_iters must be >= 1, got {cfg.geomed_iters!r}")
    try:
        nu = float(getattr(cfg, "geomed_nu", 1e-6))
    except (TypeError, ValueError):
        raise ValueError(f"geomed_nu must be a positive finite number, got {cfg.geomed_nu!r}") from None
    if not (math.isfinite(nu) and nu > 0.0):
        raise ValueError(f"geomed_nu must be positive and finite, got {cfg.geomed_nu!r}")


def make_robust(cfg, gpus_per_client: int = 1) -> Optional[RobustAggregator]:
    """The configuration's ``RobustAggregator`` (``--aggregator median``), or None for the plain mean
    (``aggregator="mean"``: today's path, untouched)."""
    agg = check_robust_config(cfg)
    if agg is None:
        return None
    f, m = getattr(cfg, "byzantine", None), getattr(cfg, "krum_select", None)
    return RobustAggregator(agg, float(cfg.trim_ratio), int(gpus_per_client),
                            byzantine=None if f is None else int(f), krum_select=None if m is None else int(m),
                            geomed_iters=int(getattr(cfg, "geomed_iters", 6)),
                            geomed_nu=float(getattr(cfg, "geomed_nu", 1e-6)))


def _report(trimmed: List[int], nonfinite: int, k: int, n: int) -> Dict:
    return {"trimmed": [int(t) for t in trimmed], "trimmed_share": [int(t) / float(n) for t in trimmed],
            "nonfinite": int(nonfinite), "k": int(k), "clients": len(trimmed)}


def most_trimmed(report: Dict) -> Tuple[int, float]:
    """(slot, share) of the slot trimmed most often (the lowest slot among equals)."""
    shares = report["trimmed_share"]
    j = max(range(len(shares)), key=lambda i: (shares[i], -i))
    return j, shares[j]


@torch.no_grad()
def robust_aggregate_(model, states: Sequence[torch.Tensor], k: int, server=None) -> Dict:
    """The robust aggregate of the participating clients' masters ``states`` (flat fp32 tensors like
    ``model.arena.master``, none of them the master itself) becomes the model's master and bf16
    shadow.  On the GPU: one ``robust_agg`` launch (2 <= M <= 16; one client is a copy).  With a
    server optimizer the aggregate is the ``avg`` of its pseudo-gradient: it is placed in the master
    and ``server.apply_(model, 1.0)`` makes the step (``inv = 1``, so ``avg = s * 1`` exactly) and
    writes the shadow.

    Returns ``{"trimmed": [M ints], "trimmed_share": [...], "nonfinite": int, "k": k, "clients": M}``
    (``trimmed_share`` divides by n, alignment pads included).  Raises a RuntimeError naming the
    most-trimmed slots when any output is not finite -- more liars than ``k`` covers: a model of
    NaNs is never adopted silently (no server step is made with it)."""
    A = model.arena
    M, k = len(states), int(k)
    n = A.master.numel()
    if M < 1:
        raise ValueError("robust aggregation with no participating clients")
    if not 0 <= 2 * k < M:
        raise ValueError(f"trim count k = {k} needs 0 <= 2k < M = {M}")
    if A.master.is_cuda:
        from ..ops import kernels as K
        shadow = A.shadow if server is None else None  # (the server step writes the shadow)
        if M == 1:
            A.master.copy_(states[0])
            if shadow is not None:
                K.scale_cast(A.master, shadow, 1.0)
            trimmed, nonfinite = [0], int((~torch.isfinite(A.master)).sum())
        else:
            if M > MAX_GPU_CLIENTS:
                raise ValueError(f"the robust aggregation kernel takes at most {MAX_GPU_CLIENTS} clients, got {M}")
            counts = torch.empty(K.ROBUST_AGG_COLS * K.robust_agg_grid(n), dtype=torch.int32, device=A.master.device)
            K.robust_agg(list(states), k, A.master, shadow, counts)
            sums = counts.view(-1, K.ROBUST_AGG_COLS).sum(dim=0, dtype=torch.int64).tolist()
            trimmed, nonfinite = sums[:M], sums[K.ROBUST_AGG_COLS - 1]
        if server is None:
            model.mark_shadow_synced()
    else:
        out, t, nonfinite = torch_robust_(list(states), k)
        A.master.copy_(out)
        trimmed = t.tolist()
        if server is None:
            model.sync_shadow(force=True)
    rep = _report(trimmed, nonfinite, k, n)
    if nonfinite > 0:
        order = sorted(range(M), key=lambda i: (-rep["trimmed_share"][i], i))[:max(1, min(M, k + 1))]
        named = ", ".join(f"slot {i} ({rep['trimmed_share'][i]:.3f})" for i in order)
        raise RuntimeError(f"robust aggregation (k = {k} of {M} clients) left {nonfinite} non-finite weights: more "
                           f"faulty clients than k covers; most trimmed: {named}")
    if server is not None:
        server.apply_(model, 1.0)
    return rep
