"""Distance-based Byzantine-robust aggregation: multi-Krum and the geometric median.

The coordinate-wise rules of ``parallel/robust.py`` judge every weight on its own; a client that stays
inside the honest range on every coordinate while being far away as a vector passes them.  The rules
here judge a client's whole update by its L2 distance to the others:

* **multi-Krum** (Blanchard et al., "Machine Learning with Adversaries: Byzantine Tolerant Gradient
  Descent", NeurIPS 2017): a client's score is the sum of its squared distances to its ``M - f - 2``
  nearest neighbours; the ``m`` clients with the lowest scores are averaged, the others are rejected by
  name.  ``m = 1`` is Krum proper.  Its guarantee needs ``M >= 2f + 3``.
* **geometric median** by smoothed Weiszfeld iterations (RFA: Pillutla, Kakade, Harchaoui, "Robust
  Aggregation for Federated Learning", IEEE TSP 2022): the point minimising the sum of the distances to
  the clients -- breakdown point 1/2, rotation invariant; every client gets a weight.

Specification.  Inputs: ``M`` flat fp32 vectors of equal length ``n`` in slot order (the participating
clients in client order).  Every operation is rounded on its own (no FMA contraction).

a. ``torch_pair_sqdist``: ``D[i][j] = sum_e (x_i[e] - x_j[e])^2``, the difference first, then the
   square -- never ``G_ii + G_jj - 2 G_ij``: client masters differ by about 1e-3 of their norm and fp32
   partial sums would cancel that away.  The function evaluates it in fp64 from the fp32 inputs: the
   oracle of the kernel, whose lanes add fp32 squares of fp32 differences.
b. ``krum_select(D, f, m)``, pure fp64 on the host and the exact mirror of the device finalizer:
   non-finite entries of ``D`` count as ``+inf``; ``c = max(1, M - f - 2)``; ``score_i`` = the ``c``
   smallest ``D[i][j]``, ``j != i``, added in ascending order; the ``m`` slots with the smallest
   ``(score, slot)`` and a finite score are selected, ``weights[i] = float32(1 / m)`` for them and
   ``+0`` for the others; fewer than ``m`` finite scores: ``flag = 1`` and every weight 0.
c. ``geomed_weights(Dz, nu)``, likewise: ``w_i = 1 / max(nu, sqrt(Dz_i))`` in fp64, 0 for a non-finite
   ``Dz_i``; ``beta_i = float32(w_i / sum(w))``, the sum in slot order; ``objective`` = the sum of
   ``sqrt(Dz_i)`` over the finite slots; ``sum(w) == 0``: ``flag = 1``.
d. ``torch_weighted_mean_(states, weights)``: ``acc = w_a * x_a`` for the first slot with ``w != 0``,
   then ``acc = acc + w_b * x_b`` for each later slot with ``w != 0``, in slot order, in fp32.  A slot
   with weight 0 is skipped, not multiplied: a rejected client's NaN does not reach the result.  No
   non-zero weight gives ``+0``.  Also ``Dz[i] = sum_e (x_i[e] - out[e])^2`` for every slot (the fp32
   difference against the rounded ``out``, squared in fp32 -- a client at 3e30 overflows to ``inf`` and
   is given weight 0 -- and added in fp64), and the count of non-finite outputs.
e. ``torch_multi_krum_`` = a, b, d.
f. ``torch_geometric_median_``: pass 0 is d with every weight zero and no output (the centre is 0, so
   ``Dz[i] = |x_i|^2`` and the first weights are roughly uniform over the clients with a finite norm);
   then c, d ``iters`` times.  A NaN, inf or overflowing client gets weight 0 at pass 0 and keeps it,
   so a failure (``flag = 1``) can only arise at pass 0, before any output was written.

An alignment pad (every client ``+0``) stays ``+0`` under both.

On the GPU (csrc/kernels/robust_dist.hip through ``ops.kernels``) the aggregate is a fixed sequence of
launches -- ``robust_pairdist``, ``robust_krum_finalize``, ``robust_wmean`` for multi-Krum;
``robust_wmean`` and ``robust_geomed_finalize`` alternating for the geometric median -- with the weights
handed from launch to launch in device memory and one host read at the end.  The fused pair sums are
fp32 per lane, so a near-tie between two scores may fall the other way than under the fp64 oracle;
each stage is exact given its input (tests/test_robust_dist_gpu.py).
"""
from __future__ import annotations

import math
from typing import Dict, List, Sequence, Tuple

import torch

from .robust import DIST_AGGREGATORS, MAX_GPU_CLIENTS, f32  # noqa: F401  (DIST_AGGREGATORS: re-exported)

MAX_CLIENTS = 32  # the torch specification's bound, that of ``robust.torch_robust_`` (the kernels stop at 16)
_CHUNK = 1 << 22  # coordinates per pass of the reference (bounds its temporaries)


def _check_states(states: Sequence[torch.Tensor], lo: int = 1) -> Tuple[int, int]:
    M = len(states)
    if M < lo or M > MAX_CLIENTS:
        raise ValueError(f"distance-based aggregation takes {lo} .. {MAX_CLIENTS} clients, got {M}")
    n, dev = states[0].numel(), states[0].device
    for s in states:
        if s.dtype != torch.float32 or s.dim() != 1 or s.numel() != n or s.device != dev:
            raise ValueError("distance-based aggregation takes flat fp32 tensors of one length on one device")
    return M, n


@torch.no_grad()
def torch_pair_sqdist(states: Sequence[torch.Tensor]) -> torch.Tensor:
    """The float64 ``[M, M]`` matrix of squared distances, evaluated in fp64 from the fp32 inputs."""
    M, n = _check_states(states)
    D = torch.zeros((M, M), dtype=torch.float64, device=states[0].device)
    for a in range(0, n, _CHUNK):
        X = torch.stack([s[a:a + _CHUNK] for s in states]).double()
        for i in range(M):
            d = X[i + 1:] - X[i]
            D[i, i + 1:] += (d * d).sum(dim=1)
    return D + D.t()


def default_byzantine(M: int) -> int:
    """The most liars Krum tolerates among ``M`` clients: ``(M - 3) // 2``, 0 below 3."""
    return max(0, (int(M) - 3) // 2)


def krum_params(M: int, byzantine=None, krum_select=None) -> Tuple[int, int]:
    """``(f, m)`` for a round of ``M`` live clients.  Unset ``byzantine``: ``default_byzantine(M)``; unset
    ``krum_select``: ``M - f``.  An explicit ``f`` with ``M < 2f + 3``, or ``m > M - f``, is a ValueError
    naming the flag."""
    M = int(M)
    if byzantine is None:
        f = default_byzantine(M)
    else:
        f = int(byzantine)
        if f < 0:
            raise ValueError(f"byzantine must be >= 0, got {byzantine!r}")
        if f > 0 and M < 2 * f + 3:
            raise ValueError(f"byzantine={f} needs at least 2f + 3 = {2 * f + 3} participating clients, got {M}")
    if krum_select is None:
        m = M - f
    else:
        m = int(krum_select)
        if m < 1:
            raise ValueError(f"krum_select must be >= 1, got {krum_select!r}")
        if m > M - f:
            raise ValueError(f"krum_select={m} exceeds the M - f = {M} - {f} = {M - f} clients that can be honest")
    return f, m


def krum_select(D, f: int, m: int) -> Tuple[List[float], List[int], List[float], int]:
    """``(scores, selected, weights, flag)`` of the ``[M, M]`` squared distances ``D`` (step b of the
    specification; plain Python floats, which are fp64).  ``selected`` is ascending; with ``flag = 1`` it
    is empty and every weight is 0."""
    rows = D.tolist() if hasattr(D, "tolist") else [list(r) for r in D]
    M, f, m = len(rows), int(f), int(m)
    if M < 2 or f < 0 or not 1 <= m <= M:
        raise ValueError(f"krum_select needs M >= 2, f >= 0 and 1 <= m <= M; got M = {M}, f = {f}, m = {m}")
    c = max(1, M - f - 2)
    scores = []
    for i in range(M):
        near = sorted(float(v) if math.isfinite(v) else math.inf for j, v in enumerate(rows[i]) if j != i)
        acc = 0.0
        for v in near[:c]:
            acc = acc + v
        scores.append(acc)
    finite = [i for i in range(M) if math.isfinite(scores[i])]
    if len(finite) < m:
        return scores, [], [0.0] * M, 1
    selected = sorted(sorted(finite, key=lambda i: (scores[i], i))[:m])
    w = f32(1.0 / m)
    return scores, selected, [w if i in selected else 0.0 for i in range(M)], 0


def geomed_weights(Dz, nu: float) -> Tuple[List[float], float, int, List[float]]:
    """``(beta, objective, flag, beta64)`` of the squared distances ``Dz`` to the current centre (step c):
    ``beta`` rounded to fp32, ``beta64`` the fp64 quotients before that rounding."""
    dz = [float(v) for v in (Dz.tolist() if hasattr(Dz, "tolist") else Dz)]
    nu = float(nu)
    if not (math.isfinite(nu) and nu > 0.0):
        raise ValueError(f"geomed_nu must be positive and finite, got {nu!r}")
    w, total, objective = [], 0.0, 0.0
    for d in dz:
        wi = 0.0
        if math.isfinite(d):
            r = math.sqrt(d)
            objective = objective + r
            wi = 1.0 / max(nu, r)
        total = total + wi
        w.append(wi)
    if total == 0.0:
        return [0.0] * len(dz), objective, 1, [0.0] * len(dz)
    beta64 = [wi / total for wi in w]
    return [f32(b) for b in beta64], objective, 0, beta64


@torch.no_grad()
def torch_weighted_mean_(states: Sequence[torch.Tensor], weights) -> Tuple[torch.Tensor, torch.Tensor, int]:
    """Step d as torch ops on the states' device: ``(out, Dz, nonfinite)`` -- the fp32 weighted sum over
    the slots with a non-zero weight, every slot's float64 squared distance to it, and the number of
    non-finite outputs."""
    M, n = _check_states(states)
    w = [f32(v) for v in (weights.tolist() if hasattr(weights, "tolist") else weights)]
    if len(w) != M:
        raise ValueError(f"{len(w)} weights for {M} clients")
    out = torch.zeros(n, dtype=torch.float32, device=states[0].device)
    first = True
    for x, wi in zip(states, w):
        if wi == 0.0:
            continue
        t = x * wi
        out = t if first else out + t
        first = False
    Dz = torch.zeros(M, dtype=torch.float64, device=out.device)
    for a in range(0, n, _CHUNK):
        for i, x in enumerate(states):
            d = x[a:a + _CHUNK] - out[a:a + _CHUNK]
            Dz[i] += (d * d).double().sum()
    return out, Dz, int((~torch.isfinite(out)).sum())


@torch.no_grad()
def torch_multi_krum_(states: Sequence[torch.Tensor], f: int, m: int) -> Dict:
    """Steps a, b, d: ``{"out", "D", "scores", "selected", "weights", "flag", "nonfinite"}``; with
    ``flag = 1`` ``out`` is None."""
    D = torch_pair_sqdist(states)
    scores, selected, weights, flag = krum_select(D, f, m)
    res = {"out": None, "D": D, "scores": scores, "selected": selected, "weights": weights, "flag": flag,
           "nonfinite": 0}
    if not flag:
        res["out"], _, res["nonfinite"] = torch_weighted_mean_(states, weights)
    return res


@torch.no_grad()
def torch_geometric_median_(states: Sequence[torch.Tensor], iters: int = 6, nu: float = 1e-6) -> Dict:
    """Step f: ``{"out", "weights", "Dz", "objective", "flag", "nonfinite"}`` -- the aggregate, the weights
    of the last pass, the squared distances to it, and the objective after each pass (``iters + 1`` values,
    pass 0 included).  With ``flag = 1`` ``out`` is None and ``Dz`` holds the squared norms."""
    M, _ = _check_states(states)
    iters = int(iters)
    if iters < 1:
        raise ValueError(f"geomed_iters must be >= 1, got {iters}")
    _, Dz, _ = torch_weighted_mean_(states, [0.0] * M)
    res = {"out": None, "weights": [0.0] * M, "Dz": Dz.tolist(), "objective": [], "flag": 0, "nonfinite": 0}
    for _ in range(iters):
        beta, objective, flag, _ = geomed_weights(Dz, nu)
        res["objective"].append(objective)
        if flag:
            res["flag"] = 1
            return res
        out, Dz, nonfinite = torch_weighted_mean_(states, beta)
        res.update(out=out, weights=beta, Dz=Dz.tolist(), nonfinite=nonfinite)
    res["objective"].append(geomed_weights(Dz, nu)[1])
    return res


def _bad_slots(values) -> str:
    bad = [i for i, v in enumerate(values) if not math.isfinite(v)]
    return ", ".join(f"slot {i}" for i in bad) if bad else "none"


def _krum_report(M, f, m, D, scores, selected) -> Dict:
    dist = [[math.sqrt(v) if v >= 0.0 else float("nan") for v in row] for row in D]
    return {"kind": "multi_krum", "clients": M, "f": int(f), "m": int(m), "scores": [float(s) for s in scores],
            "selected": list(selected), "rejected": [i for i in range(M) if i not in selected], "distances": dist}


def _geomed_report(M, iters, nu, weights, Dz, objective) -> Dict:
    return {"kind": "geometric_median", "clients": M, "iters": int(iters), "nu": float(nu),
            "weights": [float(w) for w in weights],
            "distances": [math.sqrt(v) if v >= 0.0 else float("nan") for v in Dz],
            "objective": [float(o) for o in objective]}


def _one_client_report(kind: str, iters: int, nu: float) -> Dict:
    if kind == "multi_krum":
        return _krum_report(1, 0, 1, [[0.0]], [0.0], [0])
    return _geomed_report(1, iters, nu, [1.0], [0.0], [])


@torch.no_grad()
def robust_dist_aggregate_(model, states: Sequence[torch.Tensor], kind: str, server=None, byzantine=None,
                           krum_select_m=None, iters: int = 6, nu: float = 1e-6) -> Dict:
    """The multi-Krum / geometric-median aggregate of the participating clients' masters ``states`` (flat
    fp32 tensors like ``model.arena.master``, none of them the master itself) becomes the model's master
    and bf16 shadow.  On the GPU: a fixed sequence of launches into the master, the shadow written by the
    last pass (2 <= M <= 16; one client is a copy), one host read at the end.  With a server optimizer the
    aggregate is the ``avg`` of its pseudo-gradient, as in ``robust_aggregate_``.

    Returns the round's report (``kind`` "multi_krum": ``clients, f, m, scores, selected, rejected,
    distances``; "geometric_median": ``clients, iters, nu, weights, distances, objective``).  A NaN or
    overflowing client has an ``inf`` score and ``nan`` / ``inf`` distances in it: the round records and
    ``federated_report.json`` then hold ``Infinity`` / ``NaN``, which Python's ``json`` writes and reads
    back and a strict JSON parser refuses.  Raises a
    RuntimeError naming the slots with non-finite scores / distances when the rule finds too few usable
    clients (``flag = 1``: the master is left exactly as it was) or an output is not finite; no server
    step is made then."""
    if kind not in DIST_AGGREGATORS:
        raise ValueError(f"aggregator must be one of {', '.join(DIST_AGGREGATORS)}; got {kind!r}")
    A = model.arena
    M = len(states)
    if M < 1:
        raise ValueError("robust aggregation with no participating clients")
    iters, nu = int(iters), float(nu)
    if kind == "multi_krum":
        f, m = krum_params(M, byzantine, krum_select_m)
    cuda = A.master.is_cuda
    if cuda and M > MAX_GPU_CLIENTS:
        raise ValueError(f"the robust aggregation kernels take at most {MAX_GPU_CLIENTS} clients, got {M}")
    shadow = A.shadow if (cuda and server is None) else None  # (the server step writes the shadow)
    if M == 1:
        A.master.copy_(states[0])
        if cuda and shadow is not None:
            from ..ops import kernels as K
            K.scale_cast(A.master, shadow, 1.0)
        flag, nonfinite = 0, int((~torch.isfinite(A.master)).sum())
        rep, culprits = _one_client_report(kind, iters, nu), "slot 0"
    elif cuda:
        flag, nonfinite, rep, culprits = _gpu_aggregate_(A.master, shadow, list(states), kind, iters, nu,
                                                         *((f, m) if kind == "multi_krum" else (0, 0)))
    elif kind == "multi_krum":
        r = torch_multi_krum_(list(states), f, m)
        flag, nonfinite = r["flag"], r["nonfinite"]
        rep, culprits = _krum_report(M, f, m, r["D"].tolist(), r["scores"], r["selected"]), _bad_slots(r["scores"])
        if not flag:
            A.master.copy_(r["out"])
    else:
        r = torch_geometric_median_(list(states), iters, nu)
        flag, nonfinite = r["flag"], r["nonfinite"]
        rep, culprits = _geomed_report(M, iters, nu, r["weights"], r["Dz"], r["objective"]), _bad_slots(r["Dz"])
        if not flag:
            A.master.copy_(r["out"])
    if flag:
        raise RuntimeError(f"{kind} of {M} clients found too few usable clients and left the model as it was: "
                           f"non-finite scores / distances at {culprits}")
    if server is None:
        if cuda:
            model.mark_shadow_synced()
        else:
            model.sync_shadow(force=True)
    if nonfinite > 0:
        raise RuntimeError(f"{kind} of {M} clients left {nonfinite} non-finite weights; non-finite scores / "
                           f"distances at {culprits}")
    if server is not None:
        server.apply_(model, 1.0)
    return rep


def _gpu_aggregate_(master, shadow, states, kind, iters, nu, f, m):
    """The launch sequence; ``(flag, nonfinite, report, culprits)`` from one host read."""
    from ..ops import kernels as K
    M, n, dev = len(states), master.numel(), master.device
    grid = K.robust_dist_grid(n)
    ctl = torch.empty(K.ROBUST_DIST_CTL, dtype=torch.float32, device=dev)
    wpart = torch.empty((M + 1) * grid, dtype=torch.float64, device=dev)
    if kind == "multi_krum":
        ppart = torch.empty(M * (M - 1) // 2 * grid, dtype=torch.float64, device=dev)
        stats = torch.empty(K.ROBUST_KRUM_STATS, dtype=torch.float64, device=dev)
        K.robust_pairdist(states, ppart)
        K.robust_krum_finalize(ppart, grid, M, f, m, ctl, stats)
        wpart.zero_()  # (a refused launch writes nothing: the count read below is then 0)
        K.robust_wmean(states, ctl, master, shadow, wpart)
        host = torch.cat([ctl.double(), stats, wpart.view(grid, M + 1)[:, M].sum().reshape(1)]).tolist()
        flag, st, nonfinite = int(host[16]), host[K.ROBUST_DIST_CTL:-1], int(host[-1])
        D = [st[16 * i:16 * i + M] for i in range(M)]
        scores = st[256:256 + M]
        selected = [i for i in range(M) if st[272 + i] != 0.0]
        return flag, nonfinite, _krum_report(M, f, m, D, scores, selected), _bad_slots(scores)
    R = K.ROBUST_GEOMED_ROW
    stats = torch.zeros((iters + 1) * R, dtype=torch.float64, device=dev)
    ctl.zero_()  # pass 0: every weight zero, the centre is 0
    for it in range(iters + 1):
        last = it == iters
        K.robust_wmean(states, ctl, master if last else None, shadow if last else None, wpart)
        K.robust_geomed_finalize(wpart, grid, M, nu, it, ctl, stats)
    host = torch.cat([ctl.double(), stats]).tolist()
    rows = [host[K.ROBUST_DIST_CTL + R * it:K.ROBUST_DIST_CTL + R * (it + 1)] for it in range(iters + 1)]
    flag = int(host[16])
    weights = [f32(b) for b in rows[iters - 1][18:18 + M]]  # the weights the last pass used
    Dz = rows[0 if flag else iters][2:2 + M]
    rep = _geomed_report(M, iters, nu, weights, Dz, [r[0] for r in rows[:1 if flag else iters + 1]])
    return flag, 0 if flag else int(rows[iters][1]), rep, _bad_slots(Dz)
