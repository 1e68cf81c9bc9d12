"""Federated averaging.

Reference (server.py:67-79): gather exactly NUM_CLIENTS pickled state_dicts,
``base[key] += m_i[key]; base[key] /= N`` (unweighted, in place on client 0's
dict), then broadcast the mean back (server.py:81-114) -- ~20 s of gzip + TCP
per round for 265 MB.

Here: every client's fp32 master weights already sit in one flat arena, so a
round is ONE collective (``all_reduce(SUM)`` over 66.4 M floats on RCCL/xGMI)
followed by one fused HIP pass that applies the 1/N (or 1/sum-of-weights)
scale and re-casts the bf16 compute shadow.  Options the reference lacks:
sample-count weighting (pre-scale by n_k) and partial participation (a
non-participating / dropped client contributes weight 0 and receives the
average of the live clients), and FedOpt server optimizers (``fedavg_(..., server=)``,
parallel/server_opt.py: the same all-reduce, then one fused server step on the sum instead of the
scale), and Byzantine-robust aggregation (``fedavg_(..., robust=)``, parallel/robust.py: an
all-gather instead of the sum, then one fused pass that takes the coordinate-wise trimmed mean or
median of the participating clients), and secure aggregation (``fedavg_(..., secagg=)``,
parallel/secagg.py: the clients' fixed-point updates are all-gathered under pairwise ChaCha masks that
cancel in their modular sum, and one fused pass unmasks the mean).

``aggregate_state_dicts`` keeps the reference's server-side API for
state_dict lists (floating tensors only -- an int64 buffer would make the
reference's in-place ``/=`` raise).
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Dict, List, Optional, Sequence

import torch
import torch.distributed as dist

from .comm import info


def _dist_on() -> bool:
    return dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1


@torch.no_grad()
def broadcast_model(model, src: int = 0, comm=None):
    """Make every client start from rank ``src``'s weights (identical init).

    comm: optional ``parallel.rccl.NativeComm`` (framework-owned RCCL communicator)."""
    if _dist_on():
        if comm is not None:
            comm.broadcast_(model.arena.master, root=src)
        else:
            dist.broadcast(model.arena.master, src=src)
    model.sync_shadow(force=True)


@torch.no_grad()
def fedavg_(model, weight: float = 1.0, participate: bool = True, comm=None, server=None, robust=None,
            compress=None, anchor=None, client: int = 0, round: int = 0, secagg=None) -> float:
    """In-place FedAvg of ``model`` across all ranks; returns the total weight.

    weight:      this client's aggregation weight (1 = unweighted, n_k = sample-weighted)
    participate: False -> this client's update is dropped this round (fault injection /
                 partial participation); it still receives the aggregate.
    comm:        optional ``parallel.rccl.NativeComm``; default is the torch.distributed group.
    server:      optional ``parallel.server_opt.ServerOptimizer``: the pre-scale and the all-reduce are
                 the same, and its step on the weighted sum replaces the final 1/W scale (every rank
                 holds the same server state, so the ranks stay identical; a client that does not
                 participate still makes the step).  Its norms are left in ``server.last``.
    robust:      optional ``parallel.robust.RobustAggregator`` (trimmed mean / median): the masters are
                 all-gathered instead of summed and one fused pass takes the coordinate-wise robust
                 aggregate of the participating clients' rows (``_robust_``); unweighted, so ``weight``
                 is not used and the number of participating clients is returned.  Its report is left
                 in ``robust.last``.  None: the code below, untouched.
    compress:    optional ``parallel.compress.Compressor`` (int8 / int4 codes, or top-k entries; error feedback): every
                 participating client encodes ``master - anchor`` (``anchor``: the round's starting
                 weights, a buffer apart from the master; ``client`` / ``round`` select its residual and
                 its stochastic stream), the payloads are all-gathered and their decoded mean is added
                 to the anchor (``_compressed_``); unweighted, so ``weight`` is not used and the number
                 of participating clients is returned.  Its report is left in ``compress.last``.  None:
                 the code below, untouched.
    secagg:      optional ``parallel.secagg.SecureAggregator``: every participating client sends the
                 fixed-point codes of ``master - anchor`` under the ChaCha streams it shares with the
                 round's other live clients (``client`` is its index, ``round`` goes into the nonce), the
                 payloads are all-gathered, and the mean of their modular sum -- in which the streams
                 cancel -- is added to the anchor (``_secagg_``); unweighted, so ``weight`` is not used and
                 the number of participating clients is returned.  Its report is left in ``secagg.last``.
                 None: the code below, untouched.
    """
    if secagg is not None:
        if robust is not None or compress is not None:
            raise ValueError("secure aggregation takes the plain mean of uncompressed updates (robust=None, "
                             "compress=None)")
        if anchor is None:
            raise ValueError("secure aggregation needs the round's starting weights (anchor=)")
        return _secagg_(model, participate, comm, server, secagg, anchor, client, round)
    if compress is not None:
        if robust is not None:
            raise ValueError("the quantized exchange takes the plain mean (robust=None)")
        if anchor is None:
            raise ValueError("the quantized exchange needs the round's starting weights (anchor=)")
        return _compressed_(model, participate, comm, server, compress, anchor, client, round)
    if robust is not None:
        return _robust_(model, participate, comm, server, robust)
    if server is not None:
        return _fedopt_(model, weight, participate, comm, server)
    A = model.arena
    w = float(weight) if participate else 0.0
    if not _dist_on():
        if w == 0.0:
            return 0.0
        model.sync_shadow(force=True)
        return w
    dev = A.master.device
    wt = torch.tensor([w], dtype=torch.float64, device=dev)
    use_native = comm is not None and A.master.is_cuda

    def allreduce(t):
        if use_native:
            comm.all_reduce_(t, "sum")
        else:
            dist.all_reduce(t, op=dist.ReduceOp.SUM)

    allreduce(wt)
    total = float(wt.item())
    if total <= 0:
        raise RuntimeError("FedAvg round with no participating clients")
    if A.master.is_cuda:
        from ..ops import kernels as K
        if w != 1.0:
            K.scale_cast(A.master, None, w)          # pre-scale (0 drops the update)
        allreduce(A.master)
        K.scale_cast(A.master, A.shadow, 1.0 / total)  # fused 1/W scale + bf16 shadow refresh
        model.mark_shadow_synced()
    else:
        if w != 1.0:
            A.master.mul_(w)
        dist.all_reduce(A.master, op=dist.ReduceOp.SUM)
        A.master.mul_(1.0 / total)
        model.sync_shadow(force=True)
    return total


@torch.no_grad()
def _fedopt_(model, weight: float, participate: bool, comm, server) -> float:
    """``fedavg_`` with a server optimizer: the same weight exchange, pre-scale and all-reduce, then
    ``server.apply_`` on the weighted sum instead of the 1/W scale."""
    A = model.arena
    w = float(weight) if participate else 0.0
    if not _dist_on():
        if w == 0.0:
            return 0.0
        server.apply_(model, 1.0)  # one client: its weights are the mean
        return w
    dev = A.master.device
    wt = torch.tensor([w], dtype=torch.float64, device=dev)
    use_native = comm is not None and A.master.is_cuda

    def allreduce(t):
        if use_native:
            comm.all_reduce_(t, "sum")
        else:
            dist.all_reduce(t, op=dist.ReduceOp.SUM)

    allreduce(wt)
    total = float(wt.item())
    if total <= 0:
        raise RuntimeError("FedAvg round with no participating clients")
    if w != 1.0:
        if A.master.is_cuda:
            from ..ops import kernels as K
            K.scale_cast(A.master, None, w)          # pre-scale (0 drops the update)
        else:
            A.master.mul_(w)
    allreduce(A.master)
    server.apply_(model, total)  # fused server step + bf16 shadow refresh on GPU
    return total


@torch.no_grad()
def _robust_(model, participate: bool, comm, server, robust) -> float:
    """``fedavg_`` with a robust aggregator (parallel/robust.py): every rank learns the live set from
    an all-reduced flag vector (one slot per rank), the masters are all-gathered, the rows of the
    participating clients (replica 0 of each, in client order) go through ``robust.aggregate_`` --
    one fused pass on the GPU for the coordinate-wise kinds, a few for the distance-based ones -- and,
    with a server optimizer, its step follows.  A client that does not participate contributes no row
    and still receives the aggregate; every rank computes the same aggregate from the same rows, so
    the ranks stay identical.

    Memory: the gather buffer is ``world x`` the master -- for DistilBERT (265 MB of fp32 master)
    2.1 GB at 8 ranks -- and lives for this call only."""
    A = model.arena
    if not _dist_on():
        if not participate:
            return 0.0
        robust.last = robust.aggregate_(model, [A.master.clone()], server)  # one client: its own weights
        return 1.0
    world, rank = dist.get_world_size(), dist.get_rank()
    dev = A.master.device
    use_native = comm is not None and A.master.is_cuda
    flags = torch.zeros(world, dtype=torch.float64, device=dev)
    flags[rank] = 1.0 if participate else 0.0
    if use_native:
        comm.all_reduce_(flags, "sum")
    else:
        dist.all_reduce(flags, op=dist.ReduceOp.SUM)
    g = max(1, int(robust.gpus_per_client))
    flags = flags.tolist()
    live = [c for c in range(world // g) if flags[c * g] > 0.0]
    if not live:
        raise RuntimeError("FedAvg round with no participating clients")
    if use_native:
        rows = comm.all_gather(A.master)
    else:
        rows = torch.empty((world, A.master.numel()), dtype=A.master.dtype, device=dev)
        if A.master.is_cuda:
            dist.all_gather_into_tensor(rows, A.master)
        else:
            dist.all_gather(list(rows.unbind(0)), A.master)
    robust.last = robust.aggregate_(model, [rows[c * g] for c in live], server)
    del rows
    return float(len(live))


@torch.no_grad()
def _compressed_(model, participate: bool, comm, server, compress, anchor, client: int, round: int) -> float:
    """``fedavg_`` with a quantized exchange (parallel/compress.py): every rank learns the live set
    from an all-reduced flag vector (one slot per rank), a participating rank encodes its update
    ``master - anchor`` (+ its residual) -- a rank that does not participate encodes nothing, so its
    residual keeps its content, and sends a row of zeros that no rank decodes -- the int32 payloads are
    all-gathered, and ``decode_mean_`` adds the mean of the live rows (in client order) to the anchor
    in one fused pass on the GPU; with a server optimizer its step follows.  Every rank decodes the
    same rows, so the ranks stay identical.

    Memory: the gather buffer is ``world x`` the payload -- for DistilBERT (265 MB of fp32 master)
    70.6 MB per client at int8 -- and lives for this call only."""
    A = model.arena
    compress.last = None
    if not _dist_on():
        if not participate:
            return 0.0
        compress.decode_mean_(model, [compress.encode_(A.master, anchor, client, round)], anchor, server)
        return 1.0
    world, rank = dist.get_world_size(), dist.get_rank()
    dev = A.master.device
    use_native = comm is not None and A.master.is_cuda
    flags = torch.zeros(world, dtype=torch.float64, device=dev)
    flags[rank] = 1.0 if participate else 0.0
    if use_native:
        comm.all_reduce_(flags, "sum")
    else:
        dist.all_reduce(flags, op=dist.ReduceOp.SUM)
    flags = flags.tolist()
    live = [c for c in range(world) if flags[c] > 0.0]
    if not live:
        raise RuntimeError("FedAvg round with no participating clients")
    if participate:
        mine = compress.encode_(A.master, anchor, client, round)
    else:
        mine = torch.zeros(compress.words(A.master.numel()), dtype=torch.int32, device=dev)
    if use_native:
        rows = comm.all_gather(mine)
    else:
        rows = torch.empty((world, mine.numel()), dtype=torch.int32, device=dev)
        if mine.is_cuda:
            dist.all_gather_into_tensor(rows, mine)
        else:
            dist.all_gather(list(rows.unbind(0)), mine)
    compress.decode_mean_(model, [rows[c] for c in live], anchor, server)
    del rows
    return float(len(live))


@torch.no_grad()
def _secagg_(model, participate: bool, comm, server, secagg, anchor, client: int, round: int) -> float:
    """``fedavg_`` with secure aggregation (parallel/secagg.py): every rank learns the live set from an
    all-reduced flag vector (one slot per rank = client) *before* anything is encoded, a participating
    rank masks the fixed-point codes of ``master - anchor`` with the streams of the live partners only --
    a rank that does not participate sends a row of zeros that no rank reads -- the int32 payloads are
    all-gathered, the summed check block is compared, and ``unmask_mean_`` adds the mean of the live
    rows' modular sum to the anchor in one fused pass on the GPU; with a server optimizer its step
    follows.  Every rank unmasks the same rows, so the ranks stay identical.

    Memory: the gather buffer is ``world x`` the payload (4 bytes per element, as the fp32 master) and
    lives for this call only."""
    A = model.arena
    secagg.last = None
    if not _dist_on():
        if not participate:
            return 0.0
        secagg.unmask_mean_(model, [secagg.mask_(A.master, anchor, client, round, [client])], anchor, server,
                            round=round)
        return 1.0
    world, rank = dist.get_world_size(), dist.get_rank()
    dev = A.master.device
    use_native = comm is not None and A.master.is_cuda
    flags = torch.zeros(world, dtype=torch.float64, device=dev)
    flags[rank] = 1.0 if participate else 0.0
    if use_native:
        comm.all_reduce_(flags, "sum")
    else:
        dist.all_reduce(flags, op=dist.ReduceOp.SUM)
    flags = flags.tolist()
    live = [c for c in range(world) if flags[c] > 0.0]
    if not live:
        raise RuntimeError("FedAvg round with no participating clients")
    if participate:
        mine = secagg.mask_(A.master, anchor, client, round, live)
    else:
        mine = torch.zeros(secagg.words(A.master.numel()), dtype=torch.int32, device=dev)
    if use_native:
        rows = comm.all_gather(mine)
    else:
        rows = torch.empty((world, mine.numel()), dtype=torch.int32, device=dev)
        if mine.is_cuda:
            dist.all_gather_into_tensor(rows, mine)
        else:
            dist.all_gather(list(rows.unbind(0)), mine)
    secagg.unmask_mean_(model, [rows[c] for c in live], anchor, server, round=round)
    del rows
    return float(len(live))


def aggregate_state_dicts(states: Sequence[Dict[str, torch.Tensor]], weights: Optional[Sequence[float]] = None,
                          num_clients: Optional[int] = None):
    """server.py:67-79 semantics: None unless exactly ``num_clients`` models; mean of float tensors."""
    if num_clients is not None and len(states) != num_clients:
        return None
    if not states:
        return None
    ws = list(weights) if weights is not None else [1.0] * len(states)
    tot = float(sum(ws))
    out = OrderedDict()
    for k, v0 in states[0].items():
        if torch.is_floating_point(v0):
            acc = torch.zeros_like(v0, dtype=torch.float32)
            for s, w in zip(states, ws):
                acc += s[k].to(acc.device, torch.float32) * w
            out[k] = (acc / tot).to(v0.dtype)
        else:
            out[k] = v0.clone()
    return out
