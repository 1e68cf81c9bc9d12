"""Quantized update exchange: int8 / int4 codes with per-group scales, and error feedback.

QSGD (Alistarh et al., "QSGD: Communication-Efficient SGD via Gradient Quantization and Encoding",
NeurIPS 2017) with the error feedback of EF-SGD (Karimireddy et al., "Error Feedback Fixes SignSGD
and other Gradient Compression Schemes", ICML 2019).  A client does not send its fp32 master but
the round update ``w - w_global``, quantized: one fp32 scale per group of 64 consecutive elements
and one 8- or 4-bit code per element.  What the rounding lost stays with the client as a residual
and is added to its next update, so the sum of what was sent telescopes to the sum of the updates
minus the last residual.  Bytes per fp32 byte: ``(bits / 8 + 1 / 16) / 4`` -- 3.76x smaller at int8,
7.11x at int4.

Specification (``torch_quantize_`` and ``torch_decode_mean_`` are it, literally; the HIP kernels of
csrc/kernels/compress.hip equal them bit for bit).  Flat fp32 tensors with ``n % 64 == 0`` (the
arena's alignment); every fp32 operation is rounded on its own.

* ``v = (w - anchor) + e`` (``e`` the residual; without one ``v = w - anchor``).
* Per group of 64: ``a = max |v|``.  The group is *empty* when ``a == 0``, when ``a`` is not finite, or
  when ``inv = qmax / a`` is not finite: scale ``s = +0``, codes 0, new residual ``e' = v`` -- but a
  group whose ``a`` is not finite is *bad* and gets ``e' = +0``: a NaN never lives on in the residual.
  Otherwise ``s = a / qmax``, ``t = v * inv``, ``q = clamp(floor(t + u), -qmax, qmax)``, ``e' = v - s *
  float(q)``.  ``qmax`` is 127 (int8) or 7 (int4).
* ``u = 0.5`` (nearest), or ``u = (x >> 8) * 2^-24`` (stochastic: unbiased), ``x`` word ``i % 4`` of the
  Philox4x32-10 block of float4 index ``j = first * 16 + i / 4`` with counter ``(j lo, j hi, round,
  client)`` and key ``(seed_lo ^ 0x51554e54, seed_hi)``: a seed shared with the privacy noise never
  repeats its stream.
* The payload is one int32 tensor: ``n * bits / 32`` words of codes (two's complement, element ``i`` at
  bit offset ``i * bits``, little-endian), then ``n / 64`` words holding the scales' bit patterns.
* ``stats = {update_l2 = |v|, error_l2 = |e'|, bad_groups}``: sums of squares in fp64, the root rounded
  to fp32; bad groups are left out of both sums.
* Decode: ``acc = 0``; for each of the M payloads in order ``acc = acc + s_c[g] * float(q_c[i])``;
  ``out = anchor + acc * float32(1 / M)``; ``shadow = bf16(out)``.

An arena pad (+0 in ``w`` and ``anchor``) stays +0 through encode and decode: its ``v`` is 0, its code
0 (``floor(0 + u) = 0`` for ``u < 1``), and ``anchor + 0 * inv = +0``.

Top-k sparsification (``compress="topk"``; Aji & Heafield, EMNLP 2017; Deep Gradient Compression, Lin
et al., ICLR 2018; Stich et al., "Sparsified SGD with Memory", NeurIPS 2018): the client sends only the
``k = max(1, floor(density * n))`` entries of ``v`` with the largest magnitudes and keeps everything
else as its residual, so ``sent + e' == v`` exactly and error feedback loses nothing.
``torch_topk_encode_`` and ``torch_topk_decode_mean_`` are the specification; the kernels of
csrc/kernels/sparsify.hip equal them bit for bit.

* Key of element ``i``: the 31-bit pattern of ``|v_i|``.  ``|v_i|`` inf or NaN: the element is *bad* -- no
  candidate, never sent, residual ``+0``, counted in ``bad_elems``.
* With ``k_eff = min(k, n - bad_elems)`` the sent set is the ``k_eff`` candidates with the largest keys,
  ties on the key broken by the lower index (``-0`` and ``+0`` have key 0; when fewer than ``k_eff``
  candidates are nonzero, zeros are sent, lowest index first: the payload size is fixed).
* ``e' = +0`` at sent and bad elements, ``e' = v`` elsewhere.
* Payload (int32), chunks of 4096 consecutive elements, ``C = ceil(n / 4096)``: ``C + 1`` offsets
  (``off[b]`` = sent entries in chunks ``< b``; ``off[C] = k_eff``), ``k`` words of fp32 bit patterns of
  ``v`` at the sent elements in ascending index (0 from ``k_eff`` on), ``ceil(k / 2)`` words of local
  indices ``i mod 4096`` as uint16 (entry ``j`` in the low -- ``j`` even -- or high half of word ``j / 2``;
  unused halves 0): ``topk_words(n, k) = C + 1 + k + ceil(k / 2)``, about 6 bytes per sent entry.
* ``stats = {update_l2, error_l2, bad_elems, sent = k_eff, threshold}``: the norms as above over the
  non-bad elements; ``threshold`` the smallest sent ``|v|`` (0 when nothing is sent).
* Decode: ``acc = 0``; for each payload in order ``acc[i] = acc[i] + val`` for each of its entries; ``out =
  anchor + acc * float32(1 / M)``.  A payload comes from another client, so in chunk ``b`` the decoder
  reads the entries ``[lo, hi)`` with ``lo = clamp(off[b], 0, k)``, ``hi = clamp(off[b + 1], lo, k)`` and
  drops an entry whose local index is not below the chunk's length: no content reads or writes out of
  bounds.  Limit: if a payload repeats an index inside a chunk (the encoder never does), which of the
  duplicates counts is unspecified.
* A pad stays +0: its ``v`` is +0, sent or not its residual is +0, and ``anchor + acc * inv = +0``.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .privacy import _MASK32, _seed_words, _stream_check, philox4x32_10

GROUP = 64
KEY_TAG = 0x51554E54  # "QUNT"
QMAX = {8: 127, 4: 7}
MODES = {"none": 0, "int8": 8, "int4": 4, "topk": -1}
ROUNDINGS = ("nearest", "stochastic")
MAX_CLIENTS = 16
_CHUNK4 = 1 << 16  # float4 blocks per Philox pass
TOPK_CHUNK = 4096   # elements per payload chunk: a local index fits 16 bits
TOPK_BAD = 0x7F800000  # keys from here on: inf / NaN


def _check_bits(bits: int) -> int:
    if int(bits) not in QMAX:
        raise ValueError(f"bits must be 8 or 4, got {bits!r}")
    return int(bits)


def payload_words(n: int, bits: int) -> int:
    """int32 words of the payload of ``n`` floats at ``bits``: the codes, then one scale per 64."""
    n, bits = int(n), _check_bits(bits)
    if n <= 0 or n % GROUP != 0:
        raise ValueError(f"a payload covers a positive multiple of {GROUP} elements, got {n}")
    return n * bits // 32 + n // GROUP


def payload_ratio(bits: int) -> float:
    """fp32 bytes per payload byte: 3.76 at int8, 7.11 at int4."""
    return 4.0 / (_check_bits(bits) / 8.0 + 1.0 / 16.0)


def stochastic_uniforms(n: int, seed: int, round: int, client: int, first: int = 0) -> torch.Tensor:
    """The ``n`` 24-bit uniforms in [0, 1) of the stream (seed, round, client) from group ``first`` on
    (module docstring), exact in fp32 (a CPU tensor)."""
    n = int(n)
    lo, hi = _seed_words(seed)
    _stream_check(round, client, first)
    n4 = (n + 3) // 4
    out = np.empty(4 * n4, dtype=np.float32)
    key = np.array([lo ^ KEY_TAG, hi], dtype=np.uint64)
    for a in range(0, n4, _CHUNK4):
        b = min(n4, a + _CHUNK4)
        j = np.uint64(int(first) * 16) + np.arange(a, b, dtype=np.uint64)
        ctr = np.empty((b - a, 4), dtype=np.uint64)
        ctr[:, 0] = j & _MASK32
        ctr[:, 1] = j >> np.uint64(32)
        ctr[:, 2] = np.uint64(int(round))
        ctr[:, 3] = np.uint64(int(client))
        x = philox4x32_10(ctr, key)
        out[4 * a:4 * b] = ((x >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)).reshape(-1)
    return torch.from_numpy(out[:n])


def pack_codes(q: torch.Tensor, bits: int) -> torch.Tensor:
    """int32 codes in [-2^(bits-1), 2^(bits-1)) -> int32 words, element ``i`` at bit offset ``i * bits``."""
    bits = _check_bits(bits)
    per = 32 // bits
    u = q.to(torch.int64).view(-1, per) & ((1 << bits) - 1)
    shifts = torch.arange(per, dtype=torch.int64, device=q.device) * bits
    word = (u << shifts).sum(dim=1)
    return torch.where(word >= 1 << 31, word - (1 << 32), word).to(torch.int32)


def unpack_codes(words: torch.Tensor, bits: int) -> torch.Tensor:
    """The inverse of ``pack_codes``: int32 words -> sign-extended int32 codes."""
    bits = _check_bits(bits)
    per = 32 // bits
    shifts = torch.arange(per, dtype=torch.int64, device=words.device) * bits
    u = ((words.to(torch.int64) & 0xFFFFFFFF).unsqueeze(1) >> shifts) & ((1 << bits) - 1)
    return torch.where(u >= 1 << (bits - 1), u - (1 << bits), u).to(torch.int32).reshape(-1)


def split_payload(payload: torch.Tensor, n: int, bits: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(codes int32 [n], scales fp32 [n / 64]) of a payload."""
    if payload.dtype != torch.int32 or payload.dim() != 1 or payload.numel() != payload_words(n, bits):
        raise ValueError(f"a payload of {n} elements at int{bits} is a flat int32 tensor of {payload_words(n, bits)} "
                         f"words, got {tuple(payload.shape)} {payload.dtype}")
    cw = int(n) * int(bits) // 32
    return unpack_codes(payload[:cw], bits), payload[cw:].contiguous().view(torch.float32)


def _l2(x: torch.Tensor) -> float:
    with np.errstate(over="ignore"):
        return float(np.float32(math.sqrt(float(x.double().square().sum()))))


@torch.no_grad()
def torch_quantize_(w: torch.Tensor, anchor: torch.Tensor, residual: Optional[torch.Tensor], bits: int,
                    rounding: str = "nearest", seed: int = 0, round: int = 0, client: int = 0,
                    first: int = 0) -> Tuple[torch.Tensor, Dict]:
    """The specification of the encoder in torch (module docstring): returns ``(payload, stats)`` and
    leaves the new residual in ``residual`` (in place; None: no error feedback).  ``stats`` is
    ``{"update_l2", "error_l2", "bad_groups"}``.  This is what CPU runs execute."""
    bits = _check_bits(bits)
    if rounding not in ROUNDINGS:
        raise ValueError(f"rounding must be one of {', '.join(ROUNDINGS)}; got {rounding!r}")
    ts = [w, anchor] + ([residual] if residual is not None else [])
    if any(t.dtype != torch.float32 or t.dim() != 1 or t.shape != w.shape for t in ts):
        raise ValueError("quantize takes flat fp32 tensors of one length")
    n = w.numel()
    payload_words(n, bits)
    f32 = torch.float32
    qmax = torch.tensor(float(QMAX[bits]), dtype=f32, device=w.device)
    zero = torch.zeros((), dtype=f32, device=w.device)
    v = w - anchor
    if residual is not None:
        v = v + residual
    g = v.view(-1, GROUP)
    a = g.abs().amax(dim=1)
    bad = ~torch.isfinite(a)
    inv = qmax / a
    empty = bad | (a == 0) | ~torch.isfinite(inv)
    s = torch.where(empty, zero, a / qmax)
    inv = torch.where(empty, zero, inv)
    if rounding == "stochastic":
        u = stochastic_uniforms(n, seed, round, client, first).to(w.device).view(-1, GROUP)
    else:
        _seed_words(seed)
        _stream_check(round, client, first)
        u = torch.tensor(0.5, dtype=f32, device=w.device)
    t = g * inv.unsqueeze(1)
    f = torch.floor(t + u)
    f = torch.where(empty.unsqueeze(1), zero, f).clamp(-float(QMAX[bits]), float(QMAX[bits]))
    back = s.unsqueeze(1) * f
    err = torch.where(bad.unsqueeze(1), zero, g - back)
    good = ~bad
    stats = {"update_l2": _l2(g[good]), "error_l2": _l2(err[good]), "bad_groups": int(bad.sum())}
    if residual is not None:
        residual.copy_(err.view(-1))
    payload = torch.cat([pack_codes(f.to(torch.int32).view(-1), bits), s.contiguous().view(torch.int32)])
    return payload, stats


@torch.no_grad()
def torch_decode_mean_(payloads: Sequence[torch.Tensor], anchor: torch.Tensor, out: torch.Tensor,
                       shadow: Optional[torch.Tensor], bits: int) -> None:
    """The specification of the decoder in torch: ``out = anchor + mean`` of the decoded payloads (in
    the given order), ``shadow`` (optional) = bf16(out)."""
    bits = _check_bits(bits)
    M = len(payloads)
    if not 1 <= M <= MAX_CLIENTS:
        raise ValueError(f"decode_mean takes 1 .. {MAX_CLIENTS} payloads, got {M}")
    if anchor.dtype != torch.float32 or out.dtype != torch.float32 or anchor.shape != out.shape or out.dim() != 1:
        raise ValueError("decode_mean takes flat fp32 anchor and out of one length")
    n = out.numel()
    acc = torch.zeros(n, dtype=torch.float32, device=out.device)
    for p in payloads:
        q, s = split_payload(p.to(out.device), n, bits)
        acc = acc + s.repeat_interleave(GROUP) * q.to(torch.float32)
    inv = torch.tensor(float(np.float32(1.0 / M)), dtype=torch.float32, device=out.device)
    out.copy_(anchor + acc * inv)
    if shadow is not None:
        shadow.copy_(out)


def topk_k(n: int, density: float) -> int:
    """Sent entries per client: ``max(1, floor(density * n))`` in Python floats; ``0 < density <= 0.5``."""
    density = float(density)
    if not 0.0 < density <= 0.5:
        raise ValueError(f"compress_density must lie in (0, 0.5], got {density!r}")
    return max(1, int(math.floor(density * int(n))))


def topk_words(n: int, k: int) -> int:
    """int32 words of the top-k payload of ``n`` floats with ``k`` entries: ``ceil(n / 4096) + 1``
    offsets, ``k`` values, ``ceil(k / 2)`` words of uint16 local indices."""
    n, k = int(n), int(k)
    if n <= 0 or n % GROUP != 0:
        raise ValueError(f"a payload covers a positive multiple of {GROUP} elements, got {n}")
    if not 1 <= k <= n // 2:
        raise ValueError(f"a top-k payload of {n} elements holds 1 .. {n // 2} entries, got {k}")
    return (n + TOPK_CHUNK - 1) // TOPK_CHUNK + 1 + k + (k + 1) // 2


def split_topk_payload(payload: torch.Tensor, n: int, k: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(offsets int32 [C + 1], values fp32 [k], local indices int64 [k]) of a top-k payload."""
    if payload.dtype != torch.int32 or payload.dim() != 1 or payload.numel() != topk_words(n, k):
        raise ValueError(f"a top-k payload of {n} elements with {k} entries is a flat int32 tensor of "
                         f"{topk_words(n, k)} words, got {tuple(payload.shape)} {payload.dtype}")
    C = (int(n) + TOPK_CHUNK - 1) // TOPK_CHUNK
    words = payload[C + 1 + k:].to(torch.int64) & 0xFFFFFFFF
    idx = torch.stack([words & 0xFFFF, words >> 16], dim=1).reshape(-1)[:k]
    return payload[:C + 1], payload[C + 1:C + 1 + k].contiguous().view(torch.float32), idx


@torch.no_grad()
def torch_topk_encode_(w: torch.Tensor, anchor: torch.Tensor, residual: Optional[torch.Tensor],
                       k: int) -> Tuple[torch.Tensor, Dict]:
    """The specification of the top-k encoder in torch (module docstring): returns ``(payload, stats)``
    and leaves the new residual in ``residual`` (in place; None: no error feedback).  ``stats`` is
    ``{"update_l2", "error_l2", "bad_elems", "sent", "threshold"}``.  This is what CPU runs execute."""
    ts = [w, anchor] + ([residual] if residual is not None else [])
    if any(t.dtype != torch.float32 or t.dim() != 1 or t.shape != w.shape for t in ts):
        raise ValueError("topk_encode takes flat fp32 tensors of one length")
    n, k = w.numel(), int(k)
    words = topk_words(n, k)
    dev = w.device
    C = (n + TOPK_CHUNK - 1) // TOPK_CHUNK
    v = w - anchor
    if residual is not None:
        v = v + residual
    key = v.view(torch.int32) & 0x7FFFFFFF
    bad = key >= TOPK_BAD
    n_bad = int(bad.sum())
    k_eff = min(k, n - n_bad)
    key = torch.where(bad, torch.full_like(key, -1), key)       # below every candidate
    if k_eff > 0:
        T = int(torch.kthvalue(key, n - k_eff + 1).values)      # the k_eff-th largest key
        above = key > T
        tie = key == T
        budget = k_eff - int(above.sum())                       # ties sent, lowest index first
        sent = above | (tie & (torch.cumsum(tie, 0, dtype=torch.int64) <= budget))
    else:
        T = 0
        sent = torch.zeros(n, dtype=torch.bool, device=dev)
    idx = torch.nonzero(sent).view(-1)                          # ascending
    zero = torch.zeros((), dtype=torch.float32, device=dev)
    err = torch.where(sent | bad, zero, v)
    good = ~bad
    stats = {"update_l2": _l2(v[good]), "error_l2": _l2(err[good]), "bad_elems": n_bad, "sent": k_eff,
             "threshold": float(torch.tensor(T, dtype=torch.int32).view(torch.float32)) if k_eff else 0.0}
    if residual is not None:
        residual.copy_(err)
    payload = torch.zeros(words, dtype=torch.int32, device=dev)
    counts = torch.bincount(idx // TOPK_CHUNK, minlength=C)
    payload[1:C + 1] = torch.cumsum(counts, 0).to(torch.int32)
    payload[C + 1:C + 1 + k_eff] = v[idx].view(torch.int32)
    local = torch.zeros(2 * ((k + 1) // 2), dtype=torch.int64, device=dev)
    local[:k_eff] = idx % TOPK_CHUNK
    payload[C + 1 + k:] = (local[0::2] | (local[1::2] << 16)).to(torch.int32)   # (a local index is below 2^12)
    return payload, stats


@torch.no_grad()
def torch_topk_decode_mean_(payloads: Sequence[torch.Tensor], anchor: torch.Tensor, out: torch.Tensor,
                            shadow: Optional[torch.Tensor], k: int) -> None:
    """The specification of the top-k decoder in torch: ``out = anchor + mean`` of the M sparse payloads
    (added in the given order), ``shadow`` (optional) = bf16(out), with the guards of the module
    docstring: clamped, ascending offsets and no local index beyond its chunk."""
    M, k = len(payloads), int(k)
    if not 1 <= M <= MAX_CLIENTS:
        raise ValueError(f"decode_mean takes 1 .. {MAX_CLIENTS} payloads, got {M}")
    if anchor.dtype != torch.float32 or out.dtype != torch.float32 or anchor.shape != out.shape or out.dim() != 1:
        raise ValueError("decode_mean takes flat fp32 anchor and out of one length")
    n, dev = out.numel(), out.device
    C = (n + TOPK_CHUNK - 1) // TOPK_CHUNK
    chunk_len = torch.full((C,), TOPK_CHUNK, dtype=torch.int64, device=dev)
    chunk_len[-1] = n - (C - 1) * TOPK_CHUNK
    acc = torch.zeros(n, dtype=torch.float32, device=dev)
    for p in payloads:
        off, val, loc = split_topk_payload(p.to(dev), n, k)
        off = off.to(torch.int64)
        lo = off[:-1].clamp(0, k)
        hi = torch.maximum(off[1:], lo).clamp(max=k)
        cnt = hi - lo
        chunk = torch.repeat_interleave(torch.arange(C, device=dev), cnt)      # the chunk of each read entry
        j = lo[chunk] + (torch.arange(chunk.numel(), device=dev) - (torch.cumsum(cnt, 0) - cnt)[chunk])
        li = loc[j]
        ok = li < chunk_len[chunk]
        g = (chunk * TOPK_CHUNK + li)[ok]
        acc[g] = acc[g] + val[j[ok]]
    inv = torch.tensor(float(np.float32(1.0 / M)), dtype=torch.float32, device=dev)
    out.copy_(anchor + acc * inv)
    if shadow is not None:
        shadow.copy_(out)


class Compressor:
    """The quantizer of a job: ``bits`` 8 or 4, ``rounding`` "nearest" or "stochastic" (``seed`` is
    the 64-bit Philox key; client and round go into the counter), and -- with ``error_feedback`` --
    one residual per client (a process holds its own client's; a virtual-client job one per virtual
    client), allocated at the client's first encode and zero then.  ``last`` holds the latest encode's
    report: ``{"update_l2", "error_l2", "bad_groups", "payload_bytes", "ratio"}``."""

    def __init__(self, bits: int, error_feedback: bool = True, rounding: str = "nearest", seed: int = 0):
        self.bits = _check_bits(bits)
        if rounding not in ROUNDINGS:
            raise ValueError(f"compress_rounding must be one of {', '.join(ROUNDINGS)}; got {rounding!r}")
        self.error_feedback = bool(error_feedback)
        self.rounding = rounding
        self.seed = int(seed)
        _seed_words(self.seed)
        self.residuals: Dict[int, torch.Tensor] = {}
        self.last: Optional[Dict] = None
        self._work = None  # (device, partial, stats)

    def residual(self, client: int, like: torch.Tensor) -> Optional[torch.Tensor]:
        """The client's residual (created as zeros like ``like``), or None without error feedback."""
        if not self.error_feedback:
            return None
        e = self.residuals.get(int(client))
        if e is None or e.shape != like.shape or e.device != like.device:
            e = self.residuals[int(client)] = torch.zeros_like(like)
        return e

    def reset(self) -> None:
        """Forget every residual (an elastic restart: the next encode starts from zero)."""
        self.residuals.clear()

    def words(self, n: int) -> int:
        """int32 words of one client's payload of ``n`` floats."""
        return payload_words(n, self.bits)

    def describe(self) -> str:
        """The exchange in a few words, for a log line."""
        return f"int{self.bits}"

    @torch.no_grad()
    def encode_(self, master: torch.Tensor, anchor: torch.Tensor, client: int, round: int) -> torch.Tensor:
        """The payload of ``master - anchor`` plus the client's residual, which is advanced in place.
        On CUDA one ``quant_encode`` call; on the CPU the specification."""
        n = master.numel()
        words = payload_words(n, self.bits)
        e = self.residual(client, master)
        if master.is_cuda:
            from ..ops import kernels as K
            grid = K.quant_grid(n)
            if self._work is None or self._work[0] != master.device or self._work[1].numel() < 3 * grid:
                self._work = (master.device, torch.empty(3 * grid, dtype=torch.float64, device=master.device),
                              torch.empty(4, dtype=torch.float64, device=master.device))
            _, partial, stats = self._work
            payload = torch.empty(words, dtype=torch.int32, device=master.device)
            K.quant_encode(master, anchor, e, payload, partial, stats, self.bits, self.rounding == "stochastic",
                           self.seed, int(round), int(client))
            up, er, bad, _ = stats.tolist()
            rep = {"update_l2": float(up), "error_l2": float(er), "bad_groups": int(bad)}
        else:
            payload, rep = torch_quantize_(master, anchor, e, self.bits, self.rounding, self.seed, int(round),
                                           int(client))
        rep.update(payload_bytes=4 * words, ratio=n / float(words))
        self.last = rep
        return payload

    @torch.no_grad()
    def decode_mean_(self, model, payloads: Sequence[torch.Tensor], anchor: torch.Tensor, server=None) -> None:
        """The model's master (and bf16 shadow) become ``anchor`` plus the mean of the decoded
        ``payloads`` (1 .. 16, in the given order).  With a server optimizer the mean is decoded into the
        master without a shadow and ``server.apply_(model, 1.0)`` makes its step on it."""
        A = model.arena
        if not 1 <= len(payloads) <= MAX_CLIENTS:
            raise ValueError(f"the quantized exchange takes 1 .. {MAX_CLIENTS} participating clients, got "
                             f"{len(payloads)}")
        if A.master.is_cuda:
            from ..ops import kernels as K
            shadow = A.shadow if server is None else None
            K.quant_decode_mean(list(payloads), anchor, A.master, shadow, self.bits)
            if server is None:
                if shadow is not None:
                    model.mark_shadow_synced()
                else:
                    model.sync_shadow(force=True)
        else:
            torch_decode_mean_(list(payloads), anchor, A.master, None, self.bits)
            if server is None:
                model.sync_shadow(force=True)
        if server is not None:
            server.apply_(model, 1.0)


class TopKCompressor(Compressor):
    """The top-k sparsifier of a job (module docstring): every client sends the ``k = max(1,
    floor(density * n))`` largest-magnitude entries of its update plus residual and -- with
    ``error_feedback`` -- keeps the rest as its residual; the interface is ``Compressor``'s.  ``last`` holds
    the latest encode's report: ``{"update_l2", "error_l2", "bad_elems", "sent", "threshold",
    "payload_bytes", "ratio"}``."""

    bits = None  # (no code width: ``words`` and ``describe`` are what callers ask)

    def __init__(self, density: float = 0.01, error_feedback: bool = True):
        self.density = float(density)
        topk_k(GROUP * 2, self.density)  # (the range check)
        self.error_feedback = bool(error_feedback)
        self.rounding = "nearest"
        self.seed = 0
        self.residuals: Dict[int, torch.Tensor] = {}
        self.last: Optional[Dict] = None
        self._work = None  # (device, work, stats)

    def k(self, n: int) -> int:
        return topk_k(n, self.density)

    def words(self, n: int) -> int:
        return topk_words(n, self.k(n))

    def describe(self) -> str:
        return f"top-k, density {self.density:g}"

    @torch.no_grad()
    def encode_(self, master: torch.Tensor, anchor: torch.Tensor, client: int, round: int) -> torch.Tensor:
        """The sparse payload of ``master - anchor`` plus the client's residual, which becomes what was
        not sent, in place.  On CUDA one ``topk_encode`` call (a fixed sequence of launches); on the CPU
        the specification."""
        n = master.numel()
        k = self.k(n)
        words = topk_words(n, k)
        e = self.residual(client, master)
        if master.is_cuda:
            from ..ops import kernels as K
            nbytes = K.topk_work_bytes(n)
            if self._work is None or self._work[0] != master.device or self._work[1].numel() < nbytes:
                self._work = (master.device, torch.empty(nbytes, dtype=torch.uint8, device=master.device),
                              torch.empty(8, dtype=torch.float64, device=master.device))
            _, work, stats = self._work
            payload = torch.empty(words, dtype=torch.int32, device=master.device)
            K.topk_encode(master, anchor, e, payload, work, stats, k)
            up, er, bad, sent, thr = stats.tolist()[:5]
            rep = {"update_l2": float(up), "error_l2": float(er), "bad_elems": int(bad), "sent": int(sent),
                   "threshold": float(thr)}
        else:
            payload, rep = torch_topk_encode_(master, anchor, e, k)
        rep.update(payload_bytes=4 * words, ratio=n / float(words))
        self.last = rep
        return payload

    @torch.no_grad()
    def decode_mean_(self, model, payloads: Sequence[torch.Tensor], anchor: torch.Tensor, server=None) -> None:
        """The model's master (and bf16 shadow) become ``anchor`` plus the mean of the scattered
        ``payloads`` (1 .. 16, added in the given order); a server optimizer steps as in ``Compressor``."""
        A = model.arena
        if not 1 <= len(payloads) <= MAX_CLIENTS:
            raise ValueError(f"the sparsified exchange takes 1 .. {MAX_CLIENTS} participating clients, got "
                             f"{len(payloads)}")
        k = self.k(A.master.numel())
        if A.master.is_cuda:
            from ..ops import kernels as K
            shadow = A.shadow if server is None else None
            K.topk_decode_mean(list(payloads), anchor, A.master, shadow, k)
            if server is None:
                if shadow is not None:
                    model.mark_shadow_synced()
                else:
                    model.sync_shadow(force=True)
        else:
            torch_topk_decode_mean_(list(payloads), anchor, A.master, None, k)
            if server is None:
                model.sync_shadow(force=True)
        if server is not None:
            server.apply_(model, 1.0)


def check_compress_config(cfg, gpus_per_client: int = 1) -> int:
    """The configuration's code width (8 or 4; 0 for ``compress="none"``, -1 for ``"topk"``), or a
    ValueError naming the flag for a value or a combination the compressed exchange does not run with.
    Needs no model: callers refuse a bad configuration before any work."""
    mode = str(getattr(cfg, "compress", "none")).lower()
    if mode not in MODES:
        raise ValueError(f"compress must be one of {', '.join(MODES)}; got {getattr(cfg, 'compress', None)!r}")
    rounding = str(getattr(cfg, "compress_rounding", "nearest")).lower()
    if rounding not in ROUNDINGS:
        raise ValueError(f"compress_rounding must be one of {', '.join(ROUNDINGS)}; got "
                         f"{getattr(cfg, 'compress_rounding', None)!r}")
    if mode == "none":
        return 0
    if mode == "topk":
        topk_k(GROUP * 2, getattr(cfg, "compress_density", 0.01))  # (a density outside (0, 0.5])
        if rounding == "stochastic":
            raise ValueError("compress='topk' does not take compress_rounding='stochastic': the sent values are "
                             "exact, nothing is rounded")
    if getattr(cfg, "transport", "collective") == "tcp":
        raise ValueError(f"compress={mode!r} needs transport='collective': the reference-compatible TCP server takes "
                         f"fp32 state dicts")
    if str(getattr(cfg, "aggregator", "mean")).lower() != "mean":
        raise ValueError(f"compress={mode!r} needs aggregator='mean': order statistics of quantized updates are not "
                         f"built")
    if getattr(cfg, "weighted_fedavg", False):
        raise ValueError(f"compress={mode!r} does not take weighted_fedavg=True: the decoded mean is unweighted")
    if int(gpus_per_client) > 1:
        raise ValueError(f"compress={mode!r} needs gpus_per_client=1: a client's replicas would each keep a residual")
    return MODES[mode]


def make_compressor(cfg, gpus_per_client: int = 1) -> Optional[Compressor]:
    """The configuration's ``Compressor`` (``--compress int8``) or ``TopKCompressor`` (``--compress topk
    --compress-density 0.01``), or None for ``compress="none"`` (today's path, untouched).  The stochastic
    seed is ``base_seed`` (as 64 bits)."""
    bits = check_compress_config(cfg, gpus_per_client)
    if not bits:
        return None
    if bits < 0:
        return TopKCompressor(float(getattr(cfg, "compress_density", 0.01)),
                              bool(getattr(cfg, "compress_error_feedback", True)))
    return Compressor(bits, bool(getattr(cfg, "compress_error_feedback", True)),
                      str(getattr(cfg, "compress_rounding", "nearest")).lower(),
                      int(getattr(cfg, "base_seed", 0)) & ((1 << 64) - 1))
