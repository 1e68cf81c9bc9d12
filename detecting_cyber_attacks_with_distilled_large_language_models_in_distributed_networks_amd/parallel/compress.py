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
MODES = {"none": 0, "int8": 8, "int4": 4}
ROUNDINGS = ("nearest", "stochastic")
MAX_CLIENTS = 16
_CHUNK4 = 1 << 16  # float4 blocks per Philox pass


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


def check_compress_config(cfg, gpus_per_client: int = 1) -> int:
    """The configuration's code width (8 or 4; 0 for ``compress="none"``), or a ValueError naming the
    flag for a value or a combination the quantized exchange does not run with.  Needs no model:
    callers refuse a bad configuration before any work."""
    mode = str(getattr(cfg, "compress", "none")).lower()
    if mode not in MODES:
        raise ValueError(f"compress must be one of {', '.join(MODES)}; got {getattr(cfg, 'compress', None)!r}")
    rounding = str(getattr(cfg, "compress_rounding", "nearest")).lower()
    if rounding not in ROUNDINGS:
        raise ValueError(f"compress_rounding must be one of {', '.join(ROUNDINGS)}; got "
                         f"{getattr(cfg, 'compress_rounding', None)!r}")
    if mode == "none":
        return 0
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
    """The configuration's ``Compressor`` (``--compress int8``), or None for ``compress="none"``
    (today's path, untouched).  The stochastic seed is ``base_seed`` (as 64 bits)."""
    bits = check_compress_config(cfg, gpus_per_client)
    if not bits:
        return None
    return Compressor(bits, bool(getattr(cfg, "compress_error_feedback", True)),
                      str(getattr(cfg, "compress_rounding", "nearest")).lower(),
                      int(getattr(cfg, "base_seed", 0)) & ((1 << 64) - 1))
