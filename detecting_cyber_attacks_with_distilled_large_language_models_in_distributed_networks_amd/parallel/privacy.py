"""Client-level differential privacy for the federated exchange: clip, then Gaussian noise.

DP-FedAvg (McMahan et al., "Learning Differentially Private Recurrent Language Models", ICLR 2018;
Geyer et al., "Differentially Private Federated Learning: A Client Level Perspective", 2017).  Every
sampled client bounds the L2 norm of its round update ``w - w_global`` by ``C`` and the sum of the
updates carries Gaussian noise of std ``z * C``.  There is no trusted server here -- every rank is
the server -- so the noise is distributed: each of the round's ``M`` sampled clients adds
``N(0, (z C)^2 / M)`` to its own update before the exchange, and the sum carries ``N(0, (z C)^2)``.

Specification (``torch_privatize_`` is it, literally; the HIP kernels of csrc/kernels/privacy.hip
equal it bit for bit given the same norm).  Inputs: flat fp32 ``w`` and ``anchor`` of length n.

* ``norm = float32(sqrt(sum (w - anchor)^2))``, the differences in fp32, the sum in fp64.
* ``norm <= C``: flag 0, ``u = w`` (an unclipped update is not re-rounded through ``a + (w - a)``);
  ``norm > C``: flag 1, ``scale = C / norm`` (fp32), ``d = w - a; t = scale * d; u = a + t``, every
  operation rounded on its own; a norm that is not finite: flag 2, ``u = a`` -- a diverged client
  sends a zero update, never NaN or inf.
* ``sigma != 0``: ``u = u + sigma * g(index)``, ``g`` the generator below.

The generator is counter-based, so a value depends on its global index alone: Philox4x32-10 (Salmon
et al., SC 2011) with key ``(seed_lo, seed_hi)`` and counter ``(j lo, j hi, round, client)`` for
float4 index ``j``; the block's four words give the float4's four Gaussians by two Box-Muller pairs,
``u1 = ((x0 >> 8) + 1) 2^-24`` in (0, 1], ``u2 = (x1 >> 8) 2^-24`` in [0, 1), ``r = sqrt(-2 ln u1)``,
``g0 = r cos(2 pi u2)``, ``g1 = r sin(2 pi u2)``; ``g2, g3`` likewise from ``x2, x3``.  The 24-bit
uniforms are exact in fp32, so host and device start from identical values; ``|g| <= sqrt(48 ln 2)``
= 5.77.  ``philox4x32_10`` mirrors the device's integers bit for bit; ``torch_gauss`` evaluates the
Box-Muller in fp64 and rounds to fp32 (the device's fp32 evaluation stays within 2e-5 of it:
tests/test_privacy_gpu.py).

Limits, stated plainly.  The Gaussian is a 24-bit-uniform Box-Muller in fp32 with its tail cut at
5.77 sigma: the floating-point caveats of Mironov ("On Significance of the Least Significant Bits
for Differential Privacy", CCS 2012) apply.  ``epsilon`` credits no subsampling amplification.  The
guarantee is client-level, against the other participants and the model's consumers.  A sampled
client that drops out lowers the round's noise below what is accounted.
"""
from __future__ import annotations

import math
import os
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
GAUSS_MAX = math.sqrt(48.0 * math.log(2.0))  # u1 >= 2^-24
_MASK32 = np.uint64(0xFFFFFFFF)
_CHUNK4 = 1 << 14  # float4 blocks per pass of torch_gauss (its uint64 temporaries stay in cache)


def f32(value: float) -> float:
    """``value`` rounded to fp32, as a Python float."""
    with np.errstate(over="ignore"):
        return float(np.float32(value))


def philox4x32_10(counter, key) -> np.ndarray:
    """Philox4x32-10 in numpy uint64 (a 32 x 32 product fits a uint64, so the arithmetic is exact):
    ``counter`` [..., 4] and ``key`` [..., 2] (or one key for all) of 32-bit words -> [..., 4] words."""
    c = np.asarray(counter, dtype=np.uint64)
    k = np.asarray(key, dtype=np.uint64)
    if c.shape[-1] != 4 or k.shape[-1] != 2:
        raise ValueError("philox4x32_10 takes counters of 4 words and keys of 2")
    c0, c1, c2, c3 = (c[..., i] & _MASK32 for i in range(4))
    k0, k1 = (k[..., i] & _MASK32 for i in range(2))
    m0, m1 = np.uint64(PHILOX_M0), np.uint64(PHILOX_M1)
    w0, w1 = np.uint64(PHILOX_W0), np.uint64(PHILOX_W1)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & _MASK32, (p0 >> s32) ^ c3 ^ k1, p0 & _MASK32
        k0, k1 = (k0 + w0) & _MASK32, (k1 + w1) & _MASK32
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1)


def _seed_words(seed: int) -> Tuple[int, int]:
    seed = int(seed)
    if not 0 <= seed < 1 << 64:
        raise ValueError(f"privacy seed must lie in [0, 2^64), got {seed}")
    return seed & 0xFFFFFFFF, seed >> 32


def _stream_check(round: int, client: int, first4: int):
    if not 0 <= int(round) < 1 << 32 or not 0 <= int(client) < 1 << 32 or int(first4) < 0:
        raise ValueError(f"privacy stream: round and client in [0, 2^32), first4 >= 0; got {round}, {client}, {first4}")


def torch_gauss(n: int, seed: int, round: int, client: int, first4: int = 0) -> torch.Tensor:
    """``n`` standard Gaussians of the stream (seed, round, client) from global index ``4 * first4``
    on: the generator of the module docstring, its Box-Muller evaluated in fp64 and rounded to fp32
    (a CPU tensor)."""
    n = int(n)
    lo, hi = _seed_words(seed)
    _stream_check(round, client, first4)
    n4 = (n + 3) // 4
    out = np.empty(4 * n4, dtype=np.float32)
    key = np.array([lo, hi], dtype=np.uint64)
    for a in range(0, n4, _CHUNK4):
        b = min(n4, a + _CHUNK4)
        j = np.uint64(first4) + np.arange(a, b, dtype=np.uint64)
        ctr = np.empty((b - a, 4), dtype=np.uint64)
        ctr[:, 0] = j & _MASK32
        ctr[:, 1] = j >> np.uint64(32)
        ctr[:, 2] = np.uint64(int(round))
        ctr[:, 3] = np.uint64(int(client))
        x = philox4x32_10(ctr, key)
        g = np.empty((b - a, 4), dtype=np.float64)
        for p in (0, 2):
            u1 = ((x[:, p] >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24
            u2 = (x[:, p + 1] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
            r = np.sqrt(-2.0 * np.log(u1))
            g[:, p] = r * np.cos(2.0 * np.pi * u2)
            g[:, p + 1] = r * np.sin(2.0 * np.pi * u2)
        out[4 * a:4 * b] = g.reshape(-1).astype(np.float32)
    return torch.from_numpy(out[:n])


def clip_stats(norm: float, clip: float) -> Tuple[float, int]:
    """(scale, flag) of an update of fp32 norm ``norm`` under the bound ``clip``, both as fp32."""
    norm32, clip32 = np.float32(norm), np.float32(clip)
    if not np.isfinite(norm32):
        return 0.0, 2
    if norm32 > clip32:
        return float(np.float32(clip32 / norm32)), 1
    return 1.0, 0


@torch.no_grad()
def torch_privatize_(w: torch.Tensor, anchor: torch.Tensor, clip: float, sigma: float, seed: int = 0,
                     round: int = 0, client: int = 0, first4: int = 0, stats=None,
                     shadow: Optional[torch.Tensor] = None) -> Dict:
    """The specification of norm + apply in torch, in place on ``w`` (module docstring): the norm in
    fp64, the element arithmetic in fp32, one op per step.  ``stats`` -- (norm, scale, flag), e.g. the
    device's -- takes the place of the norm pass.  ``shadow`` (optional) receives ``bf16(w)``.  Returns
    ``{"update_l2", "scale", "clipped", "sigma"}``; this is what CPU runs (``impl="torch"``, gloo)
    execute."""
    if w.dtype != torch.float32 or anchor.dtype != torch.float32 or w.shape != anchor.shape or w.dim() != 1:
        raise ValueError("privatize takes flat fp32 tensors of one length")
    clip, sigma = float(clip), f32(sigma)
    if not (math.isfinite(clip) and f32(clip) > 0.0):
        raise ValueError(f"clip must be finite and > 0, got {clip!r}")
    if not (math.isfinite(sigma) and sigma >= 0.0):
        raise ValueError(f"sigma must be finite and >= 0, got {sigma!r}")
    if stats is None:
        d = w - anchor
        norm = f32(math.sqrt(float(d.double().square().sum())))
        scale, flag = clip_stats(norm, clip)
    else:
        norm, scale, flag = float(stats[0]), float(stats[1]), int(stats[2])
    if flag == 1:
        d = w - anchor
        t = d * torch.tensor(scale, dtype=torch.float32, device=w.device)
        w.copy_(anchor + t)
    elif flag == 2:
        w.copy_(anchor)
    elif flag != 0:
        raise ValueError(f"clip flag must be 0, 1 or 2; got {flag}")
    if sigma != 0.0:
        g = torch_gauss(w.numel(), seed, round, client, first4).to(w.device)
        w.copy_(w + g * torch.tensor(sigma, dtype=torch.float32, device=w.device))
    if shadow is not None:
        shadow.copy_(w)
    return {"update_l2": norm, "scale": scale, "clipped": flag, "sigma": sigma}


def epsilon(rounds: int, z: float, delta: float) -> float:
    """The (epsilon, delta) spent by ``rounds`` releases of the Gaussian mechanism with noise multiplier
    ``z`` (std ``z C`` on a sum of sensitivity ``C``: add or remove one client), by Renyi accounting
    without amplification: ``min over alpha > 1 of R alpha / (2 z^2) + ln(1 / delta) / (alpha - 1) =
    R / (2 z^2) + sqrt(2 R ln(1 / delta)) / z``.  ``inf`` at ``z = 0``.  Partial participation only
    amplifies privacy, and none of it is credited: the figure is an upper bound."""
    R, z, delta = int(rounds), float(z), float(delta)
    if R < 0 or not (z >= 0.0) or not 0.0 < delta < 1.0:
        raise ValueError(f"epsilon takes rounds >= 0, z >= 0 and delta in (0, 1); got {rounds}, {z}, {delta}")
    if R == 0:
        return 0.0
    if z == 0.0:
        return math.inf
    return R / (2.0 * z * z) + math.sqrt(2.0 * R * math.log(1.0 / delta)) / z


def arena_pads(arena) -> List[Tuple[int, int]]:
    """The [start, end) ranges of the arena's alignment pads: behind every tensor whose size is not a
    multiple of the 64-float alignment, up to the next tensor (or the arena's end)."""
    spans = sorted((off, off + math.prod(shape)) for off, shape in arena.offsets.values())
    starts = [s for s, _ in spans[1:]] + [int(arena.numel)]
    return [(end, nxt) for (_, end), nxt in zip(spans, starts) if nxt > end]


class Privatizer:
    """Clip + noise of one client's round update, in place on the fp32 master it is about to send.

    ``clip`` is C, ``noise_multiplier`` z, ``delta`` the accountant's delta; ``seed`` the 64-bit Philox
    key (None: 64 bits from ``os.urandom``, per process -- predictable noise is no privacy; an int:
    fixed, for tests and reproduction).  Client and round go into the Philox counter, so one seed
    never repeats a stream.  ``last`` holds the latest call's report."""

    def __init__(self, clip: float, noise_multiplier: float = 0.0, delta: float = 1e-5, seed: Optional[int] = None):
        self.clip = float(clip)
        self.noise_multiplier = float(noise_multiplier)
        self.delta = float(delta)
        if not (math.isfinite(self.clip) and f32(self.clip) > 0.0):
            raise ValueError(f"privacy_clip must be finite and > 0, got {clip!r}")
        if not (math.isfinite(self.noise_multiplier) and self.noise_multiplier >= 0.0):
            raise ValueError(f"privacy_noise must be finite and >= 0, got {noise_multiplier!r}")
        if not 0.0 < self.delta < 1.0:
            raise ValueError(f"privacy_delta must lie in (0, 1), got {delta!r}")
        self.seed = int.from_bytes(os.urandom(8), "little") if seed is None else int(seed)
        _seed_words(self.seed)
        self.last: Optional[Dict] = None
        self._work = None   # (device, partial, stats)
        self._pads = None   # (arena key, index tensor)

    def sigma(self, n_sampled: int) -> float:
        """The std each of ``n_sampled`` clients adds: ``float32(z C / sqrt(n_sampled))``."""
        if int(n_sampled) < 1:
            raise ValueError(f"a round of {n_sampled} sampled clients")
        return f32(self.noise_multiplier * self.clip / math.sqrt(int(n_sampled)))

    def epsilon(self, rounds: int) -> float:
        return epsilon(rounds, self.noise_multiplier, self.delta)

    def _pad_index(self, arena, device) -> Optional[torch.Tensor]:
        key = (id(arena), int(arena.numel), str(device))
        if self._pads is None or self._pads[0] != key:
            idx = [i for a, b in arena_pads(arena) for i in range(a, b)]
            self._pads = (key, torch.tensor(idx, dtype=torch.long, device=device) if idx else None)
        return self._pads[1]

    @torch.no_grad()
    def privatize_(self, master: torch.Tensor, anchor: torch.Tensor, client_idx: int, round_idx: int,
                   n_sampled: int, shadow: Optional[torch.Tensor] = None, arena=None) -> Dict:
        """``master`` (the trained weights, flat fp32) becomes what the client sends: ``anchor`` (the
        round's starting weights) plus the clipped update plus ``N(0, sigma^2)``, ``sigma =
        float32(z C / sqrt(n_sampled))``; ``shadow`` (optional) = bf16 of it.  On CUDA the two kernel
        calls (``privacy_norm``, ``privacy_apply``; the device reads its own norm, so no host sync
        sits between the passes); on the CPU the specification.  With ``arena`` the alignment pads are
        reset to +0 in ``master`` and ``shadow`` afterwards (pad positions simply consume noise
        indices): "a pad is +0 in every client" survives the noise.  Returns (and leaves in ``last``)
        ``{"update_l2", "scale", "clipped" (0 / 1 / 2), "sigma"}``."""
        sigma = self.sigma(n_sampled)
        if master.is_cuda:
            from ..ops import kernels as K
            n = master.numel()
            if self._work is None or self._work[0] != master.device:
                self._work = (master.device,
                              torch.empty(K.privacy_grid(n), dtype=torch.float64, device=master.device),
                              torch.empty(4, dtype=torch.float32, device=master.device))
            _, partial, stats = self._work
            if partial.numel() < K.privacy_grid(n):
                partial = torch.empty(K.privacy_grid(n), dtype=torch.float64, device=master.device)
                self._work = (master.device, partial, stats)
            K.privacy_norm(master, anchor, partial, stats, self.clip)
            K.privacy_apply(master, anchor, shadow, stats, sigma, self.seed, int(round_idx), int(client_idx))
            norm, scale, flag, _ = stats.tolist()
            rep = {"update_l2": float(norm), "scale": float(scale), "clipped": int(flag), "sigma": sigma}
        else:
            rep = torch_privatize_(master, anchor, self.clip, sigma, self.seed, int(round_idx), int(client_idx),
                                   shadow=shadow)
        if arena is not None:
            idx = self._pad_index(arena, master.device)
            if idx is not None:
                master.index_fill_(0, idx, 0.0)
                if shadow is not None:
                    shadow.index_fill_(0, idx, 0.0)
        self.last = rep
        return rep


def check_privacy_config(cfg, gpus_per_client: int = 1) -> bool:
    """Whether the configuration asks for privacy (``privacy_clip > 0``), or a ValueError naming the
    flag for a value or a combination it does not run with.  Needs no model: callers refuse a bad
    configuration before any work."""
    clip = getattr(cfg, "privacy_clip", 0.0)
    z = getattr(cfg, "privacy_noise", 0.0)
    delta = getattr(cfg, "privacy_delta", 1e-5)
    seed = getattr(cfg, "privacy_seed", None)
    try:
        clip, z, delta = float(clip), float(z), float(delta)
    except (TypeError, ValueError):
        raise ValueError(f"privacy_clip / privacy_noise / privacy_delta must be numbers, got {clip!r}, {z!r}, "
                         f"{delta!r}") from None
    if not (math.isfinite(clip) and clip >= 0.0):
        raise ValueError(f"privacy_clip must be finite and >= 0 (0: off), got {clip!r}")
    if not (math.isfinite(z) and z >= 0.0):
        raise ValueError(f"privacy_noise must be finite and >= 0, got {z!r}")
    if z > 0.0 and clip == 0.0:
        raise ValueError(f"privacy_noise={z!r} needs privacy_clip > 0: the noise is calibrated to the clip bound")
    if not 0.0 < delta < 1.0:
        raise ValueError(f"privacy_delta must lie in (0, 1), got {delta!r}")
    if seed is not None and not 0 <= int(seed) < 1 << 64:
        raise ValueError(f"privacy_seed must lie in [0, 2^64), got {seed!r}")
    if clip == 0.0:
        return False
    if f32(clip) <= 0.0 or not math.isfinite(f32(clip)):
        raise ValueError(f"privacy_clip={clip!r} is not a positive fp32 number")
    if getattr(cfg, "weighted_fedavg", False):
        raise ValueError("privacy_clip does not take weighted_fedavg=True: sample weights break the sensitivity "
                         "bound of the sum")
    if int(gpus_per_client) > 1:
        raise ValueError("privacy_clip needs gpus_per_client=1: a client's replicas would draw different noise")
    return True


def make_privatizer(cfg, gpus_per_client: int = 1) -> Optional[Privatizer]:
    """The configuration's ``Privatizer`` (``--privacy-clip C --privacy-noise z``), or None when
    ``privacy_clip == 0`` (today's path, untouched)."""
    if not check_privacy_config(cfg, gpus_per_client):
        return None
    return Privatizer(float(cfg.privacy_clip), float(getattr(cfg, "privacy_noise", 0.0)),
                      float(getattr(cfg, "privacy_delta", 1e-5)), getattr(cfg, "privacy_seed", None))
