"""Secure aggregation for the federated exchange: fixed-point updates under pairwise ChaCha masks.

Bonawitz et al., "Practical Secure Aggregation for Privacy-Preserving Machine Learning" (CCS 2017), the
masking half.  Every pair of live clients shares a key; each client adds the pair's pseudorandom stream,
with opposite signs at the two ends, to a 32-bit fixed-point encoding of its round update ``w -
w_global``.  In the sum of the payloads modulo 2^32 the streams cancel and the sum of the updates is
left; a single payload, or any partial sum, is uniformly random to whoever lacks the keys.  So the
participants -- every rank is the server here -- learn the aggregate that the ``epsilon`` of
parallel/privacy.py accounts for, and not the individual updates, which carry 1 / M of its noise.

Specification (``torch_encode``, ``torch_mask`` and ``torch_unmask_mean_`` are it, literally; the HIP
kernels of csrc/kernels/secagg.hip equal them bit for bit).  Flat fp32 ``w`` and ``anchor`` of length
``n``, ``n % 16 == 0`` (the arena is 64-float aligned); ``f = secagg_frac_bits`` in 8 .. 30 (default 24);
every fp32 operation is rounded on its own.

* Fixed point: ``d = w - a``; ``t = d * 2^f``; ``r = rint(t)``, ties to even.  ``d`` not finite: ``q = 0`` and
  the element is *bad*; ``|r| >= 2^27`` (a ``t`` that overflowed included): ``q = +-(2^27 - 1)`` and the
  element is *clamped*; otherwise ``q = int32(r)``.  Sixteen clients' codes add without leaving int32.
* ``stats = {update_l2 = |d|, error_l2 = |d - float32(q) * 2^-f|, clamped, bad_elems}``: sums of squares in
  fp64 over the non-bad elements, the root rounded to fp32.
* Mask: ``y = uint32(q) + sum over the live partners j != i of s_ij * PRG(k_ij, nonce = (round, 0, 0))
  [element]  (mod 2^32)``, ``s_ij = +1`` for ``i < j`` and ``-1`` otherwise (client indices, not ranks).
* Payload: one int32 tensor of ``n + 16`` words; the last 16 are the *check block*, whose plaintext is ``q
  = 1`` in every client, under the next block of the same streams.
* PRG: the ChaCha block function of RFC 8439 section 2.3 -- four constants, 8 key words, a 32-bit block
  counter, 3 nonce words -- with ``secagg_chacha_rounds`` in {8, 12, 20} (default 20).  Block ``b`` (counter
  ``first_block + b``) covers elements ``16 b .. 16 b + 15``, and element ``e`` of the block takes the block's
  RFC word ``4 * (e % 4) + e // 4``: the transposed order, in which a quad of GPU lanes owns one column of
  the state and one float4 each (``WORD_ORDER``; ``stream_words`` applies it).  ``first_block + n / 16 + 1
  <= 2^32``.  ``chacha_block`` mirrors the device's integers bit for bit.
* Unmask, per element: ``s = int32(sum over the M live payloads of y_c mod 2^32)``; ``acc = float32(s)``
  (nearest even); ``out = anchor + (acc * 2^-f) * float32(1 / M)``; ``shadow = bf16(out)``.  Before it, the
  summed check block must equal ``M`` in all 16 words; if it does not, the live sets or the keys
  disagreed: ``RuntimeError`` naming the round, the master untouched.
* A pad stays +0: ``q = 0``, the masks cancel, ``anchor + 0 * inv = +0``.

Keys.  X25519 (RFC 7748: Montgomery ladder, ``p = 2^255 - 19``, ``a24 = 121665``, clamped scalars, the top
bit of ``u`` masked) in pure Python.  Each client draws its private key from ``os.urandom(32)`` when the
job starts (and again after an elastic restart); with ``secagg_seed`` (tests) it is ``SHA-256(b"fd-secagg
priv" + seed as 8 LE bytes + client as 4 LE bytes)``.  The 32-byte public keys are all-gathered once (as 8
int32 words each: ``gather_public_keys``), and ``setup_keys`` derives the pair keys there and then.
``k_ij = HMAC-SHA256(key = X25519(sk_i, pk_j), msg = b"fd-secagg v1" + pk_min(i,j) + pk_max(i,j))`` read as
8 little-endian words; an all-zero shared secret is refused.  The round goes into the nonce, so a pair
key never repeats a stream.

Limits, stated plainly.  The adversary is honest-but-curious.  Public keys are not authenticated: the
process group is the trusted channel.  There is no dropout recovery (the secret-sharing half of
Bonawitz et al.): the live set is agreed by the flag all-reduce before anything is masked, a rank that
dies after it fails the collective, and the elastic restart repeats the round.  The Python ladder is
not constant-time.  With two live clients the sum reveals each to the other (a warning is logged).  The
``virtual`` mode runs every client in one process: it exercises the arithmetic and hides nothing.
Fixed point adds an error of at most ``2^-(f+1)`` per client and element.
"""
from __future__ import annotations

import hashlib
import hmac
import logging
import math
import os
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

MAX_CLIENTS = 16
CHECK_WORDS = 16
QMAX = (1 << 27) - 1
FRAC_BITS = (8, 30)
CHACHA_ROUNDS = (8, 12, 20)
CHACHA_CONSTANTS = (0x61707865, 0x3320646E, 0x79622D32, 0x6B206574)  # "expand 32-byte k"
# element e of a block takes RFC word WORD_ORDER[e] = 4 * (e % 4) + e // 4
WORD_ORDER = tuple(4 * (e % 4) + e // 4 for e in range(16))
_MASK32 = np.uint64(0xFFFFFFFF)
_CHUNK = 1 << 14  # ChaCha blocks per pass of stream_words (its uint64 temporaries stay in cache)

X25519_P = (1 << 255) - 19
X25519_A24 = 121665
X25519_BASE = (9).to_bytes(32, "little")


def _check_params(frac_bits: int, rounds: int) -> Tuple[int, int]:
    if isinstance(frac_bits, bool) or int(frac_bits) != frac_bits or not FRAC_BITS[0] <= int(frac_bits) <= FRAC_BITS[1]:
        raise ValueError(f"secagg_frac_bits must be an integer in {FRAC_BITS[0]} .. {FRAC_BITS[1]}, got {frac_bits!r}")
    if isinstance(rounds, bool) or rounds not in CHACHA_ROUNDS:
        raise ValueError(f"secagg_chacha_rounds must be one of {CHACHA_ROUNDS}, got {rounds!r}")
    return int(frac_bits), int(rounds)


def secagg_words(n: int) -> int:
    """int32 words of the payload of ``n`` floats: one per element, then the check block."""
    n = int(n)
    if n <= 0 or n % 16 != 0:
        raise ValueError(f"a payload covers a positive multiple of 16 elements, got {n}")
    return n + CHECK_WORDS


# ------------------------------------------------------------------ ChaCha
def _rotl(x, k: int):
    return ((x << np.uint64(k)) & _MASK32) | (x >> np.uint64(32 - k))


def _quarter(s: List, a: int, b: int, c: int, d: int) -> None:
    s[a] = (s[a] + s[b]) & _MASK32
    s[d] = _rotl(s[d] ^ s[a], 16)
    s[c] = (s[c] + s[d]) & _MASK32
    s[b] = _rotl(s[b] ^ s[c], 12)
    s[a] = (s[a] + s[b]) & _MASK32
    s[d] = _rotl(s[d] ^ s[a], 8)
    s[c] = (s[c] + s[d]) & _MASK32
    s[b] = _rotl(s[b] ^ s[c], 7)


def chacha_block(key8, counter, nonce3, rounds: int = 20) -> np.ndarray:
    """The ChaCha block function (RFC 8439 section 2.3) with ``rounds`` rounds in numpy uint64 (a 32-bit
    sum fits a uint64, so the arithmetic is exact): ``key8`` 8 words, ``counter`` one 32-bit block counter
    or an array [...] of them, ``nonce3`` 3 words -> [..., 16] words in RFC order (as uint64)."""
    if rounds not in CHACHA_ROUNDS:
        raise ValueError(f"ChaCha rounds must be one of {CHACHA_ROUNDS}, got {rounds!r}")
    key = [int(k) for k in np.asarray(key8).reshape(-1)]
    nonce = [int(v) for v in np.asarray(nonce3).reshape(-1)]
    if len(key) != 8 or len(nonce) != 3 or any(not 0 <= v < 1 << 32 for v in key + nonce):
        raise ValueError("chacha_block takes 8 key words and 3 nonce words in [0, 2^32)")
    ctr = np.asarray(counter, dtype=np.uint64)
    if ctr.size and int(ctr.max()) >= 1 << 32:
        raise ValueError("chacha_block takes 32-bit block counters")
    init = [np.full(ctr.shape, v, dtype=np.uint64) for v in CHACHA_CONSTANTS + tuple(key)] + [ctr.copy()] \
        + [np.full(ctr.shape, v, dtype=np.uint64) for v in nonce]
    s = [x.copy() for x in init]
    for _ in range(rounds // 2):
        _quarter(s, 0, 4, 8, 12)
        _quarter(s, 1, 5, 9, 13)
        _quarter(s, 2, 6, 10, 14)
        _quarter(s, 3, 7, 11, 15)
        _quarter(s, 0, 5, 10, 15)
        _quarter(s, 1, 6, 11, 12)
        _quarter(s, 2, 7, 8, 13)
        _quarter(s, 3, 4, 9, 14)
    return np.stack([(a + b) & _MASK32 for a, b in zip(s, init)], axis=-1)


def _blocks_check(first_block: int, n: int, extra: int = 0) -> None:
    """The block counters ``first_block .. first_block + n / 16 - 1 + extra`` (``extra = 1``: the check block's)
    fit 32 bits."""
    if int(first_block) < 0 or int(first_block) + int(n) // 16 + int(extra) > 1 << 32:
        raise ValueError(f"secagg stream: first_block >= 0 and first_block + n / 16 + {int(extra)} <= 2^32; got "
                         f"first_block {first_block}, n {n}")


def stream_words(key8, nonce3, n: int, first_block: int = 0, rounds: int = 20) -> np.ndarray:
    """The ``n`` PRG words (uint32; ``n % 16 == 0``) of elements ``16 * first_block ..`` for one key and one
    nonce, in element order (``WORD_ORDER`` applied): the host mirror of ``secagg_stream``."""
    n = int(n)
    if n <= 0 or n % 16 != 0:
        raise ValueError(f"a stream covers a positive multiple of 16 elements, got {n}")
    _blocks_check(first_block, n)
    order = np.asarray(WORD_ORDER)
    out = np.empty((n // 16, 16), dtype=np.uint32)
    for a in range(0, n // 16, _CHUNK):
        b = min(n // 16, a + _CHUNK)
        ctr = np.uint64(int(first_block)) + np.arange(a, b, dtype=np.uint64)
        out[a:b] = chacha_block(key8, ctr, nonce3, rounds)[:, order].astype(np.uint32)
    return out.reshape(-1)


# ------------------------------------------------------------------ X25519 and the pair keys
def x25519(k: bytes, u: bytes) -> bytes:
    """X25519(k, u) of RFC 7748 section 5: the Montgomery ladder on Python integers (not constant-time)."""
    if len(k) != 32 or len(u) != 32:
        raise ValueError("x25519 takes a 32-byte scalar and a 32-byte u-coordinate")
    kb = bytearray(k)
    kb[0] &= 248
    kb[31] &= 127
    kb[31] |= 64
    scalar = int.from_bytes(kb, "little")
    p = X25519_P
    x1 = int.from_bytes(u, "little") & ((1 << 255) - 1)
    x2, z2, x3, z3, swap = 1, 0, x1, 1, 0
    for t in range(254, -1, -1):
        kt = (scalar >> t) & 1
        swap ^= kt
        if swap:
            x2, x3, z2, z3 = x3, x2, z3, z2
        swap = kt
        A = (x2 + z2) % p
        AA = A * A % p
        B = (x2 - z2) % p
        BB = B * B % p
        E = (AA - BB) % p
        C = (x3 + z3) % p
        D = (x3 - z3) % p
        DA = D * A % p
        CB = C * B % p
        x3 = (DA + CB) ** 2 % p
        z3 = x1 * (DA - CB) ** 2 % p
        x2 = AA * BB % p
        z2 = E * (AA + X25519_A24 * E) % p
    if swap:
        x2, x3, z2, z3 = x3, x2, z3, z2
    return (x2 * pow(z2, p - 2, p) % p).to_bytes(32, "little")


def public_key(private: bytes) -> bytes:
    return x25519(private, X25519_BASE)


def private_key(seed: Optional[int], client: int) -> bytes:
    """A client's private key: 32 bytes of ``os.urandom``, or -- with a seed (tests) -- ``SHA-256(b"fd-secagg
    priv" + seed as 8 LE bytes + client as 4 LE bytes)``."""
    if seed is None:
        return os.urandom(32)
    if not 0 <= int(seed) < 1 << 64 or not 0 <= int(client) < 1 << 32:
        raise ValueError(f"secagg_seed in [0, 2^64) and client in [0, 2^32); got {seed!r}, {client!r}")
    return hashlib.sha256(b"fd-secagg priv" + int(seed).to_bytes(8, "little") + int(client).to_bytes(4, "little")).digest()


def pair_key(private: bytes, i: int, j: int, public: Dict[int, bytes]) -> np.ndarray:
    """``k_ij`` as client ``i`` computes it from its private key and the public keys: 8 words (uint32)."""
    if i == j:
        raise ValueError("a pair key joins two different clients")
    shared = x25519(private, public[j])
    if shared == bytes(32):
        raise ValueError(f"secure aggregation: the shared secret of clients {i + 1} and {j + 1} is all zero "
                         f"(a public key of small order): refused")
    lo, hi = min(i, j), max(i, j)
    mac = hmac.new(shared, b"fd-secagg v1" + public[lo] + public[hi], hashlib.sha256).digest()
    return np.frombuffer(mac, dtype="<u4").astype(np.uint32)


def gather_public_keys(mine: bytes, n_clients: int, comm=None, device=None) -> List[bytes]:
    """One all-gather of the ranks' 32-byte public keys, in rank order: over ``comm`` (a ``NativeComm``) when
    one is given, else over ``torch.distributed``.  The key travels as 8 int32 words -- the bytes of the
    uint8 tensor, in a dtype every communicator of the project carries (``NativeComm`` takes fp32, bf16,
    fp64, int64 and int32, no 8-bit type)."""
    import torch.distributed as dist
    if len(mine) != 32:
        raise ValueError("a public key holds 32 bytes")
    dev = torch.device(device) if device is not None else torch.device("cpu")
    words = torch.frombuffer(bytearray(mine), dtype=torch.uint8).clone().view(torch.int32).to(dev)
    if comm is not None:
        rows = comm.all_gather(words)
    else:
        rows = torch.empty((int(n_clients), 8), dtype=torch.int32, device=dev)
        if words.is_cuda:
            dist.all_gather_into_tensor(rows, words)
        else:
            dist.all_gather(list(rows.unbind(0)), words)
    if rows.dtype != torch.int32 or tuple(rows.shape) != (int(n_clients), 8):
        raise RuntimeError(f"secure aggregation: gathered {tuple(rows.shape)} {rows.dtype} key words, expected "
                           f"({int(n_clients)}, 8) int32")
    rows = rows.cpu().contiguous().view(torch.uint8)
    return [bytes(rows[c].tolist()) for c in range(int(n_clients))]


# ------------------------------------------------------------------ the specification
def _l2(x: torch.Tensor) -> float:
    with np.errstate(over="ignore"):
        return float(np.float32(math.sqrt(float(x.double().square().sum()))))


@torch.no_grad()
def torch_encode(w: torch.Tensor, anchor: torch.Tensor, frac_bits: int = 24) -> Tuple[torch.Tensor, Dict]:
    """The fixed-point codes of ``w - anchor`` (module docstring): ``(q int32 [n], stats)``, ``stats`` =
    ``{"update_l2", "error_l2", "clamped", "bad_elems"}``."""
    frac_bits, _ = _check_params(frac_bits, 20)
    if w.dtype != torch.float32 or anchor.dtype != torch.float32 or w.shape != anchor.shape or w.dim() != 1:
        raise ValueError("secagg encode takes flat fp32 tensors of one length")
    secagg_words(w.numel())
    dev = w.device
    scale = torch.tensor(2.0 ** frac_bits, dtype=torch.float32, device=dev)
    inv_scale = torch.tensor(2.0 ** -frac_bits, dtype=torch.float32, device=dev)
    d = w - anchor
    t = d * scale
    r = torch.round(t)
    bad = ~torch.isfinite(d)
    clamped = ~bad & ~(r.abs() < float(1 << 27))
    zero = torch.zeros((), dtype=torch.float32, device=dev)
    q = torch.where(bad | clamped, zero, r).to(torch.int32)
    q = torch.where(clamped, torch.where(r < 0, -QMAX, QMAX).to(torch.int32), q)
    back = q.to(torch.float32) * inv_scale
    err = d - back
    good = ~bad
    stats = {"update_l2": _l2(d[good]), "error_l2": _l2(err[good]), "clamped": int(clamped.sum()),
             "bad_elems": int(bad.sum())}
    return q, stats


def _signs_list(signs, P: int) -> List[int]:
    if isinstance(signs, (int, np.integer)):
        if not 0 <= int(signs) < 1 << P:
            raise ValueError(f"signs holds one bit per partner, got {signs!r} for {P}")
        return [-1 if (int(signs) >> p) & 1 else 1 for p in range(P)]
    out = [int(s) for s in signs]
    if len(out) != P or any(s not in (1, -1) for s in out):
        raise ValueError("signs: one of +1 / -1 per partner")
    return out


@torch.no_grad()
def torch_mask(q: torch.Tensor, keys, signs, round: int = 0, rounds: int = 20, first_block: int = 0) -> torch.Tensor:
    """The payload (int32, ``n + 16``) of the codes ``q``: ``uint32(q)`` and the check block's ones under the
    signed streams of the partners -- ``keys`` [P, 8] words, ``signs`` a bit mask (bit p set: -1) or a list of
    +1 / -1, nonce ``(round, 0, 0)`` -- modulo 2^32."""
    _check_params(24, rounds)
    if q.dtype != torch.int32 or q.dim() != 1:
        raise ValueError("secagg mask takes flat int32 codes")
    n = q.numel()
    words = secagg_words(n)
    if not 0 <= int(round) < 1 << 32:
        raise ValueError(f"secagg round in [0, 2^32), got {round}")
    _blocks_check(first_block, n, 1)
    keys = np.asarray(keys, dtype=np.uint64).reshape(-1, 8)
    P = keys.shape[0]
    if P > MAX_CLIENTS - 1:
        raise ValueError(f"secure aggregation takes at most {MAX_CLIENTS - 1} partners, got {P}")
    sg = _signs_list(signs, P)
    y = np.empty(words, dtype=np.uint32)
    y[:n] = q.cpu().numpy().view(np.uint32)
    y[n:] = 1
    for p in range(P):
        x = stream_words(keys[p], (int(round), 0, 0), words, first_block, rounds)
        y = y + x if sg[p] > 0 else y - x  # (uint32 arrays wrap)
    return torch.from_numpy(y.view(np.int32).copy()).to(q.device)


def check_block_sum(payloads: Sequence[torch.Tensor]) -> torch.Tensor:
    """The 16 words of the payloads' check blocks, summed modulo 2^32 (int64)."""
    tail = torch.stack([p[-CHECK_WORDS:] for p in payloads]).to(torch.int64)
    return tail.sum(dim=0) & 0xFFFFFFFF


@torch.no_grad()
def torch_unmask_mean_(payloads: Sequence[torch.Tensor], anchor: torch.Tensor, out: torch.Tensor,
                       shadow: Optional[torch.Tensor], frac_bits: int = 24) -> None:
    """The specification of the unmask pass in torch: ``out = anchor + (float32(int32(sum of the payloads mod
    2^32)) * 2^-f) * float32(1 / M)``, ``shadow`` (optional) = bf16(out).  The check block is not looked at."""
    frac_bits, _ = _check_params(frac_bits, 20)
    M = len(payloads)
    if not 1 <= M <= MAX_CLIENTS:
        raise ValueError(f"unmask_mean takes 1 .. {MAX_CLIENTS} payloads, got {M}")
    if anchor.dtype != torch.float32 or out.dtype != torch.float32 or anchor.shape != out.shape or out.dim() != 1:
        raise ValueError("unmask_mean takes flat fp32 anchor and out of one length")
    n, dev = out.numel(), out.device
    words = secagg_words(n)
    s = torch.zeros(n, dtype=torch.int64, device=dev)
    for p in payloads:
        if p.dtype != torch.int32 or p.dim() != 1 or p.numel() != words:
            raise ValueError(f"a payload of {n} elements is a flat int32 tensor of {words} words, got "
                             f"{tuple(p.shape)} {p.dtype}")
        s = s + (p[:n].to(dev).to(torch.int64) & 0xFFFFFFFF)
    s = s & 0xFFFFFFFF
    s = torch.where(s >= 1 << 31, s - (1 << 32), s).to(torch.int32)
    acc = s.to(torch.float32)
    inv_scale = torch.tensor(2.0 ** -frac_bits, dtype=torch.float32, device=dev)
    inv = torch.tensor(float(np.float32(1.0 / M)), dtype=torch.float32, device=dev)
    out.copy_(anchor + (acc * inv_scale) * inv)
    if shadow is not None:
        shadow.copy_(out)


# ------------------------------------------------------------------ the job's object
class SecureAggregator:
    """The secure aggregation of a job: ``frac_bits`` fraction bits, ChaCha with ``rounds`` rounds, the key
    pairs of the clients this process holds (one in a rank of a collective job, all of them in a
    virtual-client job) and every client's public key.  ``last`` holds the latest ``mask_``'s report:
    ``{"update_l2", "error_l2", "clamped", "bad_elems", "payload_bytes", "masked_with"}``."""

    def __init__(self, frac_bits: int = 24, rounds: int = 20, seed: Optional[int] = None,
                 log: Optional[Callable[[str], None]] = None):
        self.frac_bits, self.rounds = _check_params(frac_bits, rounds)
        if seed is not None and not 0 <= int(seed) < 1 << 64:
            raise ValueError(f"secagg_seed must lie in [0, 2^64), got {seed!r}")
        self.seed = None if seed is None else int(seed)
        self.log = log or logging.getLogger(__name__).warning
        self.private: Dict[int, bytes] = {}
        self.public: Dict[int, bytes] = {}
        self.n_clients = 0
        self.last: Optional[Dict] = None
        self.last_round: Optional[int] = None
        self._pair: Dict[Tuple[int, int], np.ndarray] = {}
        self._dev_keys: Dict = {}
        self._work = None  # (device, partial, stats)
        self._warned_two = False

    def describe(self) -> str:
        return f"{self.frac_bits} fraction bits, ChaCha{self.rounds}"

    def words(self, n: int) -> int:
        return secagg_words(n)

    def setup_keys(self, clients, n_clients: int, comm=None, device=None) -> None:
        """Draw the key pairs of ``clients`` (an index or several: the clients this process holds) and
        learn every client's public key, then derive the pair keys of the held clients (the X25519
        ladders run here, not inside a round's exchange).  A process that holds all ``n_clients`` gathers
        nothing; otherwise the 32-byte public keys are all-gathered once (one client per rank, in rank
        order) over ``comm`` (a ``NativeComm``, for a CUDA ``device``) or ``torch.distributed`` -- as 8
        int32 words, a dtype every communicator of the project carries; the bytes are those of the uint8
        tensor."""
        import torch.distributed as dist
        own = [int(clients)] if isinstance(clients, (int, np.integer)) else [int(c) for c in clients]
        n_clients = int(n_clients)
        if not 1 <= n_clients <= MAX_CLIENTS:
            raise ValueError(f"secure aggregation takes 1 .. {MAX_CLIENTS} clients, got {n_clients}")
        if not own or any(not 0 <= c < n_clients for c in own) or len(set(own)) != len(own):
            raise ValueError(f"secure aggregation: client indices in [0, {n_clients}), got {own}")
        self.private = {c: private_key(self.seed, c) for c in own}
        self.public = {c: public_key(sk) for c, sk in self.private.items()}
        self.n_clients = n_clients
        self._pair.clear()
        self._dev_keys.clear()
        if len(own) == n_clients:
            self._derive_pair_keys()
            return
        if len(own) != 1 or not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() != n_clients:
            raise RuntimeError("secure aggregation: the public keys are exchanged one client per rank")
        if dist.get_rank() != own[0]:
            raise RuntimeError(f"secure aggregation: rank {dist.get_rank()} holds client {own[0]}")
        for c, pk in enumerate(gather_public_keys(self.public[own[0]], n_clients, comm, device)):
            if c == own[0] and pk != self.public[c]:
                raise RuntimeError("secure aggregation: the gathered public keys are out of order")
            self.public[c] = pk
        self._derive_pair_keys()

    def _derive_pair_keys(self) -> None:
        for i in self.private:
            for j in range(self.n_clients):
                if j != i:
                    self.pair_words(i, j)

    def pair_words(self, i: int, j: int) -> np.ndarray:
        """``k_ij`` as client ``i`` (held by this process) computes it: 8 words."""
        i, j = int(i), int(j)
        if i not in self.private or j not in self.public:
            raise RuntimeError(f"secure aggregation: no keys for the pair ({i + 1}, {j + 1}); call setup_keys")
        k = self._pair.get((i, j))
        if k is None:
            k = self._pair[(i, j)] = pair_key(self.private[i], i, j, self.public)
        return k

    def partners(self, client: int, live: Sequence[int]) -> List[int]:
        live = [int(c) for c in live]
        if int(client) not in live:
            raise ValueError(f"client {client} masks for a live set it is not in: {live}")
        if len(set(live)) != len(live) or len(live) > MAX_CLIENTS:
            raise ValueError(f"secure aggregation takes 1 .. {MAX_CLIENTS} distinct live clients, got {live}")
        return [j for j in live if j != int(client)]

    @torch.no_grad()
    def mask_(self, master: torch.Tensor, anchor: torch.Tensor, client: int, round: int,
              live: Sequence[int]) -> torch.Tensor:
        """The payload of ``master - anchor`` for the round's ``live`` clients (``client`` among them): its
        fixed-point codes and the check block under the streams of the live partners.  On CUDA one
        ``secagg_mask`` call; on the CPU the specification."""
        client = int(client)
        partners = self.partners(client, live)
        P = len(partners)
        if len(live) == 2 and not self._warned_two:
            self._warned_two = True
            self.log("[WARN] secure aggregation with two live clients: the sum reveals each update to the other")
        keys = np.stack([self.pair_words(client, j) for j in partners]) if P else np.zeros((0, 8), dtype=np.uint32)
        signs = sum(1 << p for p, j in enumerate(partners) if client > j)
        n = master.numel()
        words = secagg_words(n)
        if master.is_cuda:
            from ..ops import kernels as K
            grid = K.secagg_grid(n)
            if self._work is None or self._work[0] != master.device or self._work[1].numel() < 4 * grid:
                self._work = (master.device, torch.empty(4 * grid, dtype=torch.float64, device=master.device),
                              torch.empty(4, dtype=torch.float64, device=master.device))
            _, partial, stats = self._work
            ck = (client, tuple(partners), str(master.device))
            dk = self._dev_keys.get(ck)
            if dk is None:
                self._dev_keys.clear()
                dk = self._dev_keys[ck] = torch.from_numpy(keys.view(np.int32).copy()).reshape(P, 8).to(master.device)
            payload = torch.empty(words, dtype=torch.int32, device=master.device)
            K.secagg_mask(master, anchor, dk, signs, payload, partial, stats, self.frac_bits, self.rounds, int(round))
            up, er, cl, bad = stats.tolist()
            rep = {"update_l2": float(up), "error_l2": float(er), "clamped": int(cl), "bad_elems": int(bad)}
        else:
            q, rep = torch_encode(master, anchor, self.frac_bits)
            payload = torch_mask(q, keys, signs, int(round), self.rounds)
        rep.update(payload_bytes=4 * words, masked_with=P)
        self.last = rep
        self.last_round = int(round)
        return payload

    @torch.no_grad()
    def unmask_mean_(self, model, payloads: Sequence[torch.Tensor], anchor: torch.Tensor, server=None,
                     round: Optional[int] = None) -> None:
        """The model's master (and bf16 shadow) become ``anchor`` plus the fixed-point mean of the M =
        len(payloads) live clients' updates, from the modular sum of their payloads.  First the summed
        check block must hold ``M`` in all 16 words: otherwise the live sets or the keys disagreed, and a
        ``RuntimeError`` names the round and leaves the master untouched.  With a server optimizer the mean
        is unmasked into the master without a shadow and ``server.apply_(model, 1.0)`` makes its step."""
        A = model.arena
        M = len(payloads)
        if not 1 <= M <= MAX_CLIENTS:
            raise ValueError(f"secure aggregation takes 1 .. {MAX_CLIENTS} participating clients, got {M}")
        words = secagg_words(A.master.numel())
        for p in payloads:
            if p.dtype != torch.int32 or p.dim() != 1 or p.numel() != words:
                raise ValueError(f"a secure-aggregation payload of this model is a flat int32 tensor of {words} "
                                 f"words, got {tuple(p.shape)} {p.dtype}")
        r = self.last_round if round is None else int(round)
        chk = check_block_sum(payloads)
        if not bool((chk == M).all()):
            raise RuntimeError(f"secure aggregation, round {'?' if r is None else r + 1}: the check block of the {M} summed "
                               f"payloads does not hold {M} -- the clients masked for different live sets or "
                               f"with different keys; the model is left as it was")
        if A.master.is_cuda:
            from ..ops import kernels as K
            shadow = A.shadow if server is None else None
            K.secagg_unmask_mean(list(payloads), anchor, A.master, shadow, self.frac_bits)
            if server is None:
                if shadow is not None:
                    model.mark_shadow_synced()
                else:
                    model.sync_shadow(force=True)
        else:
            torch_unmask_mean_(list(payloads), anchor, A.master, None, self.frac_bits)
            if server is None:
                model.sync_shadow(force=True)
        if server is not None:
            server.apply_(model, 1.0)


def check_secagg_config(cfg, gpus_per_client: int = 1, n_clients: Optional[int] = None) -> bool:
    """Whether the configuration asks for secure aggregation (``secagg=True``), or a ValueError naming the
    flag for a value or a combination it does not run with.  Needs no model: callers refuse a bad
    configuration before any work."""
    on = getattr(cfg, "secagg", False)
    if not isinstance(on, (bool, np.bool_)):
        raise ValueError(f"secagg must be a bool, got {on!r}")
    _check_params(getattr(cfg, "secagg_frac_bits", 24), getattr(cfg, "secagg_chacha_rounds", 20))
    seed = getattr(cfg, "secagg_seed", None)
    if seed is not None and not 0 <= int(seed) < 1 << 64:
        raise ValueError(f"secagg_seed must lie in [0, 2^64), got {seed!r}")
    if not on:
        return False
    if getattr(cfg, "transport", "collective") == "tcp":
        raise ValueError("secagg needs transport='collective': the reference-compatible TCP server takes fp32 state "
                         "dicts in the clear")
    if str(getattr(cfg, "aggregator", "mean")).lower() != "mean":
        raise ValueError("secagg needs aggregator='mean': a robust aggregate takes order statistics of the individual "
                         "updates, which secure aggregation exists to hide")
    if str(getattr(cfg, "compress", "none")).lower() != "none":
        raise ValueError("secagg needs compress='none': the masks cover 32-bit fixed-point words, not codes with "
                         "per-group scales")
    if getattr(cfg, "weighted_fedavg", False):
        raise ValueError("secagg does not take weighted_fedavg=True: the unmasked mean is unweighted")
    if int(gpus_per_client) > 1:
        raise ValueError("secagg needs gpus_per_client=1: a client's replicas would each draw a key pair")
    if n_clients is not None and int(n_clients) > MAX_CLIENTS:
        raise ValueError(f"secagg takes at most {MAX_CLIENTS} participating clients (their 2^27-bounded codes add "
                         f"inside int32), got {n_clients}")
    return True


def make_secagg(cfg, gpus_per_client: int = 1, n_clients: Optional[int] = None, log=None) -> Optional[SecureAggregator]:
    """The configuration's ``SecureAggregator`` (``--secagg true``), or None when ``secagg`` is off (today's
    path, untouched).  Its keys are drawn by ``setup_keys``."""
    if not check_secagg_config(cfg, gpus_per_client, n_clients):
        return None
    return SecureAggregator(int(cfg.secagg_frac_bits), int(cfg.secagg_chacha_rounds), getattr(cfg, "secagg_seed", None),
                            log=log)
