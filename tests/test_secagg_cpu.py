"""Secure aggregation on the CPU (parallel/secagg.py: fixed-point updates under pairwise ChaCha masks):
the ChaCha and X25519 known answers, the generator against a scalar loop, the pair keys, the torch
specification against a hand-written per-element loop on a crafted vector, exact cancellation, the
check block, that a payload is not its plaintext, the arena pads, the error bound of the unmasked mean,
the configuration plumbing and its refusals, the untouched default path, the virtual run against the
2-rank gloo run bit for bit, the public-key exchange through a communicator with ``NativeComm``'s dtype
set, a dropped client, and the composition with client-level privacy and with
a server optimizer."""
import argparse
import math
import os
import re
import socket
import types

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

PKG = "detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd"

from importlib import import_module  # noqa: E402

config = import_module(f"{PKG}.config")
data_pkg = import_module(f"{PKG}.data")
models = import_module(f"{PKG}.models")
runner = import_module(f"{PKG}.fed.runner")
fedavg = import_module(f"{PKG}.parallel.fedavg")
sa = import_module(f"{PKG}.parallel.secagg")

SEED = 0x5EEDF00DCAFE
F = 24
SECAGG_KEYS = ("payload_bytes", "update_l2", "quant_error_l2", "clamped", "bad_elems", "masked_with")
RFC_KEY = np.frombuffer(bytes(range(32)), dtype="<u4")
RFC_NONCE = (0x09000000, 0x4A000000, 0)
RFC_WORDS = [0xE4E7F110, 0x15593BD1, 0x1FDD0F50, 0xC47120A3, 0xC7F4D1C7, 0x0368C033, 0x9AAA2204, 0x4E6CD4C3,
             0x466482D2, 0x09AA9F07, 0x05D7C214, 0xA2028BD9, 0xD19C12B5, 0xB94E16DE, 0xE883D0CB, 0x4E3C50A2]
NO_KEYS = np.zeros((0, 8), dtype=np.uint32)


@pytest.fixture(autouse=True)
def _cpu_only(monkeypatch):
    """Everything here is compared with CPU results bit for bit (the gloo ranks run on the CPU): on a
    machine that has a GPU the jobs of this file still choose the CPU."""
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _clear_rank_env():
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        os.environ.pop(k, None)


def _single_thread(fn):
    nthreads = torch.get_num_threads()
    torch.set_num_threads(1)  # (CPU GEMM reductions split by thread count: same count on both sides)
    try:
        return fn()
    finally:
        torch.set_num_threads(nthreads)


def _bits(t):
    return t.contiguous().view(torch.int32).tolist()


def _vectors(n, seed, scale=0.01):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(n, generator=g)
    w = a + scale * torch.randn(n, generator=g) * torch.rand(n, generator=g)
    return w, a


# ------------------------------------------------------------------ 1. ChaCha
def _scalar_chacha(key, counter, nonce, rounds):
    """The block function in Python integers, straight from RFC 8439 section 2.3."""
    def rotl(x, k):
        return ((x << k) | (x >> (32 - k))) & 0xFFFFFFFF

    def qr(s, a, b, c, d):
        s[a] = (s[a] + s[b]) & 0xFFFFFFFF
        s[d] = rotl(s[d] ^ s[a], 16)
        s[c] = (s[c] + s[d]) & 0xFFFFFFFF
        s[b] = rotl(s[b] ^ s[c], 12)
        s[a] = (s[a] + s[b]) & 0xFFFFFFFF
        s[d] = rotl(s[d] ^ s[a], 8)
        s[c] = (s[c] + s[d]) & 0xFFFFFFFF
        s[b] = rotl(s[b] ^ s[c], 7)

    init = [0x61707865, 0x3320646E, 0x79622D32, 0x6B206574] + [int(k) for k in key] + [int(counter)] + [int(v) for v in nonce]
    s = list(init)
    for _ in range(rounds // 2):
        for a, b, c, d in ((0, 4, 8, 12), (1, 5, 9, 13), (2, 6, 10, 14), (3, 7, 11, 15),
                           (0, 5, 10, 15), (1, 6, 11, 12), (2, 7, 8, 13), (3, 4, 9, 14)):
            qr(s, a, b, c, d)
    return [(x + y) & 0xFFFFFFFF for x, y in zip(s, init)]


def test_chacha_known_answer_and_scalar_loop():
    got = sa.chacha_block(RFC_KEY, 1, RFC_NONCE, 20)
    assert [int(x) for x in got] == RFC_WORDS == _scalar_chacha(RFC_KEY, 1, RFC_NONCE, 20)
    rng = np.random.default_rng(3)
    key = rng.integers(0, 1 << 32, size=8, dtype=np.uint64)
    nonce = (5, 0xFFFFFFFF, 0x80000000)
    ctrs = np.array([0, 1, 77, (1 << 32) - 1], dtype=np.uint64)
    for rounds in (8, 12, 20):
        blocks = sa.chacha_block(key, ctrs, nonce, rounds)
        assert blocks.shape == (4, 16)
        for i, c in enumerate(ctrs):
            assert [int(x) for x in blocks[i]] == _scalar_chacha(key, int(c), nonce, rounds), (rounds, int(c))
    assert not np.array_equal(sa.chacha_block(key, 0, nonce, 8), sa.chacha_block(key, 0, nonce, 12))
    # the stream: block b covers elements 16 b .. 16 b + 15, element e takes RFC word 4 (e % 4) + e // 4
    assert sa.WORD_ORDER == tuple(4 * (e % 4) + e // 4 for e in range(16)) and sorted(sa.WORD_ORDER) == list(range(16))
    words = sa.stream_words(key, nonce, 48, first_block=76, rounds=12)
    for b in range(3):
        blk = _scalar_chacha(key, 76 + b, nonce, 12)
        assert [int(x) for x in words[16 * b:16 * b + 16]] == [blk[sa.WORD_ORDER[e]] for e in range(16)]
    assert np.array_equal(sa.stream_words(key, nonce, 16, (1 << 32) - 1, 8),
                          np.array([_scalar_chacha(key, (1 << 32) - 1, nonce, 8)[k] for k in sa.WORD_ORDER], dtype=np.uint32))
    for bad in (dict(rounds=10), dict(key8=key[:7]), dict(nonce3=(1, 2)), dict(counter=1 << 32), dict(nonce3=(1, 2, 1 << 32))):
        with pytest.raises(ValueError):
            sa.chacha_block(**dict(dict(key8=key, counter=0, nonce3=nonce, rounds=20), **bad))
    for args in ((key, nonce, 24), (key, nonce, 0), (key, nonce, 32, (1 << 32) - 1), (key, nonce, 16, -1)):
        with pytest.raises(ValueError):
            sa.stream_words(*args)


# ------------------------------------------------------------------ 2. X25519 and the pair keys
def test_x25519_known_answer_and_commutation():
    sk = bytes.fromhex("77076d0a7318a57d3c16c17251b26645df4c2f87ebc0992ab177fba51db92c2a")
    assert sa.public_key(sk).hex() == "8520f0098930a754748b7ddcb43ef75a0dbf3a0d26381af4eba4a98eaa9b4e6a"
    # RFC 7748 section 5.2, the first test vector (a u-coordinate that is not the base point)
    k = bytes.fromhex("a546e36bf0527c9d3b16154b82465edd62144c0ac1fc5a18506a2244ba449ac4")
    u = bytes.fromhex("e6db6867583030db3594c1a424b15f7c726624ec26b3353b10a903a6d0ab1c4c")
    assert sa.x25519(k, u).hex() == "c3da55379de9c6908e94ea4df28d084f32eccf03491c71f754b4075577a28552"
    rng = np.random.default_rng(9)
    for _ in range(3):
        a, b = bytes(rng.integers(0, 256, 32, dtype=np.uint8)), bytes(rng.integers(0, 256, 32, dtype=np.uint8))
        assert sa.x25519(a, sa.x25519(b, sa.X25519_BASE)) == sa.x25519(b, sa.x25519(a, sa.X25519_BASE))
    top = bytearray(u)
    top[31] |= 0x80                                                       # the top bit of u is masked
    assert sa.x25519(k, bytes(top)) == sa.x25519(k, u)
    with pytest.raises(ValueError):
        sa.x25519(k[:31], u)


def test_pair_keys():
    agg = sa.SecureAggregator(seed=SEED)
    agg.setup_keys(range(4), 4)
    for i in range(4):
        assert agg.private[i] == sa.private_key(SEED, i) and agg.public[i] == sa.public_key(agg.private[i])
        for j in range(4):
            if i != j:
                kij, kji = agg.pair_words(i, j), agg.pair_words(j, i)
                assert kij.dtype == np.uint32 and kij.shape == (8,) and np.array_equal(kij, kji)      # k_ij == k_ji
    assert len({agg.pair_words(i, j).tobytes() for i in range(4) for j in range(i + 1, 4)}) == 6
    import hashlib
    import hmac
    shared = sa.x25519(agg.private[2], agg.public[1])
    mac = hmac.new(shared, b"fd-secagg v1" + agg.public[1] + agg.public[2], hashlib.sha256).digest()
    assert agg.pair_words(2, 1).tolist() == [int.from_bytes(mac[4 * k:4 * k + 4], "little") for k in range(8)]
    assert sa.private_key(SEED, 3) == hashlib.sha256(b"fd-secagg priv" + SEED.to_bytes(8, "little") + (3).to_bytes(4, "little")).digest()
    # without a seed: 32 fresh bytes per client and per call
    r1, r2 = sa.SecureAggregator(), sa.SecureAggregator()
    r1.setup_keys(range(2), 2)
    r2.setup_keys(range(2), 2)
    assert len({r1.private[0], r1.private[1], r2.private[0], r2.private[1]}) == 4
    old = r1.private[0]
    r1.setup_keys(range(2), 2)                                            # (a restart draws again)
    assert r1.private[0] != old
    # an all-zero shared secret (a public key of small order) is refused
    agg.public[3] = bytes(32)
    agg._pair.clear()
    with pytest.raises(ValueError, match="all zero"):
        agg.pair_words(0, 3)
    with pytest.raises(RuntimeError, match="setup_keys"):
        sa.SecureAggregator().pair_words(0, 1)
    for args in (([0, 0], 2), ([2], 2), ([], 2), (range(17), 17), ([0], 0)):
        with pytest.raises(ValueError):
            sa.SecureAggregator(seed=1).setup_keys(*args)
    with pytest.raises(RuntimeError, match="one client per rank"):
        sa.SecureAggregator(seed=1).setup_keys(0, 2)                      # (no process group to gather over)


# ------------------------------------------------------------------ 3. the specification against a loop
def _loop_encode(w, a, f):
    q, clamped, bad, sd, se = [], 0, 0, 0.0, 0.0
    scale, inv_scale = np.float32(2.0 ** f), np.float32(2.0 ** -f)
    with np.errstate(all="ignore"):
        for x, y in zip(w.numpy(), a.numpy()):
            d = np.float32(x - y)
            if not np.isfinite(d):
                q.append(0)
                bad += 1
                continue
            t = np.float32(d * scale)
            r = np.float32(np.rint(t))                                    # ties to even
            if not abs(r) < np.float32(2.0 ** 27):
                q.append(-sa.QMAX if r < 0 else sa.QMAX)
                clamped += 1
            else:
                q.append(int(r))
            back = np.float32(np.float32(q[-1]) * inv_scale)
            e = np.float32(d - back)
            sd += float(d) ** 2
            se += float(e) ** 2
        return q, clamped, bad, float(np.float32(math.sqrt(sd))), float(np.float32(math.sqrt(se)))


def _crafted(f):
    u = 2.0 ** -f
    edge = 2.0 ** (27 - f)                                                # 2^27 steps
    below = float(np.nextafter(np.float32(edge), np.float32(0.0)))
    vals = [0.0, -0.0, 0.5 * u, 1.5 * u, 2.5 * u, -0.5 * u, -1.5 * u, below, -below, edge, -edge, 3e38, -1e38,
            float("inf"), float("-inf"), float("nan"), 1e-40, -1e-40, 1.0 * u * 4096, -0.25 * edge]
    n = 32
    w, a = torch.zeros(n), torch.zeros(n)
    w[:len(vals)] = torch.tensor(vals)
    w[30], a[30] = 3e38, -3e38                                            # w - anchor overflows: d = inf
    w[31], a[31] = 1.5 * edge / 8, 1.25 * edge / 8                        # an ordinary element with an anchor: 2^22 steps
    return w, a, len(vals)


@pytest.mark.parametrize("f", [8, 24, 30])
def test_specification_against_a_loop(f):
    for w, a in (_vectors(256, seed=f, scale=2.0 ** (10 - f) * 50), _crafted(f)[:2]):
        q, rep = sa.torch_encode(w, a, f)
        lq, lc, lb, lup, ler = _loop_encode(w, a, f)
        assert q.dtype == torch.int32 and q.tolist() == lq
        assert rep["clamped"] == lc and rep["bad_elems"] == lb
        assert abs(rep["update_l2"] - lup) <= 2.0 ** -23 * lup and abs(rep["error_l2"] - ler) <= 2.0 ** -23 * ler
    w, a, nv = _crafted(f)
    q, rep = sa.torch_encode(w, a, f)
    top = (1 << 27) - (1 << 3)                                            # one fp32 ulp below 2^27
    assert q[:13].tolist() == [0, 0, 0, 2, 2, 0, -2, top, -top, sa.QMAX, -sa.QMAX, sa.QMAX, -sa.QMAX]
    assert q[13:18].tolist() == [0, 0, 0, 0, 0] and q[18:20].tolist() == [4096, -(1 << 25)] and q[30] == 0
    assert q[31] == 1 << 22 and rep["clamped"] == 4 and rep["bad_elems"] == 4
    assert math.isfinite(rep["update_l2"]) and rep["update_l2"] > 3e38 and rep["error_l2"] > 3e38


def _loop_mask(q, keys, signs, rnd, rounds, first_block=0):
    y = [int(v) & 0xFFFFFFFF for v in q] + [1] * 16
    for p, key in enumerate(keys):
        for i in range(len(y)):
            word = _scalar_chacha(key, first_block + i // 16, (rnd, 0, 0), rounds)[sa.WORD_ORDER[i % 16]]
            y[i] = (y[i] + (word if signs[p] > 0 else -word)) & 0xFFFFFFFF
    return [v - (1 << 32) if v >= 1 << 31 else v for v in y]


def test_mask_and_unmask_against_a_loop():
    w, a = _vectors(32, seed=2)
    q, _ = sa.torch_encode(w, a, F)
    keys = np.random.default_rng(1).integers(0, 1 << 32, size=(3, 8), dtype=np.uint64)
    payload = sa.torch_mask(q, keys, 0b010, round=9, rounds=8, first_block=5)
    assert payload.dtype == torch.int32 and payload.numel() == 48 == sa.secagg_words(32)
    assert payload.tolist() == _loop_mask(q.tolist(), keys, [1, -1, 1], 9, 8, 5)
    assert torch.equal(payload, sa.torch_mask(q, keys, [1, -1, 1], 9, 8, 5))
    assert torch.equal(sa.torch_mask(q, NO_KEYS, 0), torch.cat([q, torch.ones(16, dtype=torch.int32)]))
    # unmask, by hand: two plain payloads whose codes wrap through 2^32 on the way
    p1 = sa.torch_mask(q, keys[:1], 0, 1, 8)
    p2 = sa.torch_mask(-2 * q, keys[:1], 1, 1, 8)
    out, sh = torch.empty(32), torch.empty(32, dtype=torch.bfloat16)
    sa.torch_unmask_mean_([p1, p2], a, out, sh, F)
    want = [float(np.float32(np.float32(y) + np.float32(np.float32(np.float32(-int(v)) * np.float32(2.0 ** -F)) * np.float32(0.5))))
            for y, v in zip(a.numpy(), q.tolist())]
    assert out.tolist() == want and torch.equal(sh, out.to(torch.bfloat16))
    for args in (([], a, out, None, F), ([p1] * 17, a, out, None, F), ([p1[:-1]], a, out, None, F),
                 ([p1.float()], a, out, None, F), ([p1], a.double(), out, None, F), ([p1], a, out, None, 7)):
        with pytest.raises(ValueError):
            sa.torch_unmask_mean_(*args)
    for kw in (dict(round=-1), dict(round=1 << 32), dict(rounds=10), dict(first_block=-1), dict(first_block=(1 << 32) - 2),
               dict(signs=8), dict(signs=[1, 1]), dict(signs=[1, 0, 1]), dict(keys=np.zeros((16, 8)), signs=0)):
        with pytest.raises(ValueError):
            sa.torch_mask(**dict(dict(q=q, keys=keys, signs=0, round=0, rounds=20, first_block=0), **kw))
    for args in ((w, a[:16], F), (w.double(), a.double(), F), (w[:24], a[:24], F), (w, a, 31), (w, a, 7), (w, a, 24.5)):
        with pytest.raises(ValueError):
            sa.torch_encode(*args)


# ------------------------------------------------------------------ 4. cancellation, the check block, privacy of a payload
def _clients(M, n=2048, seed=0):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(n, generator=g)
    a[:64] = 0.0                                                          # an arena pad
    ws = []
    for c in range(M):
        w = a + 0.01 * (c + 1) * torch.randn(n, generator=g)
        w[:64] = 0.0
        ws.append(w)
    return ws, a


def _model(master):
    return types.SimpleNamespace(arena=types.SimpleNamespace(master=master, shadow=None),
                                 sync_shadow=lambda force=False: None)


@pytest.mark.parametrize("M", [1, 2, 3, 8, 16])
def test_the_masks_cancel_exactly(M):
    ws, a = _clients(M, n=256, seed=M)
    lines = []
    agg = sa.SecureAggregator(F, 8, seed=SEED, log=lines.append)
    agg.setup_keys(range(M), M)
    qs = [sa.torch_encode(w, a, F)[0] for w in ws]
    ps = [agg.mask_(ws[c], a, c, 3, range(M)) for c in range(M)]
    assert agg.last["masked_with"] == M - 1 and agg.last["payload_bytes"] == 4 * (256 + 16)
    s = sum(p.to(torch.int64) for p in ps) & 0xFFFFFFFF
    s = torch.where(s >= 1 << 31, s - (1 << 32), s)
    assert torch.equal(s[:256], sum(q.to(torch.int64) for q in qs)) and s[256:].tolist() == [M] * 16
    assert sa.check_block_sum(ps).tolist() == [M] * 16
    model, plain = _model(ws[0].clone()), _model(ws[0].clone())
    agg.unmask_mean_(model, ps, a, round=3)
    sa.torch_unmask_mean_([sa.torch_mask(q, NO_KEYS, 0) for q in qs], a, plain.arena.master, None, F)
    assert _bits(model.arena.master) == _bits(plain.arena.master)        # equal to the unmasked quantized mean
    assert (len(lines) == 1 and "two live clients" in lines[0]) if M == 2 else not lines
    if M >= 2:                                                            # any partial sum is still masked
        part = sum(p.to(torch.int64) for p in ps[:-1]) & 0xFFFFFFFF
        want = sum(q.to(torch.int64) for q in qs[:-1]) & 0xFFFFFFFF
        assert int((part[:256] == want).sum()) <= 2


def test_a_live_subset_and_a_disagreeing_client():
    M = 5
    ws, a = _clients(M, n=256, seed=1)
    agg = sa.SecureAggregator(F, 12, seed=SEED)
    agg.setup_keys(range(M), M)
    live = [0, 2, 3]
    ps = [agg.mask_(ws[c], a, c, 0, live) for c in live]
    assert agg.last["masked_with"] == 2
    model = _model(ws[0].clone())
    agg.unmask_mean_(model, ps, a)
    want = torch.empty(256)
    sa.torch_unmask_mean_([sa.torch_mask(sa.torch_encode(ws[c], a, F)[0], NO_KEYS, 0) for c in live], a, want, None, F)
    assert _bits(model.arena.master) == _bits(want)
    # client 3 masks for another live set: the check block fails, the round is named, the master stays
    before = ws[1].clone()
    model = _model(before.clone())
    bad = [agg.mask_(ws[0], a, 0, 6, live), agg.mask_(ws[2], a, 2, 6, live), agg.mask_(ws[3], a, 3, 6, [0, 2, 3, 4])]
    with pytest.raises(RuntimeError, match="round 7"):
        agg.unmask_mean_(model, bad, a)
    assert _bits(model.arena.master) == _bits(before)
    # ... as it does when a payload is left out, when the rounds differ, and when the keys differ
    for ps in ([agg.mask_(ws[c], a, c, 6, live) for c in live[:2]],
               [agg.mask_(ws[0], a, 0, 6, live), agg.mask_(ws[2], a, 2, 6, live), agg.mask_(ws[3], a, 3, 5, live)]):
        with pytest.raises(RuntimeError, match="check block"):
            agg.unmask_mean_(model, ps, a, round=6)
    other = sa.SecureAggregator(F, 12, seed=SEED + 1)
    other.setup_keys(range(M), M)
    with pytest.raises(RuntimeError, match="check block"):
        agg.unmask_mean_(model, [agg.mask_(ws[0], a, 0, 6, [0, 2]), other.mask_(ws[2], a, 2, 6, [0, 2])], a, round=6)
    assert _bits(model.arena.master) == _bits(before)
    for kw in (dict(client=1), dict(live=[0, 0, 2]), dict(live=list(range(17)))):
        with pytest.raises(ValueError):
            agg.mask_(**dict(dict(master=ws[0], anchor=a, client=0, round=0, live=live), **kw))
    with pytest.raises(ValueError):
        agg.unmask_mean_(model, [], a)
    with pytest.raises(ValueError):
        agg.unmask_mean_(model, [ps[0][:-1]], a)


def test_a_payload_is_not_its_plaintext_and_pads_stay_zero():
    n = 2048
    ws, a = _clients(3, n=n, seed=4)
    for rounds in (8, 12, 20):
        agg = sa.SecureAggregator(F, rounds, seed=SEED)
        agg.setup_keys(range(3), 3)
        ps = [agg.mask_(ws[c], a, c, 1, range(3)) for c in range(3)]
        for c in range(3):
            q, _ = sa.torch_encode(ws[c], a, F)
            assert not q[:64].any()                                       # the pad's code is 0 ...
            assert int((ps[c][:n] == q).sum()) <= n // 100                # ... and at most 1 % of the words show q
            assert int((ps[c][n:] == 1).sum()) <= 1
        model = _model(ws[0].clone())
        agg.unmask_mean_(model, ps, a)
        assert not model.arena.master[:64].view(torch.int32).any()        # +0, not -0


def test_error_bound_of_the_unmasked_mean():
    """out against the mean of the fp32 inputs taken in fp64.  Per element: d_c = fl(w_c - a) is off by at
    most 2^-24 |d_c|; every unclamped code is off by at most half a step, 2^-(f+1), and so is their mean;
    the sum of the codes is an exact integer and float32() of it, the product with float32(1 / M) (itself
    off by 2^-24 relative) and its rounding cost 2^-24 |mean d| each; the final add costs 2^-24 |out|:
    |out - mean| <= 2^-(f+1) + 2^-24 (4 max|d| + max|out|)."""
    for M, f, scale in ((3, 24, 0.01), (16, 24, 0.01), (8, 16, 0.01), (2, 30, 1e-4), (5, 8, 0.5)):
        g = torch.Generator().manual_seed(M)
        a = torch.randn(4096, generator=g)
        ws = [a + scale * torch.randn(4096, generator=g) for _ in range(M)]
        agg = sa.SecureAggregator(f, 8, seed=1)
        agg.setup_keys(range(M), M)
        ps = []
        for c in range(M):
            ps.append(agg.mask_(ws[c], a, c, 0, range(M)))
            assert agg.last["clamped"] == 0 and agg.last["error_l2"] <= 2.0 ** -(f + 1) * math.sqrt(4096)
        model = _model(torch.empty(4096))
        agg.unmask_mean_(model, ps, a)
        mean = torch.stack([w.double() for w in ws]).mean(0)
        dmax = max(float((w - a).abs().max()) for w in ws)
        bound = 2.0 ** -(f + 1) + 2.0 ** -24 * (4 * dmax + float(model.arena.master.abs().max()))
        err = float((model.arena.master.double() - mean).abs().max())
        print(f"secagg M={M} f={f}: max |out - mean| = {err:.3e} (bound {bound:.3e})")
        assert err <= bound


# ------------------------------------------------------------------ 5. plumbing and refusals
def _cfg(outdir, rounds, **kw):
    base = dict(out_dir=outdir, synthetic_rows=600, data_fraction=0.1, max_len=32, epochs=1, batch_size=8,
                eval_batch_size=16, plots=False, resume=False, rounds=rounds, verbose=False, heartbeat_s=0.0,
                save_checkpoints=False)
    base.update(kw)
    return config.FedConfig(**base)


def _client(cfg, frame):
    return runner.FederatedClient(cfg, frame=frame, model_config=models.DistilBertConfig(n_layers=1)).setup()


def test_config_env_and_cli_reach_the_runner(monkeypatch, tmp_path):
    d = config.FedConfig()
    assert (d.secagg, d.secagg_frac_bits, d.secagg_chacha_rounds, d.secagg_seed) == (False, 24, 20, None)
    parser = config.FedConfig.add_cli(argparse.ArgumentParser())
    cfg = config.FedConfig.from_args(parser.parse_args(
        ["--secagg", "true", "--secagg-frac-bits", "20", "--secagg-chacha-rounds", "12", "--secagg-seed", "7"]))
    assert (cfg.secagg, cfg.secagg_frac_bits, cfg.secagg_chacha_rounds, cfg.secagg_seed) == (True, 20, 12, 7)
    monkeypatch.setenv("FEDDDOS_SECAGG", "1")
    monkeypatch.setenv("FEDDDOS_SECAGG_CHACHA_ROUNDS", "8")
    monkeypatch.setenv("FEDDDOS_SECAGG_SEED", "99")
    cfg = config.FedConfig.from_args(parser.parse_args([]))
    assert (cfg.secagg, cfg.secagg_frac_bits, cfg.secagg_chacha_rounds, cfg.secagg_seed) == (True, 24, 8, 99)
    cfg = config.FedConfig.from_args(parser.parse_args(["--secagg-chacha-rounds", "20"]))  # flags win
    assert cfg.secagg and cfg.secagg_chacha_rounds == 20 and cfg.secagg_seed == 99
    _clear_rank_env()
    for k, v in dict(out_dir=str(tmp_path), synthetic_rows=600, max_len=32, plots=False, resume=False, verbose=False,
                     heartbeat_s=0.0).items():
        setattr(cfg, k, v)
    s = _client(cfg, None).secagg
    assert (s.frac_bits, s.rounds, s.seed) == (24, 20, 99) and s.private[0] == sa.private_key(99, 0)
    for k in ("FEDDDOS_SECAGG", "FEDDDOS_SECAGG_CHACHA_ROUNDS", "FEDDDOS_SECAGG_SEED"):
        monkeypatch.delenv(k)
    assert _client(_cfg(str(tmp_path), 1), None).secagg is None
    assert sa.make_secagg(_cfg(str(tmp_path), 1)) is None and sa.check_secagg_config(_cfg(str(tmp_path), 1)) is False
    assert sa.make_secagg(types.SimpleNamespace()) is None           # (a configuration from before the fields)
    assert sa.check_secagg_config(_cfg(str(tmp_path), 1, secagg=True)) is True
    two = _client(_cfg(str(tmp_path), 1, secagg=True, num_clients=2), None).secagg   # a virtual-client job: both pairs
    assert sorted(two.private) == [0, 1] and len(two.private[0]) == 32 and two.seed is None
    # refused at setup, before any work, with a message naming the flag
    for kw, match in ((dict(secagg=True, transport="tcp"), "transport"),
                      (dict(secagg=True, aggregator="median"), "aggregator"),
                      (dict(secagg=True, aggregator="trimmed_mean"), "aggregator"),
                      (dict(secagg=True, compress="int8"), "compress"), (dict(secagg=True, compress="topk"), "compress"),
                      (dict(secagg=True, weighted_fedavg=True), "weighted_fedavg"),
                      (dict(secagg=True, num_clients=17), "16"),
                      (dict(secagg=True, secagg_frac_bits=7), "secagg_frac_bits"),
                      (dict(secagg=True, secagg_frac_bits=31), "secagg_frac_bits"),
                      (dict(secagg_frac_bits=31), "secagg_frac_bits"),
                      (dict(secagg=True, secagg_chacha_rounds=10), "secagg_chacha_rounds"),
                      (dict(secagg_chacha_rounds=0), "secagg_chacha_rounds"),
                      (dict(secagg=True, secagg_seed=-1), "secagg_seed"), (dict(secagg_seed=1 << 64), "secagg_seed"),
                      (dict(secagg="yes"), "secagg")):
        with pytest.raises(ValueError, match=match):
            _client(_cfg(str(tmp_path), 1, **kw), None)
    with pytest.raises(ValueError, match="gpus_per_client"):
        sa.make_secagg(_cfg(str(tmp_path), 1, secagg=True), gpus_per_client=2)
    with pytest.raises(ValueError, match="gpus_per_client"):
        sa.check_secagg_config(_cfg(str(tmp_path), 1, secagg=True), 2)
    assert sa.check_secagg_config(_cfg(str(tmp_path), 1, secagg=True), 1, 16) is True
    for kw in (dict(frac_bits=31), dict(rounds=16), dict(seed=-1), dict(seed=1 << 64)):
        with pytest.raises(ValueError):
            sa.SecureAggregator(**kw)
    w, a = _vectors(128, seed=1)
    model = _model(w)
    agg = sa.SecureAggregator(seed=1)
    agg.setup_keys([0], 1)
    with pytest.raises(ValueError, match="anchor"):
        fedavg.fedavg_(model, secagg=agg)
    with pytest.raises(ValueError, match="robust"):
        fedavg.fedavg_(model, secagg=agg, anchor=a, robust=object())
    with pytest.raises(ValueError, match="compress"):
        fedavg.fedavg_(model, secagg=agg, anchor=a, compress=object())
    # one process: its own update through the fixed point, or nothing when it is not sampled
    assert fedavg.fedavg_(model, participate=False, secagg=agg, anchor=a) == 0.0 and agg.last is None
    sent = w.clone()
    assert fedavg.fedavg_(model, secagg=agg, anchor=a, client=0, round=2) == 1.0 and agg.last["masked_with"] == 0
    want = torch.empty(128)
    sa.torch_unmask_mean_([sa.torch_mask(sa.torch_encode(sent, a, 24)[0], NO_KEYS, 0)], a, want, None, 24)
    assert _bits(model.arena.master) == _bits(want) and float((want - sent).abs().max()) <= 2.0 ** -25 + 2.0 ** -23


# ------------------------------------------------------------------ 6. the default path
def _shape(msg):
    return re.sub(r"[-+]?\d[\d.e+-]*", "#", str(msg))


def test_secagg_off_is_the_path_without_it(tmp_path, monkeypatch):
    """2 virtual clients x 2 rounds with secagg off equal, bit for bit and log line for log line, the run
    of a client object that has no ``secagg`` attribute at all; nothing of the module is reached."""
    _clear_rank_env()
    frame = data_pkg.generate_cicids2017(600, seed=0)

    def boom(*a, **k):
        raise AssertionError("the default path reached secure aggregation")

    monkeypatch.setattr(sa.SecureAggregator, "mask_", boom)
    monkeypatch.setattr(sa.SecureAggregator, "unmask_mean_", boom)
    monkeypatch.setattr(sa.SecureAggregator, "setup_keys", boom)
    monkeypatch.setattr(sa, "torch_encode", boom)
    monkeypatch.setattr(sa, "x25519", boom)
    monkeypatch.setattr(fedavg, "_secagg_", boom)

    def run(strip):
        lines = []
        client = runner.FederatedClient(_cfg(str(tmp_path / f"s{int(strip)}"), 2, secagg=False), frame=frame,
                                        model_config=models.DistilBertConfig(n_layers=1))
        client.log.info = lambda msg, *a, **k: lines.append(msg)
        client.setup()
        assert client.secagg is None and client._round_anchor is None
        if strip:
            del client.secagg
            assert not hasattr(client, "secagg")
        return client, runner.run_virtual_clients(client, 2, rounds=2, progress=lines.append), lines

    (ca, ra, la), (cb, rb, lb) = _single_thread(lambda: (run(False), run(True)))
    assert _bits(ca.model.arena.master) == _bits(cb.model.arena.master)
    assert [_shape(m) for m in la] == [_shape(m) for m in lb] and len(la) > 4
    assert not any("secure aggregation" in str(m) or "masked" in str(m) for m in la)
    for ha, hb in zip(ra["rounds"], rb["rounds"]):
        assert not any(k in ha for k in SECAGG_KEYS)
        assert ha["aggregated_confusion"] == hb["aggregated_confusion"]
        for a, b in zip(ha["clients"], hb["clients"]):
            assert not any(k in a for k in SECAGG_KEYS)
            assert a["aggregated_test"] == b["aggregated_test"] and a["local_test"] == b["local_test"]
            assert a["train"]["epoch_losses"] == b["train"]["epoch_losses"]
    lines = []
    solo = runner.FederatedClient(_cfg(str(tmp_path / "solo"), 1), frame=frame,
                                  model_config=models.DistilBertConfig(n_layers=1))
    solo.log.info = lambda msg, *a, **k: lines.append(msg)
    solo.setup()
    rec = _single_thread(lambda: solo.run_round(0))
    assert not any(k in rec for k in SECAGG_KEYS) and solo._round_anchor is None
    assert not any("secure aggregation" in str(m) or "masked" in str(m) for m in lines)


# ------------------------------------------------------------------ 7. virtual == 2-rank gloo
def _fed_worker(rank, world, port, outdir, rounds, kw):
    os.environ.update({"RANK": str(rank), "WORLD_SIZE": str(world), "LOCAL_RANK": str(rank),
                       "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port)})
    comm = import_module(f"{PKG}.parallel.comm")
    comm.init_distributed(device="cpu")
    torch.set_num_threads(1)
    cfg = _cfg(outdir, rounds, **kw)
    frame = data_pkg.generate_cicids2017(cfg.synthetic_rows, seed=0)
    client = runner.FederatedClient(cfg, frame=frame, model_config=models.DistilBertConfig(n_layers=1))
    client.setup()
    for r in range(client.start_round, cfg.rounds):
        client.run_round(r)
    s = client.secagg
    torch.save({"master": client.model.arena.master.clone(), "history": client.history,
                "private": sorted(s.private), "public": dict(s.public),
                "pair": s.pair_words(rank, 1 - rank).tolist()}, os.path.join(outdir, f"state_rank{rank}.pt"))
    client.log.close()
    comm.shutdown()


def test_virtual_equals_two_rank_gloo_run(tmp_path):
    """tests/test_virtual_rounds.py's configuration with secure aggregation over 2 rounds: the virtual run
    and the 2-rank gloo run agree bit for bit -- weights and records -- though every process drew its keys
    from os.urandom: the result does not depend on the keys."""
    world, rounds = 2, 2
    real = tmp_path / "real"
    real.mkdir()
    kw = dict(synthetic_rows=1500, max_len=64, secagg=True, secagg_chacha_rounds=8)
    mp.spawn(_fed_worker, args=(world, _free_port(), str(real), rounds, kw), nprocs=world, join=True)
    _clear_rank_env()
    cfg = _cfg(str(tmp_path / "virtual"), rounds, num_clients=world, **kw)
    frame = data_pkg.generate_cicids2017(cfg.synthetic_rows, seed=0)

    def virtual():
        client = _client(cfg, frame)
        init = client.model.arena.master.clone()
        return client, init, runner.run_virtual_clients(client, world, rounds=rounds)

    client, init, res = _single_thread(virtual)
    st = [torch.load(real / f"state_rank{r}.pt", weights_only=False) for r in range(world)]
    assert torch.equal(st[0]["master"], st[1]["master"])
    assert torch.equal(st[0]["master"], client.model.arena.master) and not torch.equal(init, st[0]["master"])
    # each rank held its own private key alone, learned both public keys, and derived the same pair key
    assert st[0]["private"] == [0] and st[1]["private"] == [1]
    assert st[0]["public"] == st[1]["public"] and len(set(st[0]["public"].values())) == 2
    assert st[0]["pair"] == st[1]["pair"] and st[0]["public"][0] != client.secagg.public[0]
    n = client.model.arena.master.numel()
    for r in range(rounds):
        got = res["rounds"][r]
        assert got["payload_bytes"] == 4 * (n + 16) and got["masked_with"] == 1 and got["clamped"] == 0
        for rank in range(world):
            want, c = st[rank]["history"][r], got["clients"][rank]
            for k in SECAGG_KEYS:
                assert c[k] == want[k], (rank, r, k)
            assert c["bad_elems"] == 0 and 0 < c["quant_error_l2"] <= 2.0 ** -25 * math.sqrt(n) < c["update_l2"]
            assert c["aggregated_test"]["loss"] == want["aggregated_test"]["loss"], (rank, r)
            assert c["local_test"]["loss"] == want["local_test"]["loss"], (rank, r)


# ------------------------------------------------------------------ 7b. the key exchange over a native communicator
class _StubNativeComm:
    """``NativeComm.all_gather`` as far as a CPU can play it: the dtypes csrc/binding.cpp ``comm_dtype`` takes
    (fp32, bf16, fp64, int64, int32 -- no 8-bit type) and nothing else, the gather itself over gloo."""
    DTYPES = (torch.float32, torch.bfloat16, torch.float64, torch.int64, torch.int32)

    def __init__(self, world_size):
        self.world_size = world_size
        self.calls = []

    def all_gather(self, t, wait=True):
        import torch.distributed as dist
        if t.dtype not in self.DTYPES:
            raise RuntimeError(f"comm: unsupported dtype {t.dtype}")
        self.calls.append((t.dtype, tuple(t.shape)))
        out = torch.empty((self.world_size,) + tuple(t.shape), dtype=t.dtype)
        dist.all_gather(list(out.unbind(0)), t.contiguous())
        return out


def _keys_worker(rank, world, port, outdir):
    os.environ.update({"RANK": str(rank), "WORLD_SIZE": str(world), "LOCAL_RANK": str(rank),
                       "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port)})
    comm = import_module(f"{PKG}.parallel.comm")
    comm.init_distributed(device="cpu")
    out = {}
    for tag, c in (("native", _StubNativeComm(world)), ("torch", None)):
        s = sa.SecureAggregator(F, 8)
        s.setup_keys(rank, world, comm=c, device="cpu")
        out[tag] = {"private": sorted(s.private), "public": dict(s.public), "own": sa.public_key(s.private[rank]),
                    "pairs": {j: s.pair_words(rank, j).tolist() for j in range(world) if j != rank},
                    "derived": sorted(s._pair), "calls": c.calls if c is not None else None}
    torch.save(out, os.path.join(outdir, f"keys_rank{rank}.pt"))
    comm.shutdown()


def test_public_keys_travel_over_a_native_communicator(tmp_path):
    """``setup_keys(comm=)`` gathers the public keys through the communicator it is given, in a dtype
    ``NativeComm`` carries (its binding refuses uint8): one call of 8 int32 words, every rank learns every
    key byte for byte, and both ends of a pair derive the same pair key -- at setup, not in the first round."""
    world = 3
    mp.spawn(_keys_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    st = [torch.load(tmp_path / f"keys_rank{r}.pt", weights_only=False) for r in range(world)]
    for tag in ("native", "torch"):
        for r in range(world):
            got = st[r][tag]
            assert got["private"] == [r] and sorted(got["public"]) == list(range(world))
            assert got["public"] == st[0][tag]["public"] and got["public"][r] == got["own"]
            assert all(len(pk) == 32 for pk in got["public"].values())
            assert got["derived"] == [(r, j) for j in range(world) if j != r]
            for j in got["pairs"]:
                assert got["pairs"][j] == st[j][tag]["pairs"][r]
        assert len({st[0][tag]["public"][c] for c in range(world)}) == world
    assert all(st[r]["native"]["calls"] == [(torch.int32, (8,))] for r in range(world))
    assert st[0]["native"]["public"] != st[0]["torch"]["public"]            # (fresh keys per setup)
    with pytest.raises(ValueError):
        sa.gather_public_keys(bytes(31), 1)


# ------------------------------------------------------------------ 8. a dropped client
def _drop_worker(rank, world, port, outdir):
    os.environ.update({"RANK": str(rank), "WORLD_SIZE": str(world), "LOCAL_RANK": str(rank),
                       "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port)})
    comm = import_module(f"{PKG}.parallel.comm")
    comm.init_distributed(device="cpu")
    torch.set_num_threads(1)
    model = models.DDoSClassifier(config=models.DistilBertConfig(n_layers=1), device="cpu", impl="torch", seed=0)
    A = model.arena
    live = torch.zeros(A.numel, dtype=torch.bool)
    for off, shape in A.offsets.values():
        live[off:off + math.prod(shape)] = True
    s = sa.SecureAggregator(F, 8)
    s.setup_keys(rank, world)
    out = {}
    for r, participate in enumerate((True, rank != 1)):               # round 2: rank 1 is dropped
        anchor = A.master.clone()
        g = torch.Generator().manual_seed(10 * r + rank)
        with torch.no_grad():
            A.master.add_(1e-3 * torch.randn(A.numel, generator=g) * live)
        sent = A.master.clone()
        total = fedavg.fedavg_(model, participate=participate, comm=None, secagg=s, anchor=anchor, client=rank, round=r)
        out[r] = {"total": total, "anchor": anchor, "sent": sent, "master": A.master.clone(), "last": s.last}
    out["pads"] = bool(A.master[~live].view(torch.int32).any())
    torch.save(out, os.path.join(outdir, f"drop_rank{rank}.pt"))
    comm.shutdown()


def test_a_dropped_client(tmp_path):
    world = 3
    mp.spawn(_drop_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    st = [torch.load(tmp_path / f"drop_rank{r}.pt", weights_only=False) for r in range(world)]
    for r in range(2):
        assert all(torch.equal(st[0][r]["master"], st[k][r]["master"]) for k in (1, 2))   # the ranks stay identical
        assert all(st[k][r]["total"] == (3.0 if r == 0 else 2.0) for k in range(world))
    assert not any(st[k]["pads"] for k in range(world))
    # round 1: all three mask for two partners; round 2: ranks 0 and 2 for each other alone, rank 1 for nobody
    assert [st[k][0]["last"]["masked_with"] for k in range(world)] == [2, 2, 2]
    assert st[1][1]["last"] is None and st[0][1]["last"]["masked_with"] == st[2][1]["last"]["masked_with"] == 1
    want = torch.empty_like(st[0][0]["sent"])
    for r, live in ((0, (0, 1, 2)), (1, (0, 2))):
        plain = [sa.torch_mask(sa.torch_encode(st[k][r]["sent"], st[k][r]["anchor"], F)[0], NO_KEYS, 0) for k in live]
        sa.torch_unmask_mean_(plain, st[0][r]["anchor"], want, None, F)
        assert _bits(want) == _bits(st[0][r]["master"])


# ------------------------------------------------------------------ 9. composition
@pytest.mark.parametrize("kw,keys", [(dict(server_opt="adam", server_lr=0.01), ("delta_l2", "step_l2")),
                                     (dict(privacy_clip=0.01, privacy_noise=0.2, privacy_seed=SEED),
                                      ("privacy_epsilon",))])
def test_composes_with_the_other_features(tmp_path, kw, keys):
    _clear_rank_env()
    frame = data_pkg.generate_cicids2017(600, seed=0)
    client = _client(_cfg(str(tmp_path), 2, secagg=True, secagg_chacha_rounds=8, num_clients=2, **kw), frame)
    order = []
    if client.privacy is not None:
        real_priv = client.privacy.privatize_
        client.privacy.privatize_ = lambda *a, **k: (order.append("privatize"), real_priv(*a, **k))[1]
    real_mask = client.secagg.mask_
    client.secagg.mask_ = lambda *a, **k: (order.append("mask"), real_mask(*a, **k))[1]
    res = _single_thread(lambda: runner.run_virtual_clients(client, 2, rounds=2))
    assert bool(torch.isfinite(client.model.arena.master).all())
    if "privacy_clip" in kw:
        assert order == ["privatize", "mask"] * 4
    else:
        assert order == ["mask"] * 4 and client.server.rounds == 2
    for h in res["rounds"]:
        assert all(k in h for k in keys) and h["bad_elems"] == 0 and h["clamped"] == 0 and h["quant_error_l2"] > 0
        for c in h["clients"]:
            assert all(k in c for k in SECAGG_KEYS) and 0 < c["quant_error_l2"] < c["update_l2"] and c["masked_with"] == 1
            if "privacy_clip" in kw:   # privacy's update_l2 (before the clip) stays
                assert c["clipped"] == 1 and c["update_l2"] > 0.01
    # without it the same job ends within the fixed point's error of this one (same data, same seeds)
    if "privacy_clip" not in kw:
        plain = _client(_cfg(str(tmp_path / "plain"), 2, num_clients=2, **kw), frame)
        _single_thread(lambda: runner.run_virtual_clients(plain, 2, rounds=2))
        assert float((plain.model.arena.master - client.model.arena.master).abs().max()) < 1e-3


def test_run_round_order_log_and_record(tmp_path):
    """run_round in one process: privatize, then poison, then mask; the log lines and the record carry the
    secure-aggregation keys."""
    _clear_rank_env()
    frame = data_pkg.generate_cicids2017(600, seed=0)
    lines = []
    cfg = _cfg(str(tmp_path), 1, secagg=True, secagg_frac_bits=20, privacy_clip=1e-3, privacy_seed=SEED, poison_client=0,
               poison_kind="scale", poison_scale=1.0, verbose=False)
    client = runner.FederatedClient(cfg, frame=frame, model_config=models.DistilBertConfig(n_layers=1))
    client.log.info = lambda msg, *a, **k: lines.append(msg)
    client.setup()
    assert any("secure aggregation" in m and "20 fraction bits" in m and "ChaCha20" in m for m in lines)
    order = []
    real_priv, real_mask, real_poison = client.privacy.privatize_, client.secagg.mask_, runner.faults.poison_
    client.privacy.privatize_ = lambda *a, **k: (order.append("privatize"), real_priv(*a, **k))[1]
    client.secagg.mask_ = lambda *a, **k: (order.append("mask"), real_mask(*a, **k))[1]
    try:
        runner.faults.poison_ = lambda *a, **k: (order.append("poison"), real_poison(*a, **k))[1]
        rec = _single_thread(lambda: client.run_round(0))
    finally:
        runner.faults.poison_ = real_poison
    assert order == ["privatize", "poison", "mask"]
    n = client.model.arena.master.numel()
    assert rec["payload_bytes"] == 4 * (n + 16) and rec["masked_with"] == 0 and rec["clamped"] == 0 and rec["bad_elems"] == 0
    assert 0 < rec["quant_error_l2"] <= 2.0 ** -21 * math.sqrt(n) and rec["clipped"] == 1
    assert any("masked update" in m and "B sent" in m and "0 pair stream" in m for m in lines)
